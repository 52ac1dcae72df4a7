"""The guard-band harness of tests/util.py ("memory contract of the ABI") must be able to fail: planted stray writes and reads
on host arenas are reported at the right argument, band and byte; views and aliased operands are laid out as one span / one arena; every
CPU twin of oracle/var_oracle.c that tests/test_kernels_gpu.py::both reaches runs once on guarded host arenas (also under gcc's
AddressSanitizer where the machine has its runtime); and every entry point of the ABI that takes a device pointer is named in a guarded
call of the GPU suite."""
import ast
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from var_amd import abi

torch = pytest.importorskip('torch')

ORACLE_LIB_ENV = 'VAR_GUARD_ORACLE_LIB'             # the sanitizer run of this file binds the twins of this library instead


def _f32(p, n, first=0):
    """n floats of raw memory starting `first` elements after pointer p"""
    return np.frombuffer((ctypes.c_float * n).from_address(p.value + 4 * first), dtype=np.float32)


def _i64(p, n, first=0):
    return np.frombuffer((ctypes.c_int64 * n).from_address(p.value + 8 * first), dtype=np.int64)


MAKE = {'numpy': lambda a: a, 'torch': lambda a: torch.from_numpy(a)}


def test_band_length_rule():
    assert util.guard_band_bytes(1) == 4096 and util.guard_band_bytes(4097) == 4608 and util.guard_band_bytes(5000) == 5120
    assert util.guard_band_bytes(1 << 20) == 1 << 20 and util.guard_band_bytes(1 << 30) == 1 << 20
    # the largest window a descriptor declares in front of its operand (fp32 conv, 256 wide, 160 channels) is inside the cap
    assert (256 + 1) * 160 * 4 < util.GUARD_CAP
    x = np.zeros(100000, np.float32)
    (ar,), _ = util.guard_layout([x])
    assert ar.o0 >= ar.band == 400384 and ar.ptr(x.ctypes.data) % 512 == x.ctypes.data % 512
    assert len(ar.buf) - ar.o0 - ar.nbytes >= ar.band and ar.nbytes == 400000
    assert bool((ar.buf[:ar.o0] == 0xFF).all()) and bool((ar.buf[ar.o0 + ar.nbytes:] == 0xFF).all())
    for dt in (np.float16, np.float32, np.float64):
        assert np.isnan(np.full(8, 0xFF, np.uint8).view(dt)).all()
    assert np.isnan(torch.full((8,), 0xFF, dtype=torch.uint8).view(torch.bfloat16).float().numpy()).all()
    assert (np.full(8, 0xFF, np.uint8).view(np.int32) == -1).all() and (np.full(8, 0xFF, np.uint8).view(np.int64) == -1).all()


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_planted_stray_writes_are_reported_at_the_right_place(kind):
    mk = MAKE[kind]
    n = 1000
    x, y = mk(np.arange(n, dtype=np.float32)), mk(np.zeros(n, np.float32))
    band = util.guard_band_bytes(4 * n)

    def scale(xp, yp, n):                                    # the honest kernel
        _f32(yp, n)[:] = 2 * _f32(xp, n)
        return 0
    assert util.guarded_invoke('scale', [x, y, n], scale) == 0
    assert np.array_equal(np.asarray(y), 2 * np.arange(n, dtype=np.float32)) and np.array_equal(np.asarray(x), np.arange(n, dtype=np.float32))

    def one_before(xp, yp, n):
        _f32(yp, 1, -1)[0] = 1.0
        return scale(xp, yp, n)

    def one_after(xp, yp, n):
        _f32(yp, 1, n)[0] = 1.0
        return scale(xp, yp, n)

    def far_end(xp, yp, n):                                  # the last element of the band behind y
        _f32(yp, 1, n + band // 4 - 1)[0] = 1.0
        return scale(xp, yp, n)

    def into_input(xp, yp, n):                               # a store next to an INPUT operand
        _f32(xp, 2, n)[:] = 1.0
        return scale(xp, yp, n)

    for kern, arg, where, first, last in ((one_before, 1, 'front', -4, -1), (one_after, 1, 'back', 4 * n, 4 * n + 3),
                                          (far_end, 1, 'back', 4 * n + band - 4, 4 * n + band - 1), (into_input, 0, 'back', 4 * n, 4 * n + 7)):
        with pytest.raises(util.GuardError) as e:
            util.guarded_invoke(kern.__name__, [x, y, n], kern)
        (f,) = e.value.findings
        assert (f['name'], f['args'], f['band'], f['first'], f['last']) == (kern.__name__, [arg], where, first, last), f
        msg = str(e.value)
        assert kern.__name__ in msg and f'argument {arg}' in msg and ('in front of' if where == 'front' else 'behind') in msg and f'bytes {first} to {last}' in msg
    # the one store a band cannot see is its own pattern; the canonical quiet NaN (0x7FC00000) is not that pattern
    def nan_after(xp, yp, n):
        _f32(yp, 1, n)[0] = np.float32(np.nan)
        return 0
    with pytest.raises(util.GuardError):
        util.guarded_invoke('nan_after', [x, y, n], nan_after)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_planted_stray_reads_poison_the_result(kind):
    mk = MAKE[kind]
    n = 257
    x = mk(np.linspace(-1, 1, n).astype(np.float32)); s = mk(np.zeros(1, np.float32))

    def total(xp, sp, n, over):
        _f32(sp, 1)[0] = _f32(xp, n + over).sum(dtype=np.float64)
        return 0
    util.guarded_invoke('sum', [x, s, n, 0], total)
    assert abs(float(s[0]) - float(np.asarray(x, dtype=np.float64).sum())) < 1e-6
    util.guarded_invoke('sum one past', [x, s, n, 1], total)
    assert np.isnan(float(s[0])), 'a float read from a band must poison the sum'
    total(ctypes.c_void_p(util._addr(x)), ctypes.c_void_p(util._addr(s)), n, 0)           # (unguarded the stand-in is fine)
    assert np.isfinite(float(s[0]))

    # an index read one past an int64 input is -1: the gather then reads the last element of the band in front of the table (NaN)
    V = 64
    table = mk(np.arange(V, dtype=np.float32) * 3); idx = mk(np.arange(0, 2 * n, 2, dtype=np.int64) % V); out = mk(np.zeros(n, np.float32))

    def gather(tp, ip, op, n, shift):
        ii = _i64(ip, n, shift)
        o = _f32(op, n)
        for k in range(n):
            o[k] = _f32(tp, 1, int(ii[k]))[0]
        return 0
    util.guarded_invoke('gather', [table, idx, out, n, 0], gather)
    want = np.asarray(table)[np.asarray(idx)]
    assert np.array_equal(np.asarray(out), want)
    util.guarded_invoke('gather one past', [table, idx, out, n, 1], gather)
    got = np.asarray(out)
    assert np.array_equal(got[:-1], want[1:]) and np.isnan(got[-1]) and not np.array_equal(got, want)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_views_and_aliased_operands_layout_and_round_trip(kind):
    mk = MAKE[kind]
    G, C = 5, 48
    ada = mk(np.arange(G * 6 * C, dtype=np.float32).reshape(G, 6 * C))
    before = np.asarray(ada).copy()
    sc, sh = ada[:, 2 * C:], ada[:, 4 * C:]                  # the scale / shift rows of an AdaLN table: interior views with ld = 6C
    arenas, placed = util.guard_layout([sc, 6 * C, sh, 6 * C])
    (ar,) = arenas                                           # overlapping spans: one arena, from the first view's first to the last addressed element
    assert ar.positions == [0, 2] and ar.addr == util._addr(ada) + 4 * 2 * C and ar.nbytes == 4 * (G * 6 * C - 2 * C)
    assert {p[0]: p[3].ptr(p[1]) - ar.ptr(ar.addr) for p in placed} == {0: 0, 2: 4 * 2 * C}
    assert ar.ptr(ar.addr) % 512 == ar.addr % 512, 'an interior pointer keeps its misalignment'
    seen = {}

    def look(sp, ld, hp, ld2):
        seen['sc'] = _f32(sp, (G - 1) * ld + 4 * C).copy(); seen['d'] = hp.value - sp.value
        assert np.isnan(_f32(sp, 1, -1)[0]) and np.isnan(_f32(sp, 1, (G - 1) * ld + 4 * C)[0])       # bands on both sides of the span
        return 0
    util.guarded_invoke('look', [sc, 6 * C, sh, 6 * C], look)
    assert seen['d'] == 4 * 2 * C and np.array_equal(seen['sc'], before.reshape(-1)[2 * C:])
    assert np.array_equal(np.asarray(ada), before), 'round trip changed the caller\'s bytes'

    # in-place x (the same tensor as input and output) and a strided output: one arena, the kernel's writes come back, the gaps survive
    x = mk(np.arange(40, dtype=np.float32))

    def double_in_place(ip, op, n):
        assert ip.value == op.value
        _f32(op, n)[:] = 2 * _f32(ip, n)
        return 0
    arenas, _ = util.guard_layout([x, x, 40])
    assert len(arenas) == 1 and arenas[0].positions == [0, 1] and arenas[0].nbytes == 160
    util.guarded_invoke('double', [x, x, 40], double_in_place)
    assert np.array_equal(np.asarray(x), 2 * np.arange(40, dtype=np.float32))
    big = mk(np.full((6, 10), -7.0, np.float32)); v = big[1:5, 2:7]

    def fill_rows(op, rows, cols, ld):
        for r in range(rows):
            _f32(op, cols, r * ld)[:] = r
        return 0
    (ar,), _ = util.guard_layout([v])
    assert ar.nbytes == 4 * (3 * 10 + 5)
    util.guarded_invoke('fill', [v, 4, 5, 10], fill_rows)
    want = np.full((6, 10), -7.0, np.float32); want[1:5, 2:7] = np.arange(4, dtype=np.float32)[:, None]
    assert np.array_equal(np.asarray(big), want)
    # two arrays that do not overlap never share an arena; None and scalars pass through
    a, b = mk(np.zeros(8, np.float32)), mk(np.zeros(8, np.float32))
    arenas, _ = util.guard_layout([a, None, 3, b])
    assert [ar.positions for ar in arenas] in ([[0], [3]], [[3], [0]])
    util.guarded_invoke('none', [a, None, 3, b], lambda ap, n, k, bp: int(not (n is None and k == 3 and ap.value != bp.value)))


# ---------------------------------------------------------------------------------------------------------------------
def _oracle():
    path = os.environ.get(ORACLE_LIB_ENV)
    if path:
        return abi.bind(ctypes.CDLL(path), 'varref_', with_stream=False)
    util.ensure_oracle_built()
    from oracle import var_oracle
    return var_oracle.lib()


def _run_twins(monkeypatch):
    """every case function of tests/test_kernels_gpu.py that is written on both(), at the first ragged case of its list, with both()
    replaced by its host half: the twin alone, on guarded numpy arenas -> the set of twins that ran"""
    from tests import test_kernels_gpu as tk
    L = _oracle()
    ran = set()

    def host_both(name, args, outs):
        copies, arrays, ptrs = {}, [], []
        for a in args:
            off = 0
            if isinstance(a, tuple):
                a, off = a
            if isinstance(a, np.ndarray):
                ra = copies.setdefault(id(a), np.ascontiguousarray(a).copy())
                arrays.append(ra); ptrs.append(ra.reshape(-1)[off:])
            else:
                arrays.append(None); ptrs.append(a)
        rc = util.guarded_invoke(f'varref_{name}', ptrs, L[name])
        assert rc == 0, f'oracle {name} rc={rc}'
        ran.add(name)
        res = [arrays[i] for i in outs]
        return res, res
    monkeypatch.setattr(tk, 'both', host_both)
    import types
    helpers = types.SimpleNamespace(gn_scratch_elems=lambda *a: int(L['gn_scratch_elems'](*a)),             # the twins' own size helpers
                                    conv_gn_blocks=lambda H, W, C, phase=False: int(L['conv_gn_blocks'](H, W, C, int(phase))))
    monkeypatch.setattr(tk, '_setup', lambda: (L, helpers))
    tk.test_gemm_exact(25, 33, 25, 2); tk.test_gemm_exact(1, 128, 32, 0)
    tk.test_gemm_batched_bias_per_row_and_shared_operand()
    tk.test_qkv_prep_exact(4, 9, 2, 5, 14, 1)
    tk.test_gemm_qkv_fused_epilogue_exact(4, 4, 3, 192, 1, 14, 0)
    tk.test_adaln_block_composite_exact(4, 9, 2, 512, 5, 14, 1)
    tk.test_neighbor_table_exact(300, 5, 17)
    tk.test_smooth_select_exact(2, 9, 4096, 6, 3, None)
    tk.test_attn_cached_exact(4, 4, 2, 5, 14); tk.test_attn_cached_exact(1, 33, 1, 33, 33)
    tk.test_cfg_sample_exact(1, 7, 512, 1.0, 100, 0.9, 2.0, 0)
    tk.test_quant_step_exact(2, 2, 3)
    tk.test_gumbel_softmax_quant_h_and_token_select_exact()
    tk.test_encode_side_kernels_exact()
    tk.test_prologue_and_small_ops_exact()
    tk.test_conv3x3_exact(3, 5, 7, 64, 128, 0, 1, 0); tk.test_conv3x3_exact(2, 32, 32, 128, 64, 1, 0, 0); tk.test_conv3x3_exact(1, 40, 40, 160, 3, 0, 0, 1)
    tk.test_upconv_phase(2, 6, 6, 32, 32)
    tk.test_groupnorm(3, 100, 64)
    tk.test_softmax_rows_exact()
    for name in ('nearest_code_f32', 'nearest_code_cos_f32'):
        tk.test_nearest_code_exact(name, 7, 300, 8)
    tk.test_conv3x3_with_groupnorm_partials(3, 16, 8, 64, 64, 0)
    tk.test_upconv_phase_with_groupnorm_partials()
    rng = np.random.default_rng(0)
    M, C, rpg, ld = 37, 1024, 9, 6                                         # test_ln_modulate_exact's second case (its 16-bit half needs a GPU)
    G = (M + rpg - 1) // rpg
    x = tk.rnd(rng, M, C, scale=2.0) + 0.3; ada = tk.rnd(rng, G, ld * C, scale=0.5); out = np.zeros_like(x)
    tk.both('ln_modulate_f32', [x, (ada, 2 * C), ld * C, (ada, 4 * C), ld * C, out, M, C, rpg, 1e-6], [5])
    return ran


def test_every_twin_leaves_its_bands_intact(monkeypatch):
    ran = _run_twins(monkeypatch)
    assert ran == set(abi.SIGNATURES), f'twins not run on guarded arenas: {sorted(set(abi.SIGNATURES) - ran)}'


def test_every_twin_leaves_its_bands_intact_under_address_sanitizer(tmp_path):
    """the same run against an AddressSanitizer build of oracle/var_oracle.c (host code only), in a child interpreter that has the
    sanitizer's runtime loaded first: a stray access of a twin that stays inside an arena's bands is still inside numpy's allocation"""
    if os.environ.get(ORACLE_LIB_ENV):
        pytest.skip('this is the sanitizer run itself')
    cc = shutil.which('gcc')
    if cc is None:
        pytest.skip('no gcc on this machine')
    rt = subprocess.run([cc, '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip(f'gcc has no AddressSanitizer runtime here (-print-file-name=libasan.so -> {rt!r})')
    probe_c = tmp_path / 'probe.c'
    probe_c.write_text('int probe(int x) { return x + 1; }\n')
    r = subprocess.run([cc, '-fsanitize=address', '-fPIC', '-shared', '-o', str(tmp_path / 'probe.so'), str(probe_c)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f'gcc cannot link a one-line file with -fsanitize=address here: {r.stderr[-300:]}')
    so = str(tmp_path / 'libvar_oracle_asan.so')
    flags = '-O1 -g -fsanitize=address -fno-omit-frame-pointer -ffp-contract=off -fno-math-errno -mavx2 -mfma -mf16c -fopenmp -fPIC'.split()
    r = subprocess.run([cc, *flags, '-shared', '-o', so, os.path.join(util.ROOT, 'oracle', 'var_oracle.c'), '-lm'], capture_output=True, text=True)
    assert r.returncode == 0, f'oracle/var_oracle.c does not build with -fsanitize=address:\n{r.stderr[-3000:]}'
    pre = os.environ.get('LD_PRELOAD', '')
    env = dict(os.environ, LD_PRELOAD=rt + (':' + pre if pre else ''), ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=86', **{ORACLE_LIB_ENV: so})
    probe = subprocess.run([sys.executable, '-c', 'print(1)'], env=env, capture_output=True, text=True)
    if probe.returncode != 0 or probe.stdout.strip() != '1':
        pytest.skip(f'the interpreter does not start under the sanitizer runtime: {probe.stderr[-300:]}')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-p', 'no:cacheprovider', os.path.abspath(__file__), '-k', 'test_every_twin_leaves_its_bands_intact'],
                       env=env, cwd=util.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and '1 passed' in r.stdout, f'sanitizer run failed (exit {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}'


# ---------------------------------------------------------------------------------------------------------------------
# Coverage condition: every entry point that takes a device pointer is named in a both(...) or guarded_call(...) of the GPU suite.
NO_DEVICE_POINTER = {                                        # everything else var_amd/abi.py and var_amd/hip.py bind: no kernel may be listed here
    'version': 'returns the build string',
    'gn_scratch_elems': 'size helper: host arithmetic (its answer is tested by allocating exactly that much inside an arena)',
    'conv_gn_blocks': 'size helper: host arithmetic (likewise)',
    'conv16_gn_fusable': 'shape predicate: host arithmetic',
    'timing_enable': 'timing table switch', 'timing_select': 'timing table family mask', 'timing_reset': 'timing table', 'timing_read': 'timing table: host pointers',
    'timing_name': 'timing table family name',
    'gemm16_force_tile': 'test hook: tile choice', 'conv16_force_tile': 'test hook: tile choice', 'gemm16_persistent': 'test hook: kernel choice',
    'sampler_force_walk': 'test hook: top-p walk',
    'gemm_force_tile': 'test hook: tile choice', 'gemm_qkv_force_tile': 'test hook: tile choice', 'gemm_last_pick': 'test hook: reports the path of the latest dispatch',
    'gemm_last_evec': 'test hook: reports the epilogue switch of the latest dispatch',
    'conv16_last_pick': 'test hook: reports the kernel instantiation of the latest 16-bit convolution',
    'gemm16_deep': 'test hook: kernel choice', 'gemm16_last_pick': 'test hook: reports the kernel instantiations of the latest 16-bit GEMM',
    'quant_last_route': 'test hook: reports the kernel route of the latest quantizer-step, word-embed or nearest-code call',
    'attn16_last_waves': 'test hook: reports the waves per workgroup of the latest 16-bit attention launch',
    'attn_force_waves': 'test hook: waves per workgroup of the fp32 attention launches',
    'attn_last_waves': 'test hook: reports the waves per workgroup of the latest fp32 attention launch',
    'vq_stats_blocks': 'size helper: host arithmetic (the workgroup partials of varhip_vq_scale_stats_f32 for n elements)',
}
FLAVOURS = ('f16', 'bf16')


def _strings(node):
    """every string the expression can evaluate to as far as the source tells: constants, f-strings and 'prefix' + variable with the
    variable expanded over the 16-bit flavours.  The expansion does not look at what the variable is bound to: a flavour that no
    parametrize list names would still count as covered.  The coverage test below is therefore a necessary condition (no entry point is
    forgotten altogether), not a proof that every flavour runs."""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return [node.value]
    if isinstance(node, ast.JoinedStr):
        outs = ['']
        for v in node.values:
            parts = [v.value] if isinstance(v, ast.Constant) else list(FLAVOURS)
            outs = [o + p for o in outs for p in parts]
        return outs
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
        left, right = _strings(node.left) or list(FLAVOURS), _strings(node.right) or list(FLAVOURS)
        return [a + b for a in left for b in right]
    if isinstance(node, ast.IfExp):
        return _strings(node.body) + _strings(node.orelse)
    return []


def _bound_strings(fn, var):
    """the strings function `fn` binds to variable `var`: its parametrize lists, for loops and assignments (tuple assignments by position)"""
    got = []
    for dec in fn.decorator_list:
        if isinstance(dec, ast.Call) and len(dec.args) > 1 and var in [v.strip() for s in _strings(dec.args[0]) for v in s.split(',')]:
            got += [s for c in ast.walk(dec.args[1]) for s in _strings(c)]
    for n in ast.walk(fn):
        if isinstance(n, ast.For) and any(isinstance(t, ast.Name) and t.id == var for t in ast.walk(n.target)):
            got += [s for c in ast.walk(n.iter) for s in _strings(c)]
        elif isinstance(n, ast.Assign):
            for tgt in n.targets:
                if isinstance(tgt, ast.Name) and tgt.id == var:
                    got += _strings(n.value)
                elif isinstance(tgt, ast.Tuple) and isinstance(n.value, ast.Tuple):
                    got += [s for t, v in zip(tgt.elts, n.value.elts) if isinstance(t, ast.Name) and t.id == var for s in _strings(v)]
    return got


def _guarded_names(path):
    tree = ast.parse(open(path).read())
    names = set()
    for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Lambda))]:
        for call in [n for n in ast.walk(fn) if isinstance(n, ast.Call)]:
            f = call.func
            if not ((isinstance(f, ast.Name) and f.id in ('both', 'guarded_call')) or (isinstance(f, ast.Attribute) and f.attr in ('both', 'guarded_call'))) or not call.args:
                continue
            first = call.args[0]
            got = _strings(first)
            if not got and isinstance(first, ast.Name) and isinstance(fn, ast.FunctionDef):
                got = _bound_strings(fn, first.id)
            names.update(got)
    return names


def test_every_entry_point_with_a_device_pointer_is_called_guarded():
    table = {}
    for t in (abi.SIGNATURES, abi.SIGNATURES_F16, abi.SIGNATURES_BF16, abi.SIGNATURES_HIP_ONLY):
        table.update(t)
    assert all(abi.P in sig for sig in table.values()), 'an entry of the signature tables takes no pointer'
    # the exemption list is exactly what is bound beside the signature tables, and holds nothing from them
    assert not set(NO_DEVICE_POINTER) & set(table)
    bound = set(abi.bind(_AllSymbols(), 'varhip_', with_stream=True))
    assert bound - set(table) <= set(NO_DEVICE_POINTER), f'bound beside the tables and not exempted: {sorted(bound - set(table) - set(NO_DEVICE_POINTER))}'
    src = open(os.path.join(util.ROOT, 'var_amd', 'hip.py')).read()
    for name in NO_DEVICE_POINTER:
        assert name in bound or f'varhip_{name}' in src, f'{name} is exempted but nothing binds it'
    named = set()
    for path in sorted(glob.glob(os.path.join(util.ROOT, 'tests', 'test_*_gpu.py'))):
        named |= _guarded_names(path)
    missing = sorted(set(table) - named)
    assert not missing, f'entry points with a device pointer that no both(...) / guarded_call(...) of tests/test_*_gpu.py names: {missing}'


class _AllSymbols:
    """stands in for a loaded library: abi.bind() only sets attributes on what it looks up"""
    def __getattr__(self, name):
        f = type('F', (), {})()
        setattr(self, name, f)
        return f
