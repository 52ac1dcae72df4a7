"""Every kernel route of the quantizer step on a real MI355X (var_amd/csrc/quant.hip, the edit forms of var_amd/csrc/edit.hip): the LDS-staged
and the plain Phi kernels (k_phi_accum_lds up to 96 bytes under its 64 KiB limit, k_phi_accum / k_phi_accum_rest from the first shape past it),
k_word_embed32 and the generic k_word_embed, the MFMA nearest-code kernels and their generic fallbacks, at Cvae = 32 and off it.

The cases, operands, route predicates and float64 bars are tests/quantcases.py (validated on the twins alone by
tests/test_quant_dispatch_cpu.py).  Here every call runs with all operands in guard arenas (tests/util.py); the HIP result must equal the
oracle's twin bit for bit (the edit forms: the plain twin on the substituted rows), varhip_quant_last_route() must name the route the case
was built for, and the result must stay within the derived bar of the float64 reference — the twin walks the kernel's own fma chains,
float64 torch does not."""
import numpy as np
import pytest

from tests import quantcases as qc
from tests import util
from tests.test_kernels_gpu import _setup
from var_amd import abi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def dev_call(name, args, outs, expect=0):
    """varhip_<name> on device copies of `args` inside guard arenas (an arg may be (array, element_offset)) -> (output arrays, route)"""
    _, hip = _setup()
    copies, arrays, dargs = {}, [], []
    for a in args:
        off = 0
        if isinstance(a, tuple):
            a, off = a
        if isinstance(a, np.ndarray):
            da = copies.setdefault(id(a), torch.from_numpy(np.ascontiguousarray(a)).cuda())
            arrays.append(da); dargs.append(da.view(-1)[off:])
        else:
            arrays.append(None); dargs.append(a)
    if expect == 0:
        util.guarded_call(name, *dargs)
    else:
        rc = util.guarded_invoke(f'varhip_{name}', dargs, lambda *a: hip.lib().fn[name](*a, hip.current_stream()), torch.cuda.synchronize)
        assert rc == expect, f'varhip_{name} rc={rc}, expected {expect}'
    return [None if arrays[i] is None else arrays[i].cpu().numpy() for i in outs], hip.lib().so.varhip_quant_last_route()


def same_bits(name, got, want):
    gb, wb = qc.bits(got).reshape(-1), qc.bits(want).reshape(-1)
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, (f'{name}: {bad.size}/{gb.size} elements differ from the twin bit for bit, first at flat element {int(bad[0])}: '
                           f'got {np.asarray(got).reshape(-1)[bad[0]]!r} want {np.asarray(want).reshape(-1)[bad[0]]!r}')


@pytest.mark.parametrize('case', qc.phi_cases(), ids=lambda c: c['name'])
def test_phi_step_every_entry_point(case):
    L, _ = _setup()
    host = qc.host_call(L)
    b = qc.build_phi(case)
    for entry in qc.PHI_ENTRIES:
        name, args, outs, what = qc.phi_call(b, entry, 'twin')
        want = host(name, args, outs)
        name, args, outs, what = qc.phi_call(b, entry, 'hip')
        got, route = dev_call(name, args, outs)
        assert route == case['route'], f"{case['name']} {entry}: route {route}, expected {case['route']}"
        ref = qc.phi_reference(b, entry)
        for w, g, r in zip(what, got, want):
            same_bits(f"{case['name']} {entry} {w}", g, r)
            qc.within(f"{case['name']} {entry} {w}", g, *ref[w])


def _run_table(kind, cases=None):
    L, _ = _setup()
    host = qc.host_call(L)
    res = {}
    for c in cases if cases is not None else [c for c in qc.all_cases() if c['kind'] == kind]:
        b = qc.BUILD[kind](c)
        want = host(b.name, b.args, b.outs)
        got, route = dev_call(b.name, b.args, b.outs)
        if 'route' in c:
            assert route == c['route'], f"{c['name']}: route {route}, expected {c['route']}"
        for g, w in zip(got, want):
            same_bits(c['name'], g, w)
        res[c['name']] = (qc.VERIFY[kind](b, *got), got)
    return res


@pytest.mark.parametrize('P,pq', qc.NEXT_PQ)
def test_next_map(P, pq):
    """area pool + word embed at Cv 32 / 40 / 8 and C 128 / 300 / 64: pooled and both CFG halves of x_out"""
    _run_table('next', [c for c in qc.next_cases() if (c['P'], c['pq']) == (P, pq)])


def test_area_pool():
    _run_table('pool')


def test_word_embed_row_tail_and_generic_kernel():
    """k_word_embed32 with 18 rows (a full block across both images and a 2-row tail), with 8, with two column blocks (C = 300); the generic
    kernel at Cv 40 and 8 and at Cv 32 behind a misaligned word_w, which must give the aligned call's bits"""
    res = _run_table('embed')
    for c in qc.embed_cases():
        if c['Cv'] == 32 and c['w_off']:
            aligned = c['name'].replace(f"w+{c['w_off']}", 'w+0')
            same_bits(c['name'] + ' against the aligned call', res[c['name']][1][0], res[aligned][1][0])


@pytest.mark.parametrize('cos', [False, True], ids=['l2', 'cos'])
def test_nearest_code_alignment_fallbacks(cos):
    res = _run_table('nearest', [c for c in qc.nearest_cases() if c['cos'] == cos])
    for c in qc.nearest_cases():
        if c['cos'] == cos:
            excused, (idx,) = res[c['name']]
            assert excused <= 0.02, c['name']
            aligned = c['name'].replace(f"z+{c['z_off']} cb+{c['cb_off']}", 'z+0 cb+0')
            assert np.array_equal(idx, res[aligned][1][0]), f"{c['name']}: other indices than the aligned call"


def test_refused_calls_write_nothing():
    """Cv = 65, Cv = 0, pn > P, null taps with pn != P, null f_rest, ld_gt < pn * pn, null keep: VARHIP_EINVAL from every entry point, up / f_hat /
    f_rest still the sentinel, no band touched, the route hook unchanged; and Cv = 65 / 0 on the nearest-code calls, Cv = 0 on the maps"""
    _, hip = _setup()
    b = qc.build_phi(dict(kind='phi', name='refused', Cv=8, P=5, pn=2, B=2, ratio=0.5, route=qc.ROUTE_PHI_LDS))
    before = hip.lib().so.varhip_quant_last_route()
    def untouched(nm, outs, route):
        for r in outs:
            assert r is None or bool((qc.bits(r) == (qc.SENTINEL_BITS if r.dtype == np.float32 else -7)).all()), f'{nm}: a refused call wrote'
        assert route == before, f'{nm}: a refused call changed varhip_quant_last_route()'
    for nm, entry, ch in qc.einval_phi_cases():
        name, args, outs, what = qc.phi_call(b, entry, 'hip', refused=True, **ch)
        untouched(nm, *dev_call(name, args, outs, expect=abi.EINVAL))
    for kind, c, pos in (('nearest', qc.nearest_cases()[0], 5), ('nearest', qc.nearest_cases()[-1], 5), ('next', qc.next_cases()[0], 10),
                         ('pool', qc.pool_cases()[0], 5), ('embed', qc.embed_cases()[0], 8)):
        for Cv in ((65, 0) if kind == 'nearest' else (0,)):
            bb = qc.BUILD[kind](c)
            args = list(bb.args); args[pos] = Cv
            untouched(f"{c['name']} Cv={Cv}", *dev_call(bb.name, args, bb.outs, expect=abi.EINVAL))
