"""The engine's buffer plumbing without a GPU: the one table of what a buffer set holds, the one cache rule, the one GEMM
caller.

The expected tables below are literal.  They were transcribed from the four hand-written allocators of the revision before the spec
(d967b26: `_alloc_workspace`, `_mix_workspace`, `_bop_workspace`, `_tf_workspace`) for the tiny model — depth 2, C = 128, 2 heads,
patch_nums (1, 2, 3) (L = 14, widest scale 9 tokens, P = 3), V = 4096, Cvae = 32, hidden 512 — and checked against those allocators run with
the `meta` device.  The GEMM argument tuples are the ones that revision's call sites spelled out."""
import weakref
from types import SimpleNamespace

import pytest
import torch

from var_amd import engine, hip, workspace
from var_amd.abi import EPI_NONE, EPI_RESID
from var_amd.workspace import Dims, allocate, cached, keep_precision, sampler_rows, workspace_spec

F, I64 = torch.float32, torch.int64
ACT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def dims(shared_aln):
    return Dims(C=128, H=2, V=4096, Cvae=32, P=3, depth=2, hidden=512, shared_aln=shared_aln, L=14)


def adaln(R, shared_aln):
    """the AdaLN tables of R rows: per block [R, 6C] under shared_aln (plus the shared projection), else one [R, depth * 6C]"""
    return {'ada': ((2, R, 768), F), 'shared': ((R, 768), F)} if shared_aln else {'ada': ((R, 1536), F), 'shared': None}


def expected(variant, shared_aln, A):
    """{name: (shape, dtype)}; kc / vc: one tensor of that shape per block (2), the only zeroed ones"""
    if variant == 'sampling B=2':                                    # R = 2B = 4 rows, M = 36
        return {'x': ((36, 128), F), 'x2': ((36, 128), F), 'xn': ((36, 128), A), 'q': ((36, 128), A), 'att': ((36, 128), A), 'hid': ((36, 512), A),
                'logits': ((36, 4096), F), 'idx': ((18,), I64), 'lvl_pos': ((14, 128), F), 'cond': ((4, 128), F), 'cond_silu': ((4, 128), F),
                'hn': ((4, 256), F), **adaln(4, shared_aln), 'kc': ((4, 2, 14, 64), A), 'vc': ((4, 2, 14, 64), A),
                'f_hat': ((2, 3, 3, 32), F), 'up': ((2, 3, 3, 32), F), 'pooled': ((18, 32), F)}
    if variant == 'composed B=2 G=3':                                # R = 6 rows, M = 54; x, cond, cond_silu at 2x
        return {'x': ((108, 128), F), 'x2': ((54, 128), F), 'xn': ((54, 128), A), 'q': ((54, 128), A), 'att': ((54, 128), A), 'hid': ((54, 512), A),
                'logits': ((54, 4096), F), 'idx': ((18,), I64), 'lvl_pos': ((14, 128), F), 'cond': ((12, 128), F), 'cond_silu': ((12, 128), F),
                'hn': ((6, 256), F), **adaln(6, shared_aln), 'kc': ((6, 2, 14, 64), A), 'vc': ((6, 2, 14, 64), A),
                'f_hat': ((2, 3, 3, 32), F), 'up': ((2, 3, 3, 32), F), 'pooled': ((18, 32), F), 'masked': ((18, 4096), F), 'mixed': ((36, 4096), F)}
    if variant == 'best-of-pruned stage cap=4':                      # R = 8 rows, M = 72
        return {'x': ((72, 128), F), 'x2': ((72, 128), F), 'xn': ((72, 128), A), 'q': ((72, 128), A), 'att': ((72, 128), A), 'hid': ((72, 512), A),
                'logits': ((72, 4096), F), 'idx': ((36,), I64), 'lvl_pos': ((14, 128), F), 'cond': ((8, 128), F), 'cond_silu': ((8, 128), F),
                'hn': ((8, 256), F), **adaln(8, shared_aln), 'kc': ((8, 2, 14, 64), A), 'vc': ((8, 2, 14, 64), A),
                'f_hat': ((4, 3, 3, 32), F), 'up': ((4, 3, 3, 32), F), 'pooled': ((36, 32), F), 'masked': ((36, 4096), F)}
    if variant == 'teacher-forced R=3 last scale':                   # 9 tokens a row, M = 27, caches of 14; x, cond, cond_silu at 2x
        return {'x': ((54, 128), F), 'x2': ((27, 128), F), 'xn': ((27, 128), A), 'q': ((27, 128), A), 'att': ((27, 128), A), 'hid': ((27, 512), A),
                'lg': ((27, 4096), F), 'lvl_pos': ((14, 128), F), 'cond': ((6, 128), F), 'cond_silu': ((6, 128), F),
                'hn': ((3, 256), F), **adaln(3, shared_aln), 'kc': ((3, 2, 14, 64), A), 'vc': ((3, 2, 14, 64), A), 'Lmax': 14}
    if variant == 'teacher-forced R=3 scale 1':                      # 4 tokens a row, M = 12, caches of 1 + 4 = 5
        return {'x': ((24, 128), F), 'x2': ((12, 128), F), 'xn': ((12, 128), A), 'q': ((12, 128), A), 'att': ((12, 128), A), 'hid': ((12, 512), A),
                'lg': ((12, 4096), F), 'lvl_pos': ((14, 128), F), 'cond': ((6, 128), F), 'cond_silu': ((6, 128), F),
                'hn': ((3, 256), F), **adaln(3, shared_aln), 'kc': ((3, 2, 5, 64), A), 'vc': ((3, 2, 5, 64), A), 'Lmax': 5}
    raise KeyError(variant)


# what SamplingEngine hands workspace_spec for each variant: (R, lmax, Lkv, what it needs on top)
ASKED = {
    'sampling B=2': (4, 9, 14, dict(B=2)),
    'composed B=2 G=3': (6, 9, 14, dict(B=2, twin=True, masked=True, mixed=True)),
    'best-of-pruned stage cap=4': (8, 9, 14, dict(B=4, masked=True)),
    'teacher-forced R=3 last scale': (3, 9, 14, dict(twin=True, logits='lg', Lmax=True)),
    'teacher-forced R=3 scale 1': (3, 4, 5, dict(twin=True, logits='lg', Lmax=True)),
}


def flat(spec):
    """a spec as the expected tables write it: (shape, dtype) with the per-block entries' leading depth checked and dropped"""
    out = {}
    for name, v in spec.items():
        if isinstance(v, tuple):
            shape, dt, zeroed = v
            assert zeroed == (name in ('kc', 'vc')), name
            if name in workspace.PER_BLOCK:
                assert shape[0] == 2
                shape = shape[1:]
            v = (tuple(shape), dt)
        out[name] = v
    return out


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('shared_aln', [False, True])
@pytest.mark.parametrize('variant', list(ASKED))
def test_spec_equals_the_literal_table(variant, shared_aln, prec):
    R, lmax, Lkv, on_top = ASKED[variant]
    spec = workspace_spec(dims(shared_aln), ACT[prec], R, lmax, Lkv, **on_top)
    want = expected(variant, shared_aln, ACT[prec])
    assert flat(spec) == want
    ws = allocate(spec, torch.device('meta'))
    assert set(ws) == set(want) | {'dev'} and ws['dev'] == torch.device('meta')
    for name, v in want.items():
        if name in ('kc', 'vc'):
            assert isinstance(ws[name], list) and [(tuple(t.shape), t.dtype) for t in ws[name]] == [v, v]
        elif isinstance(v, tuple):
            assert (tuple(ws[name].shape), ws[name].dtype) == v, name
        else:
            assert ws[name] is v or ws[name] == v


def test_the_shapes_most_likely_to_go_wrong():
    d, A = dims(False), torch.bfloat16
    spec = {k: workspace_spec(d, A, *ASKED[k][:3], **ASKED[k][3]) for k in ASKED}
    M = lambda k: ASKED[k][0] * ASKED[k][1]
    assert spec['sampling B=2']['x'][0] == (M('sampling B=2'), 128) == (36, 128)                        # the B labels' twins are its own CFG rows
    for k in ('composed B=2 G=3', 'teacher-forced R=3 last scale', 'teacher-forced R=3 scale 1'):
        assert spec[k]['x'][0] == (2 * M(k), 128) and spec[k]['x2'][0] == (M(k), 128)
    assert spec['teacher-forced R=3 last scale']['cond'][0] == spec['teacher-forced R=3 last scale']['cond_silu'][0] == (2 * 3, 128)
    assert spec['composed B=2 G=3']['cond'][0] == spec['composed B=2 G=3']['cond_silu'][0] == (2 * 3 * 2, 128)
    assert spec['composed B=2 G=3']['mixed'][0] == (2 * 2 * 9, 4096)
    for k in ASKED:
        assert spec[k]['hn'][0] == (ASKED[k][0], 2 * 128)
        assert spec[k]['kc'][0] == spec[k]['vc'][0] == (2, ASKED[k][0], 2, ASKED[k][2], 64) and spec[k]['kc'][1:] == (A, True)
    assert spec['teacher-forced R=3 scale 1']['kc'][0][3] == 5 and spec['teacher-forced R=3 scale 1']['Lmax'] == 5
    # the buffers _masked adds on first use come from the same table
    rows = sampler_rows(d, 2, 9)
    assert {k: v[:2] for k, v in rows.items()} == {'masked': ((18, 4096), F), 'probs': ((18, 4096), F), 'h': ((18, 32), F)}
    assert spec['composed B=2 G=3']['masked'] == rows['masked']


# ---- the engine asks for what ASKED says -------------------------------------------------------------------------------------------------
class _Var:
    """the attributes of a VAR module that the workspace methods read"""
    C, num_heads, V, Cvae, depth, L, shared_aln = 128, 2, 4096, 32, 2, 14, False
    patch_nums, begin_ends = (1, 2, 3), [(0, 1), (1, 5), (5, 14)]
    pos_start = torch.empty(0, device='meta')
    blocks = [type('B', (), {'ffn': type('F', (), {'fc1': type('L', (), {'weight': torch.empty(512, 128, device='meta')})})})]


def _engine(monkeypatch, stream=0):
    eng = object.__new__(engine.SamplingEngine)
    eng.var, eng.policy, eng.precision, eng.dec, eng._ws, eng._ws_tf, eng._ws_bop = _Var, 'auto', 'f32', SimpleNamespace(), {}, {}, {}
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: type('S', (), {'cuda_stream': stream}))
    return eng


def test_the_engine_asks_for_the_five_variants(monkeypatch):
    eng = _engine(monkeypatch)
    for prec in ('f32', 'bf16'):
        eng.precision = prec
        got = {'sampling B=2': eng.workspace(2), 'composed B=2 G=3': eng._mix_workspace(2, 3), 'best-of-pruned stage cap=4': eng._bop_workspace(4, 1),
               'teacher-forced R=3 last scale': eng._tf_workspace(3), 'teacher-forced R=3 scale 1': eng._tf_workspace(3, 1)}
        for variant, ws in got.items():
            want = expected(variant, False, ACT[prec])
            assert set(ws) == set(want) | {'dev'}, variant
            for name, v in want.items():
                t = ws[name][0] if name in ('kc', 'vc') else ws[name]
                assert ((tuple(t.shape), t.dtype) if isinstance(v, tuple) else t) == v, (variant, name)
        assert eng._masked(got['sampling B=2'], 2, True) is got['sampling B=2']['masked']
        assert {k: tuple(got['sampling B=2'][k].shape) for k in ('masked', 'probs', 'h')} == {'masked': (18, 4096), 'probs': (18, 4096), 'h': (18, 32)}
    assert list(eng._ws) == [(2, 0, 'f32'), (2, 0, 'f32', 3), (2, 0, 'bf16'), (2, 0, 'bf16', 3)]
    assert list(eng._ws_bop) == [(4, 0, 'f32', 1), (4, 0, 'bf16', 1)]
    assert list(eng._ws_tf) == [(3, 0, 'f32', 14), (3, 0, 'f32', 5), (3, 0, 'bf16', 14), (3, 0, 'bf16', 5)]
    assert eng.workspace(2) is eng._ws[(2, 0, 'bf16')]
    eng.set_precision('f32')                                    # an explicit switch away from the last call's bf16
    assert all(k[2] == 'f32' for c in (eng._ws, eng._ws_tf, eng._ws_bop) for k in c) and len(eng._ws) == 2 and len(eng._ws_tf) == 2 and len(eng._ws_bop) == 1


# ---- the cache rule ---------------------------------------------------------------------------------------------------------------------------
class _Set:
    pass


class Alloc:
    """a counting allocator whose sets can be watched dying; before_alloc runs first, inside the call"""

    def __init__(self, dev='d0'):
        self.n, self.dev, self.before_alloc = 0, dev, lambda: None

    def __call__(self):
        self.before_alloc()
        self.n += 1
        return {'dev': self.dev, 'n': self.n, 'buf': _Set()}


def test_a_second_size_replaces_the_first_before_the_allocator_runs():
    cache, alloc = {}, Alloc()
    first = cached(cache, 8, (0, 'f32'), 6, 'd0', alloc)
    assert cached(cache, 8, (0, 'f32'), 6, 'd0', alloc) is first and alloc.n == 1
    dead = weakref.ref(first['buf'])
    del first

    def check():
        assert (8, 0, 'f32') not in cache and dead() is None, 'the replaced set was still alive when the new one was allocated'
    alloc.before_alloc = check
    second = cached(cache, 4, (0, 'f32'), 6, 'd0', alloc)
    assert alloc.n == 2 and list(cache) == [(4, 0, 'f32')] and cache[(4, 0, 'f32')] is second


def test_streams_precisions_and_slot_values_coexist():
    cache, alloc = {}, Alloc()
    slots = [(0, 'f32'), (1, 'f32'), (0, 'bf16'), (0, 'f32', 3), (0, 'f32', 4)]         # stream | precision | G, L_e or stage
    sets = [cached(cache, 8, s, 6, 'd0', alloc) for s in slots]
    assert alloc.n == 5 and list(cache) == [(8,) + s for s in slots]
    assert [cached(cache, 8, s, 6, 'd0', alloc) for s in slots] == sets and alloc.n == 5
    cached(cache, 2, (0, 'f32', 3), 6, 'd0', alloc)                                     # another size in one slot touches that slot alone
    assert list(cache) == [(8, 0, 'f32'), (8, 1, 'f32'), (8, 0, 'bf16'), (8, 0, 'f32', 4), (2, 0, 'f32', 3)]


def test_the_bound_evicts_oldest_first():
    cache, alloc = {}, Alloc()
    for sid in range(6):
        cached(cache, 8, (sid, 'f32'), 6, 'd0', alloc)
    assert len(cache) == 6
    cached(cache, 8, (0, 'f32'), 6, 'd0', alloc)                                          # a hit makes nothing younger and evicts nothing
    assert alloc.n == 6
    alloc.before_alloc = lambda: len(cache) == 5 or pytest.fail('the allocator ran with the cache full')
    cached(cache, 8, (6, 'f32'), 6, 'd0', alloc)
    assert list(cache) == [(8, sid, 'f32') for sid in range(1, 7)]
    cached(cache, 4, (3, 'f32'), 6, 'd0', alloc)                                          # replacing in a slot frees its place: nobody else goes
    assert list(cache) == [(8, 1, 'f32'), (8, 2, 'f32'), (8, 4, 'f32'), (8, 5, 'f32'), (8, 6, 'f32'), (4, 3, 'f32')]


def test_a_device_change_reallocates():
    cache, alloc = {}, Alloc('d0')
    first = cached(cache, 8, (0, 'f32'), 6, 'd0', alloc)
    dead = weakref.ref(first['buf'])
    del first
    alloc.dev = 'd1'
    alloc.before_alloc = lambda: dead() is None or pytest.fail("the other device's set was alive during the allocation")
    moved = cached(cache, 8, (0, 'f32'), 6, 'd1', alloc)
    assert alloc.n == 2 and moved['dev'] == 'd1' and list(cache) == [(8, 0, 'f32')]
    assert cached(cache, 8, (0, 'f32'), 6, 'd1', alloc) is moved and alloc.n == 2


def test_dropping_by_precision_keeps_only_that_precision():
    cache, alloc = {}, Alloc()
    for slot in [(0, 'f32'), (0, 'bf16'), (0, 'f16', 3), (1, 'bf16', 5)]:
        cached(cache, 8, slot, 6, 'd0', alloc)
    keep_precision(cache, 'bf16')
    assert list(cache) == [(8, 0, 'bf16'), (8, 1, 'bf16', 5)]
    keep_precision(cache, 'f32')
    assert cache == {}


def test_the_stage_cache_evicts_nothing_from_the_plain_one(monkeypatch):
    eng = _engine(monkeypatch)
    plain = eng.workspace(3)
    for stage in range(3):
        eng._bop_workspace(4, stage)
    for stream in range(1, 5):                                   # 4 * len(patch_nums) = 12 sets at most, the oldest go first
        monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, s=stream: type('S', (), {'cuda_stream': s}))
        for stage in range(3):
            eng._bop_workspace(4, stage)
    assert len(eng._ws_bop) == 12 and list(eng._ws_bop)[0] == (4, 1, 'f32', 0)
    assert list(eng._ws) == [(3, 0, 'f32')] and eng._ws[(3, 0, 'f32')] is plain


# ---- the GEMM caller --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(hip, 'call', lambda name, *args, stream=None: log.append((name,) + args))
    return log


def same(got, want):
    return len(got) == len(want) and all(a is b if isinstance(b, torch.Tensor) else (type(a) is type(b) and a == b) for a, b in zip(got, want))


def test_gemm_f32_forms(calls):
    A, W, bias, out, resid, gamma = (torch.empty(1) for _ in range(6))
    M, N, K, Cc, HW, B, D6 = 10, 24, 16, 64, 9, 2, 1536
    # plain: the per-block AdaLN projection into a strided view
    engine.gemm_nt('f32', A, W, bias, out, M, 768, 128, lda=128, ldw=128, ldo=D6)
    assert same(calls[-1], ('gemm_nt_f32', A, 128, W, 128, bias, out, D6, M, 768, 128, EPI_NONE, None, 0, None, 0, 1, 0, 1, 0, 0, 0))
    # residual + gamma: SamplingEngine.gemm, which hands N over as the residual's stride whether there is one or not
    eng = object.__new__(engine.SamplingEngine)
    W2 = torch.empty(N, K)
    eng.gemm(A, W2, bias, out, M, epi=EPI_RESID, resid=resid, gamma=gamma, ldg=6 * N, rpg=9)
    assert same(calls[-1], ('gemm_nt_f32', A, K, W2, K, bias, out, N, M, N, K, EPI_RESID, resid, N, gamma, 6 * N, 9, 0, 1, 0, 0, 0))
    eng.gemm(A, W2, None, out, M)
    assert same(calls[-1], ('gemm_nt_f32', A, K, W2, K, None, out, N, M, N, K, EPI_NONE, None, N, None, 0, 1, 0, 1, 0, 0, 0))
    # bias per row + batch: the decoder attention's V^T projection
    engine.gemm_nt('f32', W, A, bias, out, Cc, HW, Cc, lda=Cc, ldw=Cc, ldo=HW, bias_per_row=1, batch=B, sA=0, sW=HW * Cc, sO=Cc * HW)
    assert same(calls[-1], ('gemm_nt_f32', W, Cc, A, Cc, bias, out, HW, Cc, HW, Cc, EPI_NONE, None, 0, None, 0, 1, 1, B, 0, HW * Cc, Cc * HW))
    assert len(calls) == 4


@pytest.mark.parametrize('prec', ['f16', 'bf16'])
def test_gemm_16_bit_forms(calls, prec):
    dt = engine.DT16[prec]
    A, W = torch.empty(1, dtype=dt), torch.empty(1, dtype=dt)
    bias, out32, res32 = (torch.empty(1) for _ in range(3))
    out16, res16 = torch.empty(1, dtype=dt), torch.empty(1, dtype=dt)
    Cc, HW, B = 64, 64, 2
    name = 'gemm_nt_' + prec
    # 16-bit output, no residual: the q / k projection
    engine.gemm_nt(prec, A, W, bias, out16, B * HW, 2 * Cc, Cc, lda=Cc, ldw=Cc, ldo=2 * Cc)
    assert same(calls[-1], (name, A, Cc, W, Cc, bias, out16, 2 * Cc, 1, B * HW, 2 * Cc, Cc, EPI_NONE, None, 0, 0, None, 0, 1, 1, 0, 0, 0))
    # fp32 output, batched: the scores
    engine.gemm_nt(prec, A, W, None, out32, HW, HW, Cc, lda=2 * Cc, ldw=2 * Cc, ldo=HW, batch=B, sA=HW * 2 * Cc, sW=HW * 2 * Cc, sO=HW * HW)
    assert same(calls[-1], (name, A, 2 * Cc, W, 2 * Cc, None, out32, HW, 0, HW, HW, Cc, EPI_NONE, None, 0, 0, None, 0, 1, B, HW * 2 * Cc, HW * 2 * Cc, HW * HW))
    # 16-bit output + 16-bit residual: proj_out
    engine.gemm_nt(prec, A, W, bias, out16, B * HW, Cc, Cc, lda=Cc, ldw=Cc, ldo=Cc, epi=EPI_RESID, resid=res16, ldr=Cc)
    assert same(calls[-1], (name, A, Cc, W, Cc, bias, out16, Cc, 1, B * HW, Cc, Cc, EPI_RESID, res16, Cc, 1, None, 0, 1, 1, 0, 0, 0))
    # fp32 output + fp32 residual, and 16-bit output + fp32 residual
    engine.gemm_nt(prec, A, W, bias, out32, B * HW, Cc, Cc, lda=Cc, ldw=Cc, ldo=Cc, epi=EPI_RESID, resid=res32, ldr=Cc)
    assert same(calls[-1], (name, A, Cc, W, Cc, bias, out32, Cc, 0, B * HW, Cc, Cc, EPI_RESID, res32, Cc, 0, None, 0, 1, 1, 0, 0, 0))
    engine.gemm_nt(prec, A, W, bias, out16, B * HW, Cc, Cc, lda=Cc, ldw=Cc, ldo=Cc, epi=EPI_RESID, resid=res32, ldr=Cc)
    assert same(calls[-1], (name, A, Cc, W, Cc, bias, out16, Cc, 1, B * HW, Cc, Cc, EPI_RESID, res32, Cc, 0, None, 0, 1, 1, 0, 0, 0))
    n = len(calls)
    with pytest.raises(ValueError, match='per-row bias'):
        engine.gemm_nt(prec, A, W, bias, out16, Cc, HW, Cc, lda=Cc, ldw=Cc, ldo=HW, bias_per_row=1)
    assert len(calls) == n


def test_record_and_pointer_helpers():
    rec = engine.stats_record((2, 3), 'cpu')
    assert tuple(rec) == engine.STATS_FIELDS and all(tuple(t.shape) == (2, 3) for t in rec.values())
    assert {k: t.dtype for k, t in rec.items()} == {k: torch.int32 if k == 'kept' else torch.float32 for k in engine.STATS_FIELDS}
    rec = engine.stats_record((2, 1, 3), 'cpu', fill=(-1, float('nan')), fields=engine.STATS_FIELDS[1:])
    assert tuple(rec) == engine.STATS_FIELDS[1:] and bool((rec['kept'] == -1).all()) and all(bool(t.isnan().all()) for k, t in rec.items() if k != 'kept')
    bufs = [torch.empty(4), torch.empty(2)]
    tab = engine.pointer_table(bufs)
    assert tab.dtype == torch.int64 and tab.device.type == 'cpu' and tab.tolist() == [t.data_ptr() for t in bufs]
