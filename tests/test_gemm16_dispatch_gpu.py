"""Every kernel varhip_gemm_nt_{f16,bf16} and varhip_gemm_qkv_{f16,bf16} can launch (var_amd/csrc/gemm16.hip) — k_gemm16<4,4>, <1,1,2,2,4>,
<2,2,2,2,4>, <2,2>, <6,4,2,4>, <8,4,2,4>, the persistent k_gemm16p, the q/k/v kernels <1,4,2,2,3>, <2,4,2,2,3>, <2,4>, and the two-launch row
split — on the table of tests/gemm16cases.py (validated without a GPU by tests/test_gemm16_dispatch_cpu.py), in both 16-bit flavours.

After every call varhip_gemm16_last_pick(0 / 1) must name the kernels the case was built for (a forced tile is a request; a forced 2 that fell
through to the one-tile kernel, a "tile 1" that ran the 32x32 kernel instead of the 64x64 one, a split that did not happen fail here).  Then
every buffer the call writes — out with its padding, q_out and both caches — NaN-filled before the call, must EQUAL the float64 reference
cast once, bit for bit: the operands lie on a dyadic grid on which every partial sum is exact in fp32 in any order, so the rounding point,
the place of the bias, gamma and the residual, the row group, the (image, position) decode and every store address are pinned on every
kernel.  GELU and l2norm = 1 keep their bars against float64 and must be bit-equal across every kernel that can run the same call."""
import pytest

from tests import gemm16cases as gc
from tests import gemmcases
from tests import util

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

LAUNCHES = {}                                        # (entry, flavour, code) -> launches, from the hook (each test prints its own: run with -s)


def _hip():
    from var_amd import hip
    return hip


def _reset(so):
    so.varhip_gemm16_force_tile(-1); so.varhip_gemm16_persistent(1); so.varhip_gemm16_deep(1)


@pytest.fixture(autouse=True)
def hooks_reset():
    yield
    _reset(_hip().lib().so)


def _call(c, flav, o, outs):
    """the case's call under its switches, every operand in a guard arena -> (launch 0, launch 1) of varhip_gemm16_last_pick"""
    hip = _hip()
    so = hip.lib().so
    dt = gc.DTYPE[flav]
    g = gc.geometry(c)
    M, N, K, B = c['M'], c['N'], c['K'], c['batch']
    A = gc.place(o.A, g['lda'], g['sA'], dt).cuda()
    W = gc.place(o.W, g['ldw'], g['sW'], dt).cuda()
    bias = o.bias.float().cuda()
    so.varhip_gemm16_force_tile(c['tile']); so.varhip_gemm16_persistent(c['persist']); so.varhip_gemm16_deep(c['deep'])
    try:
        if c['entry'] == 'qkv':
            smul = o.smul.cuda() if c['l2'] else None
            util.guarded_call('gemm_qkv_' + flav, A, g['lda'], W, g['ldw'], bias, M, c['H'] * 64, K, smul, gc.Q_PLAIN, c['l2'],
                              outs['q'], outs['kc'], outs['vc'], c['B2'], c['l'], c['H'], c['pos0'], c['Lmax'])
        else:
            resid = gamma = None
            if o.resid is not None:
                resid = gc.place(o.resid[None], g['ldr'], 0, dt if c['resid'] == 16 else torch.float32).cuda()
            if o.gamma is not None:
                gamma = gc.place(o.gamma[None].float(), g['ldg'], 0, torch.float32).cuda()
            batched = B > 1
            util.guarded_call('gemm_nt_' + flav, A, g['lda'], W, g['ldw'], bias, outs['out'], g['ldo'], c['out16'], M, N, K,
                              {'none': 0, 'gelu': 1, 'resid': 2}[c['epi']], resid, g['ldr'], int(c['resid'] == 16), gamma, g['ldg'], c['rpg'], B,
                              g['sA'] if batched else 0, g['sW'] if batched else 0, g['sO'] if batched else 0)
        return so.varhip_gemm16_last_pick(0), so.varhip_gemm16_last_pick(1)
    finally:
        _reset(so)


def _fresh(c, flav):
    dts = {'out': gc.out_dtype(c, flav), 'q': gc.DTYPE[flav], 'kc': gc.DTYPE[flav], 'vc': gc.DTYPE[flav]}
    return {nm: torch.full((n,), gc.NAN, dtype=dts[nm], device='cuda') for nm, n in gc.buffer_sizes(c).items()}


def _count(c, flav, picks):
    for p in picks:
        if p:
            LAUNCHES[(c['entry'], flav, p)] = LAUNCHES.get((c['entry'], flav, p), 0) + 1


def _assert_bits(c, nm, got, want):
    gb, wb = gc.bits(got), gc.bits(want)
    if torch.equal(gb, wb):
        return
    bad = (gb != wb).nonzero().flatten()
    i = int(bad[0])
    raise AssertionError(f'{gc.name(c)}: {nm}: {bad.numel()}/{gb.numel()} elements differ from the float64 reference rounded once (fill outside the result '
                         f'included); first at flat element {i}: got {float(got[i])!r} want {float(want[i])!r}')


def run_exact(c):
    flav = c['flav']
    o = gc.operands(c)
    want = gc.expected(c, o)
    outs = _fresh(c, flav)
    picks = _call(c, flav, o, outs)
    assert picks == c['expect'], f'{gc.name(c)}: varhip_gemm16_last_pick(0), (1) = {picks}'
    _count(c, flav, picks)
    for nm, w in want.items():
        _assert_bits(c, nm, outs[nm].cpu(), w)


def _check_tolerance(c, flav, o, outs):
    g = gc.geometry(c)
    if c['entry'] == 'nt':
        ref = gc.value64(c, o)
        got = outs['out'].cpu()
        inside = torch.zeros(got.numel(), dtype=torch.bool)
        view = (c['batch'], c['M'], c['N']), (g['sO'], g['ldo'], 1)
        inside.as_strided(*view).fill_(True)
        assert bool(torch.isnan(got[~inside]).all()), f'{gc.name(c)}: padding of out was written'
        val = got.as_strided(*view).double()
        tol = torch.from_numpy(gemmcases.gemm16_tolerance(gc.mag64(c, o).numpy(), ref.numpy(), bool(c['out16']), ulp16=gc.ULP16[flav]))
        err = (val - ref).abs()
        assert bool((err <= tol).all()), f'{gc.name(c)}: {int((~(err <= tol)).sum())} outside tolerance, max err {float(err.nan_to_num(1e30).max()):.3e}'
        return
    rq, rk, rv = gc.value64(c, o)
    B2, l, H, pos0, Lmax = c['B2'], c['l'], c['H'], c['pos0'], c['Lmax']
    q = outs['q'].cpu().view(B2 * l, H, 64)
    kc, vc = outs['kc'].cpu().view(B2, H, Lmax, 64), outs['vc'].cpu().view(B2, H, Lmax, 64)
    for nm, got, ref in (('q', q, rq), ('k cache rows', kc[:, :, pos0:pos0 + l].permute(0, 2, 1, 3).reshape(-1, H, 64), rk),
                         ('v cache rows', vc[:, :, pos0:pos0 + l].permute(0, 2, 1, 3).reshape(-1, H, 64), rv)):
        err = (got.double() - ref).abs()
        assert bool((err <= gc.qkv_tolerance(ref, flav)).all()), f'{gc.name(c)}: {nm}: max err {float(err.nan_to_num(1e30).max()):.3e}'
    for cache in (kc, vc):
        assert bool(torch.isnan(cache[:, :, :pos0]).all()) and bool(torch.isnan(cache[:, :, pos0 + l:]).all()), f'{gc.name(c)}: a cache row outside [pos0, pos0 + l) was written'


def run_inexact(c):
    flav = c['flav']
    o = gc.operands(c)
    outs = _fresh(c, flav)
    picks = _call(c, flav, o, outs)
    assert picks == c['expect'], f'{gc.name(c)}: varhip_gemm16_last_pick(0), (1) = {picks}'
    _count(c, flav, picks)
    _check_tolerance(c, flav, o, outs)


def _run(cases):
    assert cases
    before = dict(LAUNCHES)
    for c in cases:
        (run_exact if c['exact'] else run_inexact)(c)
    print('varhip_gemm16_last_pick -> launches:', dict(sorted((f'{e}_{f} {k}', v - before.get((e, f, k), 0)) for (e, f, k), v in LAUNCHES.items() if v > before.get((e, f, k), 0))))


@pytest.mark.parametrize('code', list(gc.NT_INST))
@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_gemm_nt_every_instantiation(flav, code):
    """a ragged M with N four past the tile, one row, an exact fit; NONE / GELU / RESID with fp32 and 16-bit stores, fp32 and 16-bit residuals, gamma
    row groups; K / 64 below, equal to and above the kernel's stage count; padded lda, ldw, ldo, ldr, ldg"""
    _run([c for c in gc.cases('inst', flav) if c['expect'][0] == code])


@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_forced_256_tile_falls_through_to_the_one_tile_kernel(flav):
    """persistence on, tile 2 forced, N % 256 != 0 or rows % 256 != 0: k_gemm16<8,4,2,4>, never k_gemm16p (which stores whole tiles only)"""
    _run(gc.cases('fallthrough', flav))


@pytest.mark.parametrize('code', list(gc.QKV_INST))
@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_gemm_qkv_every_instantiation(flav, code):
    """l2norm 0 (exact: q scaled by 2^-3) and 1 (within one 16-bit rounding + 2e-4), pos0 > 0, Lmax > pos0 + l, H 1 and 3, M = 1, padded lda / ldw"""
    _run([c for c in gc.cases('qkv', flav) if c['expect'][0] == code])


@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_batched_launches_on_every_tile(flav):
    _run(gc.cases('batched', flav))


@pytest.mark.parametrize('i', range(len(gc.split_cases())))
@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_row_split(flav, i):
    """two launches over row ranges: the first on k_gemm16p or k_gemm16<8,4,2,4>, the second (m_base > 0) on the 128x128, a 64-row or the 32x32
    kernel; gamma's row groups and a q/k/v image straddle the cut"""
    _run([gc.cases('split', flav)[i]])


@pytest.mark.parametrize('part', range(4))
@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_automatic_picker_either_side_of_each_decision(flav, part):
    _run(gc.cases('picker', flav)[part::4])


@pytest.mark.parametrize('i', range(len(gc.equal_groups())))
@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_gelu_and_l2norm_are_bit_equal_across_instantiations(flav, i):
    """one call under every setting that can run it (the two-stage kernels and the persistent one included): the hook names each kernel, the first
    result is within the bar against float64, all others equal it bit for bit"""
    base, variants = gc.equal_groups()[i]
    base = dict(base, flav=flav)
    o = gc.operands(base)
    first = None
    for tile, persist, deep, code in variants:
        c = dict(base, tile=tile, persist=persist, deep=deep, expect=(code, 0))
        outs = _fresh(c, flav)
        picks = _call(c, flav, o, outs)
        assert picks == c['expect'], f'{gc.name(c)}: varhip_gemm16_last_pick(0), (1) = {picks}'
        _count(c, flav, picks)
        if first is None:
            _check_tolerance(c, flav, o, outs)
            first = outs
        else:
            for nm in outs:
                assert torch.equal(gc.bits(outs[nm]), gc.bits(first[nm])), (f'{gc.name(c)}: {nm} differs from the first variant '
                                                                            f'{variants[0]} in {int((gc.bits(outs[nm]) != gc.bits(first[nm])).sum())} elements')


def test_a_refused_call_leaves_the_hook_unchanged():
    hip = _hip()
    so = hip.lib().so
    c = dict(gc.nt('inst', 49, 36, 64, 'none16', gc.K32D, tile=1), flav='f16')
    run_exact(c)
    before = (so.varhip_gemm16_last_pick(0), so.varhip_gemm16_last_pick(1))
    assert before == (gc.K32D, 0)
    A = torch.zeros(49, 64, dtype=torch.float16, device='cuda'); W = torch.zeros(36, 64, dtype=torch.float16, device='cuda')
    out = torch.full((49 * 36,), gc.NAN, dtype=torch.float16, device='cuda')
    with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
        hip.call('gemm_nt_f16', A, 64, W, 64, None, out, 36, 1, 49, 34, 64, 0, None, 0, 0, None, 0, 1, 1, 0, 0, 0)      # N % 4 != 0
    torch.cuda.synchronize()
    assert (so.varhip_gemm16_last_pick(0), so.varhip_gemm16_last_pick(1)) == before and bool(torch.isnan(out).all())
    assert so.varhip_gemm16_last_pick(2) == 0 and so.varhip_gemm16_last_pick(-1) == 0
