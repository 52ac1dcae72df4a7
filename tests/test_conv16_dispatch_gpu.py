"""Every kernel instantiation dispatch_conv16 (var_amd/csrc/conv16.hip) can launch — k_conv16h<TNW, PW, GN> over TNW in {5, 4}, PW in {32, 16},
plain and GroupNorm-fused, and k_conv16<5,3,4,2>, <5,4,2>, <4,3,4,2>, <4,4,2>, <2,4,2>, <1,4,2>, each as a 3x3 convolution and in the four-phase
form of Upsample2x — in both 16-bit flavours, on the table of tests/conv16cases.py (validated without a GPU by tests/test_conv16_dispatch_cpu.py).

After every call varhip_conv16_last_pick() must name the instantiation the case was built for (forcing a tile is a request; a case that fell
through to another kernel fails here), and the output, NaN-filled before the call, must EQUAL the float64 reference cast once to the output
type: the operands lie on a dyadic grid on which every partial sum is exact in fp32 in any order, so the rounding point, the precision of the
bias add and the place of the residual are pinned bit for bit on every kernel.  The GroupNorm-fused cases keep their criterion: bit-equal to
gn_apply followed by the plain convolution (map and partials), both within the float64 bar."""
import pytest

from tests import conv16cases as cc
from tests import util

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _hip():
    from var_amd import hip
    return hip


@pytest.fixture(autouse=True)
def force_reset():
    yield
    _hip().lib().so.varhip_conv16_force_tile(0)


def _forced(hip, c, fn):
    """fn() under the case's forced tile -> (fn's result, varhip_conv16_last_pick() right after it)"""
    so = hip.lib().so
    so.varhip_conv16_force_tile(c['wm'])
    try:
        res = fn()
        return res, so.varhip_conv16_last_pick()
    finally:
        so.varhip_conv16_force_tile(0)


def _assert_equal(c, got, want):
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    i = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f'{cc.name(c)}: {int(bad.sum())}/{got.numel()} elements differ from the float64 reference rounded once, {int(torch.isnan(got).sum())} of '
                         f'them not written; first at {i}: got {float(got[i])!r} want {float(want[i])!r}')


def _check_partials(c, part, out, nblk, low_hw=None):
    """GroupNorm partials = per-channel (sum, sum of squares) of the ROUNDED outputs; the existing bars (conv16cases.PART_BLOCK / PART_SAMPLE)"""
    B, Cout = c['B'], c['Cout']
    assert not bool(torch.isnan(part).any()), f'{cc.name(c)}: GroupNorm partials were not written'
    part = part.cpu()
    o = out.double().cpu()
    kernel = c['expect'] % 10
    if c['entry'] == 'conv' and kernel in (cc.K128, cc.K256):
        o = o.view(B, nblk, 128, Cout)
        assert torch.allclose(part[..., 0], o.sum(2), **cc.PART_BLOCK) and torch.allclose(part[..., 1], (o * o).sum(2), **cc.PART_BLOCK), cc.name(c)
    else:
        o = o.view(B, -1, Cout)
        assert torch.allclose(part[..., 0].sum(1), o.sum(1), **cc.PART_SAMPLE) and torch.allclose(part[..., 1].sum(1), (o * o).sum(1), **cc.PART_SAMPLE), cc.name(c)


def run_dyadic(c):
    hip = _hip()
    dt, flav = cc.DTYPE[c['flav']], c['flav']
    o = cc.operands(c)
    want = cc.expected(c, o)
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    x, w, bias = o.x.to(dt).cuda(), o.w.to(dt).cuda(), o.bias.float().cuda()
    resid = None if o.resid is None else o.resid.to(dt).cuda()
    up = c['entry'] == 'upconv'
    nblk = hip.conv_gn_blocks(H, W, Cout, phase=up) if (c['omode'] == 0 and Cout % 4 == 0) else 0
    part = torch.full((B, nblk, Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if nblk else None
    if c['omode']:
        out = torch.full((B, Cout, H, W), cc.SENTINEL32, dtype=torch.float32, device='cuda')
    else:
        out = torch.full((B, H, W, Cout), float('nan'), dtype=dt, device='cuda')
    if up:
        call = lambda: util.guarded_call('upconv_phase_' + flav, x, w, bias, out, part, B, H, W, Cin, Cout)
    else:
        call = lambda: util.guarded_call('conv3x3_nhwc_' + flav, x, w, bias, resid, out, part, B, H, W, Cin, Cout, c['omode'])
    _, pick = _forced(hip, c, call)
    assert pick == c['expect'], f'{cc.name(c)}: varhip_conv16_last_pick() = {pick}'
    got = out.cpu()
    if c['omode']:
        assert not bool((got == cc.SENTINEL32).any()), f'{cc.name(c)}: {int((got == cc.SENTINEL32).sum())} elements were not written'
    _assert_equal(c, got, want)
    if nblk:
        _check_partials(c, part, out, nblk)
    return pick


def run_gn(c):
    """tests/test_f16_gpu.py::test_gnconv16_fused_equals_apply_then_conv on the table's shapes, with the hook: the two launches must run
    k_conv16h<.., false>, the fused call k_conv16h<.., true> of the same TNW and patch form"""
    hip = _hip()
    so = hip.lib().so
    dt, flav = cc.DTYPE[c['flav']], c['flav']
    B, H, W, Cin, Cout, res, silu = c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['res'], c['silu']
    g = torch.Generator().manual_seed(H * 5 + W + Cin + Cout)
    x = (torch.randn(B, H, W, Cin, generator=g) * 1.3 + 0.2).to(dt).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * (2.0 / (9 * Cin) ** 0.5)).to(dt).cuda()
    bias = (torch.randn(Cout, generator=g) * 0.1).cuda()
    resid = torch.randn(B, H, W, Cout, generator=g).to(dt).cuda() if res else None
    gamma, beta = (torch.randn(Cin, generator=g) * 0.2 + 1.0).cuda(), (torch.randn(Cin, generator=g) * 0.2).cuda()
    stats = torch.empty(B, 32, 2, dtype=torch.float32, device='cuda')
    scratch = torch.empty(hip.gn_scratch_elems(B, H * W, Cin, 32), dtype=torch.float64, device='cuda')
    util.guarded_call('gn_stats_' + flav, x, stats, scratch, B, H * W, Cin, 32, 1e-6)
    xn = torch.empty_like(x)
    util.guarded_call('gn_apply_' + flav, x, stats, gamma, beta, xn, B, H * W, Cin, 32, silu)
    table = torch.empty(B, 2, Cin, dtype=torch.float32, device='cuda')
    util.guarded_call('gn_scale_shift_f32', stats, gamma, beta, table, B, Cin, 32)
    nblk = hip.conv_gn_blocks(H, W, Cout)
    nan = float('nan')
    two = torch.full((B, H, W, Cout), nan, dtype=dt, device='cuda')
    part2 = torch.full((B, nblk, Cout, 2), nan, dtype=torch.float64, device='cuda') if nblk else None
    (_, plain_pick) = _forced(hip, c, lambda: util.guarded_call('conv3x3_nhwc_' + flav, xn, w, bias, resid, two, part2, B, H, W, Cin, Cout, 0))
    fused = torch.full((B, H, W, Cout), nan, dtype=dt, device='cuda')
    part1 = torch.full((B, nblk, Cout, 2), nan, dtype=torch.float64, device='cuda') if nblk else None
    if c['einval']:
        so.varhip_conv16_force_tile(c['wm'])
        try:
            assert not hip.conv16_gn_fusable(B, H, W, Cin, Cout), cc.name(c)
            with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
                hip.call('gnconv3x3_nhwc_' + flav, x, table, silu, w, bias, resid, fused, part1, B, H, W, Cin, Cout)
            assert so.varhip_conv16_last_pick() == plain_pick, 'a refused call changed the hook'
        finally:
            so.varhip_conv16_force_tile(0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(fused).all()), f'{cc.name(c)}: a refused call wrote to out'
        return None
    assert plain_pick == c['expect'] - 100, f'{cc.name(c)}: the two launches ran {plain_pick}'
    def fused_call():
        assert hip.conv16_gn_fusable(B, H, W, Cin, Cout), cc.name(c)
        util.guarded_call('gnconv3x3_nhwc_' + flav, x, table, silu, w, bias, resid, fused, part1, B, H, W, Cin, Cout)
    _, pick = _forced(hip, c, fused_call)
    assert pick == c['expect'], f'{cc.name(c)}: varhip_conv16_last_pick() = {pick}'
    assert not bool(torch.isnan(fused).any()) and not bool(torch.isnan(two).any()), f'{cc.name(c)}: elements of out were not written'
    assert torch.equal(fused, two), (f'{cc.name(c)}: fused differs from the two launches in {int((fused != two).sum())} of {fused.numel()} elements, '
                                     f'max {float((fused.float() - two.float()).abs().max()):.3e}')
    if nblk:
        assert not bool(torch.isnan(part1).any()) and torch.equal(part1, part2), f'{cc.name(c)}: GroupNorm partials differ'
    ref = torch.nn.functional.conv2d(xn.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2), bias.double().cpu(), padding=1)
    if res:
        ref = ref + resid.double().cpu().permute(0, 3, 1, 2)
    tol = cc.gn_tolerance(ref, Cin, flav)
    for nm, t in (('fused', fused), ('two launches', two)):
        err = (t.double().cpu().permute(0, 3, 1, 2) - ref).abs()
        assert bool((err <= tol).all()), f'{cc.name(c)}: {nm}: max err {float(err.max()):.3e}'
    return pick


def _run(cases):
    picks = {}
    for c in cases:
        p = run_gn(c) if c['entry'] == 'gnconv' else run_dyadic(c)
        picks[p] = picks.get(p, 0) + 1
    print('varhip_conv16_last_pick -> calls:', dict(sorted((k, v) for k, v in picks.items() if k is not None)))


@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_halo_patch_kernel_every_instantiation(flav):
    """k_conv16h<5|4, 32|16, false>: one, two and three channel tiles, 2 to 9 workgroups (the XCD dealing with and without a remainder), 1 to 5
    chunks, W = 48, with and without a residual, Cout = 640"""
    _run(cc.cases('halo', flav))


@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_halo_patch_kernel_groupnorm_fused(flav):
    """k_conv16h<5|4, 32|16, true> on the same shapes, and the refusal of a table that does not fit"""
    _run(cc.cases('gn', flav))


@pytest.mark.parametrize('tnw', [5, 4, 2, 1])
@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_pixel_tile_kernel_every_instantiation(flav, tnw):
    """k_conv16<TNW, ..> on 128- and 256-pixel tiles: second and third channel tiles, partial last channel tiles under the vector epilogue, the
    element-wise epilogue's 16-bit store, pixel counts off every tile, several images inside one tile"""
    _run([c for c in cc.cases('tile', flav) if (c['expect'] // 10) % 10 == tnw])


@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_fp32_nchw_stores(flav):
    _run(cc.cases('omode', flav))


@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_phase_form_every_instantiation(flav):
    _run(cc.cases('phase', flav))


@pytest.mark.parametrize('flav', cc.FLAVOURS)
def test_automatic_picker_on_either_side_of_its_thresholds(flav):
    _run(cc.cases('auto', flav))
