"""varhip_conv3x3_wino_up_nhwc_f32: the fp32 decoder's Upsample2x convolutions as position-sparse Winograd F(2x2,3x3) on the low-resolution
map (var_amd/csrc/winograd.hip).

Shapes are the smallest at which the kernel can go wrong: low-res 8x8 -> 16x16 (one patch, all four borders padded), 16x16 -> 32x32 (four
patches: seams and interior borders), 8x24 -> 16x48 (non-square, three patches), channels (32, 32), (64, 32), (32, 96): one and several K
tiles, the peeled last pair alone and behind a loop trip, one and several channel groups.

Bars.  Against float64 (nearest upsample, then a 9-tap convolution, on the CPU) the rule of tests/test_winograd_gpu.py: the new kernel's
max error is at most 2x the direct four-phase kernel's on the same operands.  With small integer operands every fp32 sum is exact in any
order, so the output equals the reference bit for bit: that pins which low-res pixel, tap, tile and channel lands where.  The GroupNorm
statistics folded from the new launch's partials agree with a full pass over its output, and with those folded from the direct launch's
partials where that launch has them, to test_winograd_gpu.py's tolerance for that quantity (rtol 1e-6, atol 1e-7).

The kernel reads the pre-summed phase weights (varhip_upconv_pack_f32), as the direct form does.  The decoder reaches it through
varhip_upconv_phase[_gn]_f32 with the library's switch on (var_amd.hip.upconv_winograd); off, which is the default, those entry points
run the four-phase kernel."""
import functools

import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu

GEOM = [(2, 8, 8), (2, 16, 16), (3, 8, 24)]                        # (B, low-res H, low-res W)
CHAN = [(32, 32), (64, 32), (32, 96)]


def _hip():
    from var_amd import hip
    return hip


@functools.lru_cache(maxsize=None)
def _case(B, Hl, Wl, Cin, Cout, integer=False):
    """operands, the float64 reference (computed once, shared, never written) and the direct four-phase result"""
    hip = _hip()
    g = torch.Generator(device='cuda').manual_seed(Hl * 131 + Wl * 17 + Cin + Cout)
    if integer:
        x = torch.randint(-8, 9, (B, Hl, Wl, Cin), device='cuda', generator=g).float()
        wt = torch.randint(-4, 5, (Cout, 3, 3, Cin), device='cuda', generator=g).float()
        bias = torch.randint(-16, 17, (Cout,), device='cuda', generator=g).float()
    else:
        x = F.silu(torch.randn(B, Hl, Wl, Cin, device='cuda', generator=g))
        wt = (torch.rand(Cout, 3, 3, Cin, device='cuda', generator=g) * 2 - 1) / (9 * Cin) ** 0.5
        bias = torch.rand(Cout, device='cuda', generator=g) * 0.2 - 0.1
    xu = x.double().cpu().permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    ref = F.conv2d(xu, wt.double().cpu().permute(0, 3, 1, 2), bias.double().cpu(), padding=1).permute(0, 2, 3, 1).contiguous()
    wp = torch.empty(4, Cout, 2, 2, Cin, device='cuda')
    hip.call('upconv_pack_f32', wt, wp, Cin, Cout)
    H, W = 2 * Hl, 2 * Wl
    yd = torch.empty(B, H, W, Cout, device='cuda')
    nd = hip.conv_gn_blocks(H, W, Cout, phase=True)
    pd = torch.full((B, nd, Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if nd else None
    if nd:
        util.guarded_call('upconv_phase_gn_f32', x, wp, bias, yd, pd, B, H, W, Cin, Cout)
    else:
        util.guarded_call('upconv_phase_f32', x, wp, bias, yd, B, H, W, Cin, Cout)
    return x, wp, bias, ref, yd, pd


def _up(x, wp, bias, B, H, W, Cin, Cout, with_part=True):
    out = torch.full((B, H, W, Cout), float('nan'), device='cuda')
    nblk = _hip().conv_gn_blocks(H, W, Cout)
    assert nblk == H * W // 128
    part = torch.full((B, nblk, Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if with_part else None
    util.guarded_call('conv3x3_wino_up_nhwc_f32', x, wp, bias, out, part, B, H, W, Cin, Cout)
    return out, part


def _stats(part, B, nblk, HW, C):
    st = torch.empty(B, 32, 2, device='cuda')
    util.guarded_call('gn_stats_part_f32', part, st, B, nblk, HW, C, 32, 1e-6)
    return st


@pytest.mark.parametrize('B,Hl,Wl', GEOM)
@pytest.mark.parametrize('Cin,Cout', CHAN)
def test_up_vs_float64_and_direct(B, Hl, Wl, Cin, Cout):
    x, wp, bias, ref, yd, pd = _case(B, Hl, Wl, Cin, Cout)
    H, W = 2 * Hl, 2 * Wl
    yw, part = _up(x, wp, bias, B, H, W, Cin, Cout)
    ew, ed = (yw.double().cpu() - ref).abs().max().item(), (yd.double().cpu() - ref).abs().max().item()
    print(f'B={B} {Hl}x{Wl}->{H}x{W} {Cin}->{Cout}: |wino_up - f64| {ew:.3g}, |direct - f64| {ed:.3g}, ratio {ew / ed:.3f}')
    assert ed > 0 and ew <= 2 * ed
    # partials: every (block, channel) written; folded, they are the statistics of a full pass over this output
    assert not torch.isnan(part).any()
    hip = _hip()
    nblk = H * W // 128
    st_part = _stats(part, B, nblk, H * W, Cout)
    st_full = torch.empty(B, 32, 2, device='cuda')
    scratch = torch.empty(hip.gn_scratch_elems(B, H * W, Cout, 32), dtype=torch.float64, device='cuda')
    util.guarded_call('gn_stats_f32', yw, st_full, scratch, B, H * W, Cout, 32, 1e-6)
    torch.testing.assert_close(st_part, st_full, rtol=1e-6, atol=1e-7)
    # block 2 t + h = 8-row half h of the t-th 16 x 16 output patch: the last block's channel sums directly
    t, h, pw = (H // 16) * (W // 16) - 1, 1, W // 16
    py, px = divmod(t, pw)
    blk = yw[B - 1, py * 16 + 8 * h: py * 16 + 8 * h + 8, px * 16: px * 16 + 16, :].double()
    torch.testing.assert_close(part[B - 1, 2 * t + h, :, 0], blk.sum((0, 1)), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(part[B - 1, 2 * t + h, :, 1], (blk * blk).sum((0, 1)), rtol=1e-12, atol=1e-9)
    if pd is not None:
        st_dir = _stats(pd, B, pd.shape[1], H * W, Cout)           # the direct launch produces partials here too
        print(f'   folded (mean, rstd), new vs direct: max |difference| {(st_part - st_dir).abs().max().item():.3g}')
        torch.testing.assert_close(st_part, st_dir, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('B,Hl,Wl', GEOM)
@pytest.mark.parametrize('Cin,Cout', CHAN)
def test_up_position_map_exact(B, Hl, Wl, Cin, Cout):
    """|x| <= 8, |w| <= 4, Cin <= 64: phase taps and their sums are integers up to 36, transformed inputs up to 32, so every partial sum is an
    integer below 2^24, exact in fp32"""
    x, wp, bias, ref, yd, _ = _case(B, Hl, Wl, Cin, Cout, integer=True)
    yw, _ = _up(x, wp, bias, B, 2 * Hl, 2 * Wl, Cin, Cout, with_part=False)
    assert torch.equal(yw.double().cpu(), ref)
    assert torch.equal(yd.double().cpu(), ref)                     # (the operands are exact for the phase form too)


@pytest.mark.parametrize('Hl,Wl,Cin,Cout', [(8, 8, 64, 32), (16, 16, 32, 96), (8, 24, 32, 32)])
def test_up_batch_invariant(Hl, Wl, Cin, Cout):
    """image 0 alone and as image 1 of B = 3: output and partials bit for bit"""
    x, wp, bias, _, _, _ = _case(3, Hl, Wl, Cin, Cout)
    H, W = 2 * Hl, 2 * Wl
    xb = torch.stack([x[1], x[0], x[2]]).contiguous()
    yb, pb = _up(xb, wp, bias, 3, H, W, Cin, Cout)
    y1, p1 = _up(x[0:1].contiguous(), wp, bias, 1, H, W, Cin, Cout)
    assert torch.equal(y1[0], yb[1]) and torch.equal(p1[0], pb[1])


@pytest.mark.parametrize('B,Hl,Wl,Cin,Cout', [(2, 16, 16, 64, 32), (3, 8, 24, 32, 96)])
def test_phase_entry_points_follow_the_switch(B, Hl, Wl, Cin, Cout):
    """varhip_upconv_phase[_gn]_f32: with the switch on, the bits of varhip_conv3x3_wino_up_nhwc_f32; off (the default), the four-phase kernel"""
    hip = _hip()
    x, wp, bias, _, yd, pd = _case(B, Hl, Wl, Cin, Cout)
    H, W = 2 * Hl, 2 * Wl
    yw, part = _up(x, wp, bias, B, H, W, Cin, Cout)
    nd = hip.conv_gn_blocks(H, W, Cout, phase=True)
    out = torch.full((B, H, W, Cout), float('nan'), device='cuda')
    pp = torch.full((B, nd, Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if nd else None
    call = (lambda: util.guarded_call('upconv_phase_gn_f32', x, wp, bias, out, pp, B, H, W, Cin, Cout)) if nd else \
           (lambda: util.guarded_call('upconv_phase_f32', x, wp, bias, out, B, H, W, Cin, Cout))
    hip.upconv_winograd(True)
    try: call()
    finally: hip.upconv_winograd(False)
    assert torch.equal(out, yw) and (pp is None or torch.equal(pp, part))
    call()
    assert torch.equal(out, yd) and (pp is None or torch.equal(pp, pd)) and not torch.equal(out, yw)


def test_up_argument_errors():
    from var_amd.hip import VarHipError
    x, wp, bias, _, _, _ = _case(2, 8, 8, 32, 32)
    out = torch.empty(2, 16, 16, 32, device='cuda')
    call = lambda *a: _hip().call('conv3x3_wino_up_nhwc_f32', *a)
    for H, W, Cin, Cout in [(24, 16, 32, 32), (16, 8, 32, 32), (16, 16, 48, 32), (16, 16, 32, 16), (0, 16, 32, 32)]:
        with pytest.raises(VarHipError):
            call(x, wp, bias, out, None, 2, H, W, Cin, Cout)
    with pytest.raises(VarHipError):
        call(x, wp, None, out, None, 2, 16, 16, 32, 32)
    with pytest.raises(VarHipError):
        call(x.view(-1)[1:], wp, bias, out, None, 1, 16, 16, 32, 32)


def test_switch_off_is_the_direct_path_and_on_takes_the_new_kernel():
    """ch = 32, f_hat 4 x 4 (the smallest pyramid of the decoder's launch-trace cases): with winograd off the decode is, bit for bit, the
    decode whose every Upsample2x runs the four-phase kernel and every ResnetBlock conv the direct kernel; with it on, the three upsamples
    onto 16^2, 32^2 and 64^2 run in the new family and the image moves by less than the decode tests' 1e-5"""
    from var_amd import hip
    from var_amd.detinit import fill_module_device_
    from var_amd.models.vqvae import VQVAE
    vae = VQVAE(vocab_size=64, z_channels=32, ch=32, test_mode=True, share_quant_resi=4, v_patch_nums=(1, 2, 4)).cuda()
    fill_module_device_(vae, depth=16, seed=0, prefix='vae.')
    eng = vae._decoder_engine()
    fh = torch.randn(2, 4, 4, 32, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 0.5

    def timed():
        hip.timing_reset(); hip.timing_enable(True)
        try:
            img = eng.decode_nhwc(fh, denorm=True)
            return img, hip.timing_read()
        finally:
            hip.timing_enable(False)
    with torch.no_grad():
        eng.winograd = False
        try:
            a, ta = timed()
            a2, _ = timed()
        finally:
            eng.winograd = True
        b, tb = timed()
    assert ta['conv_wino_up']['launches'] == 0 and ta['conv_wino']['launches'] == 0 and torch.equal(a, a2)
    assert tb['conv_wino_up']['launches'] == 3
    assert tb['conv_wino_up']['flops'] == sum(2.0 * 2 * (s * s / 4) * 9 * c * c for s, c in ((16, 64), (32, 64), (64, 32)))
    d = (a - b).abs().max().item()
    print(f'ch32 decode: max |winograd on - off| = {d:.3g}')
    assert 0 < d <= 1e-5
