"""varhip_conv3x3_wino_nhwc_f32: the decoder's ResnetBlock convolutions as fused Winograd F(2x2,3x3) (var_amd/csrc/winograd.hip).

Error bars.  The direct kernel sums 9*Cin products in one fp32 fma chain; the Winograd kernel sums Cin products per transform position
(in fp32 MFMA order) between a few exact-order additions (B^T d B: 2 roundings, A^T M A: 4 roundings, U rounded once from float64).  On
SiLU-like input with unit-variance weights per output both are a few ulp of the output scale; measured on MI355X at every decoder shape
the Winograd error against float64 is 0.32-0.34x the direct kernel's.  The bar is 2x the direct kernel's error measured
in the same test on the same data: it fails on any transform slip (which costs orders of magnitude) and leaves 6x headroom over the
measured ratio.  Against the direct kernel the difference is bounded by the sum of both errors, so 3x the direct error.
"""
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu

# (H = W, Cin, Cout) of every decoder level at ch=160 (ch_mult 1, 1, 2, 2, 4): 256^2 / 128^2 at 160, 64^2 160 -> 320 and 320, 32^2, 16^2
SHAPES = [(256, 160, 160), (128, 160, 160), (64, 160, 320), (64, 320, 320), (32, 320, 320), (16, 640, 640)]


def _hip():
    from var_amd import hip
    return hip


def _data(B, H, Cin, Cout, seed=0, W=None):
    W = H if W is None else W
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = F.silu(torch.randn(B, H, W, Cin, device='cuda', generator=g))
    wt = (torch.rand(Cout, 3, 3, Cin, device='cuda', generator=g) * 2 - 1) / (9 * Cin) ** 0.5
    bias = torch.rand(Cout, device='cuda', generator=g) * 0.2 - 0.1
    resid = torch.randn(B, H, W, Cout, device='cuda', generator=g)
    return x, wt, bias, resid


def _wino(x, u, bias, resid, B, H, W, Cin, Cout, part=None):
    out = torch.empty(B, H, W, Cout, device='cuda')
    util.guarded_call('conv3x3_wino_nhwc_f32', x, u, bias, resid, out, part, B, H, W, Cin, Cout)
    return out


def _direct(x, wt, bias, resid, B, H, W, Cin, Cout):
    out = torch.empty(B, H, W, Cout, device='cuda')
    util.guarded_call('conv3x3_nhwc_f32', x, wt, bias, resid, out, B, H, W, Cin, Cout, 0, 0)
    return out


def _ref64(x, wt, bias, resid):
    y = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1)
    return y if resid is None else y + resid.double()


@pytest.mark.parametrize('H,Cin,Cout', SHAPES)
@pytest.mark.parametrize('with_resid', [False, True])
def test_wino_vs_float64_direct_and_gn_partials(H, Cin, Cout, with_resid):
    from var_amd.engine import wino_filter
    hip = _hip()
    B = 2
    x, wt, bias, resid = _data(B, H, Cin, Cout)
    rs = resid if with_resid else None
    nblk = hip.conv_gn_blocks(H, H, Cout)
    assert nblk == H * H // 128
    part = torch.full((B, nblk, Cout, 2), float('nan'), dtype=torch.float64, device='cuda')
    yw = _wino(x, wino_filter(wt), bias, rs, B, H, H, Cin, Cout, part)
    yd = _direct(x, wt, bias, rs, B, H, H, Cin, Cout)
    r = _ref64(x, wt, bias, rs)
    ew, ed = (yw.double() - r).abs().max().item(), (yd.double() - r).abs().max().item()
    print(f'{H}x{H} {Cin}->{Cout} resid={with_resid}: |wino - f64| {ew:.3g}, |direct - f64| {ed:.3g}')
    assert ed > 0 and ew <= 2 * ed
    assert (yw - yd).abs().max().item() <= 3 * ed
    # the partials cover every (block, channel) and give the statistics of a full pass over the output (fp64 block order: ~1e-16 relative)
    assert not torch.isnan(part).any()
    st_part = torch.empty(B, 32, 2, device='cuda'); st_full = torch.empty(B, 32, 2, device='cuda')
    util.guarded_call('gn_stats_part_f32', part, st_part, B, nblk, H * H, Cout, 32, 1e-6)
    scratch = torch.empty(hip.gn_scratch_elems(B, H * H, Cout, 32), dtype=torch.float64, device='cuda')
    util.guarded_call('gn_stats_f32', yw, st_full, scratch, B, H * H, Cout, 32, 1e-6)
    torch.testing.assert_close(st_part, st_full, rtol=1e-6, atol=1e-7)
    # block 2 t + h = half h of 16 x 16 patch t (row-major patches): check one block's channel sums directly
    t, h, pw = (H // 16) * (H // 16) - 1, 1, H // 16
    py, px = divmod(t, pw)
    blk = yw[1, py * 16 + 8 * h: py * 16 + 8 * h + 8, px * 16: px * 16 + 16, :].double()
    torch.testing.assert_close(part[1, 2 * t + h, :, 0], blk.sum((0, 1)), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(1, 16, 48, 64, 64), (1, 48, 16, 64, 64), (1, 16, 48, 160, 160), (2, 48, 16, 160, 160), (1, 32, 32, 64, 64), (1, 16, 16, 160, 160)])
@pytest.mark.parametrize('with_resid', [False, True])
def test_wino_single_image_and_non_square(B, H, W, Cin, Cout, with_resid):
    """B = 1 and H != W (a swap of H and W in the patch indexing is invisible on square images): against float64 and the direct kernel with this
    file's bar.  The kernel's descriptor window is exactly one image (halo pixels outside it carry offset 0x80000000), so with one image the
    window is the whole allocation and a request that strays past either end of the image lands in a band instead of a neighbouring image;
    the GroupNorm partials, allocated at exactly conv_gn_blocks' answer, give the statistics of a full pass over the output"""
    from var_amd.engine import wino_filter
    hip = _hip()
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=H + W, W=W)
    rs = resid if with_resid else None
    nblk = hip.conv_gn_blocks(H, W, Cout)
    assert nblk == H * W // 128
    part = torch.full((B, nblk, Cout, 2), float('nan'), dtype=torch.float64, device='cuda')
    yw = _wino(x, wino_filter(wt), bias, rs, B, H, W, Cin, Cout, part)
    yd = _direct(x, wt, bias, rs, B, H, W, Cin, Cout)
    r = _ref64(x, wt, bias, rs)
    ew, ed = (yw.double() - r).abs().max().item(), (yd.double() - r).abs().max().item()
    print(f'B={B} {H}x{W} {Cin}->{Cout} resid={with_resid}: |wino - f64| {ew:.3g}, |direct - f64| {ed:.3g}')
    assert ed > 0 and ew <= 2 * ed
    assert (yw - yd).abs().max().item() <= 3 * ed
    assert not torch.isnan(part).any()
    st_part = torch.empty(B, 32, 2, device='cuda'); st_full = torch.empty(B, 32, 2, device='cuda')
    util.guarded_call('gn_stats_part_f32', part, st_part, B, nblk, H * W, Cout, 32, 1e-6)
    scratch = torch.empty(hip.gn_scratch_elems(B, H * W, Cout, 32), dtype=torch.float64, device='cuda')
    util.guarded_call('gn_stats_f32', yw, st_full, scratch, B, H * W, Cout, 32, 1e-6)
    torch.testing.assert_close(st_part, st_full, rtol=1e-6, atol=1e-7)
    # block 2 t + h = half h of 16 x 16 patch t, patches row-major over (H / 16, W / 16): the last block's channel sums directly
    t, h, pw = (H // 16) * (W // 16) - 1, 1, W // 16
    py, px = divmod(t, pw)
    blk = yw[B - 1, py * 16 + 8 * h: py * 16 + 8 * h + 8, px * 16: px * 16 + 16, :].double()
    torch.testing.assert_close(part[B - 1, 2 * t + h, :, 0], blk.sum((0, 1)), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('H,Cin,Cout', [(32, 320, 320), (16, 640, 640), (64, 160, 320)])
def test_wino_batch_invariant(H, Cin, Cout):
    """an image's result does not depend on B or on its position in the batch: B = 64 against each image alone, bit for bit"""
    from var_amd.engine import wino_filter
    B = 64
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=1)
    u = wino_filter(wt)
    yb = _wino(x, u, bias, resid, B, H, H, Cin, Cout)
    for i in (0, 17, 63):
        y1 = _wino(x[i:i + 1].contiguous(), u, bias, resid[i:i + 1].contiguous(), 1, H, H, Cin, Cout)
        assert torch.equal(y1[0], yb[i]), i


def test_wino_argument_errors():
    from var_amd.engine import wino_filter
    from var_amd.hip import VarHipError
    x, wt, bias, resid = _data(1, 32, 64, 64)
    u = wino_filter(wt)
    out = torch.empty(1, 32, 32, 64, device='cuda')
    call = lambda *a: _hip().call('conv3x3_wino_nhwc_f32', *a)
    call(x, u, bias, None, out, None, 1, 32, 32, 64, 64)                                   # the valid call
    for H, W, Cin, Cout in [(24, 32, 64, 64), (32, 31, 64, 64), (33, 32, 64, 64), (32, 32, 48, 64), (32, 32, 64, 48), (0, 32, 64, 64)]:
        with pytest.raises(VarHipError):
            call(x, u, bias, None, out, None, 1, H, W, Cin, Cout)
    with pytest.raises(VarHipError):
        call(x, u, bias, None, out, None, 0, 32, 32, 64, 64)                                # B = 0
    with pytest.raises(VarHipError):
        call(x, u, None, None, out, None, 1, 32, 32, 64, 64)                                # no bias
    with pytest.raises(VarHipError):
        call(x.view(-1)[1:], u, bias, None, out, None, 1, 16, 16, 64, 64)                   # misaligned input


def test_wino_decode_vs_direct_decode():
    """A full B = 64 fp32 decode of the bench's VQVAE (ch 160, detinit seed 0) with the Winograd path on and forced off: images in [0, 1]
    differ by at most 1e-5 (measured 3.8e-6 with 64^2 and up on it, 4.8e-6 with 32^2 and up), and the on-switch
    actually changes which kernels run."""
    from var_amd import hip
    from var_amd.detinit import fill_module_device_
    from var_amd.models.vqvae import VQVAE
    vae = VQVAE(vocab_size=4096, z_channels=32, ch=160, test_mode=True, share_quant_resi=4,
                v_patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16)).cuda()
    fill_module_device_(vae, depth=16, seed=0, prefix='vae.')
    eng = vae._decoder_engine()
    fh = torch.randn(64, 16, 16, 32, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 0.5
    with torch.no_grad():
        eng.winograd = False
        a = eng.decode_nhwc(fh, denorm=True)
        eng.winograd = True
        hip.timing_reset(); hip.timing_enable(True)
        try:
            b = eng.decode_nhwc(fh, denorm=True)
            t = hip.timing_read()
        finally:
            hip.timing_enable(False)
    assert t['conv_wino']['launches'] == 2 * (2 + 3 * eng.nlev)          # conv1 + conv2 of every ResnetBlock (16^2 and up all take it)
    d = (a - b).abs().max().item()
    print(f'decode B=64: max |wino - direct| = {d:.3g}')
    assert 0 < d <= 1e-5
