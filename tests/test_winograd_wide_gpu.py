"""The wide workgroup shape of varhip_conv3x3_wino_nhwc_f32 (k_conv3x3_wino_wide: 32 tiles x 80 output channels, var_amd/csrc/winograd.hip,
DESIGN.md §13.3) against the shape it stands in for (k_conv3x3_wino: 64 tiles x 32 channels).

The arithmetic is the same, accumulator by accumulator: the K order, the A^T (.) A association, bias then residual, and the fp64 GroupNorm
partials' pairs and tree.  So the comparison of the two shapes is torch.equal, on the output and on the partials.  The float64 check is the
bar of tests/test_winograd_gpu.py (2x the direct kernel's error on the same data) and does not lean on the twin.  Every call goes through
util.guarded_call: each operand sits between guard bands, which is what the 18 x 10 patch addressing, the ragged last DMA
request and the 80-channel stores are held to.  Outputs and partials start as NaN, so an element nobody writes stays visible.
"""
import pytest

torch = pytest.importorskip('torch')

from tests import util
from tests.test_winograd_gpu import _data, _direct, _ref64

pytestmark = pytest.mark.gpu


def _run(shape, x, u, bias, resid, B, H, W, Cin, Cout, with_part=True):
    """one launch with `shape` forced -> (out, partials or None, the shape that ran); the hook is back at -1 afterwards"""
    from var_amd import hip
    out = torch.full((B, H, W, Cout), float('nan'), device='cuda')
    # H * W / 128 blocks of 16 x 8 pixels on both shapes (varhip_conv_gn_blocks answers for Cout in whole groups of 32 only)
    part = torch.full((B, H * W // 128, Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if with_part else None
    hip.wino_force_shape(shape)
    try:
        util.guarded_call('conv3x3_wino_nhwc_f32', x, u, bias, resid, out, part, B, H, W, Cin, Cout)
        ran = hip.wino_last_shape()
    finally:
        hip.wino_force_shape(-1)
    return out, part, ran


# 16 x 16: one patch, every border; 32 x 16: two patches in a column; 32 x 32: patch edges inside the image.  Cin = 32: the peeled last pair alone
@pytest.mark.parametrize('H,W', [(16, 16), (32, 16), (32, 32)])
@pytest.mark.parametrize('Cin', [32, 64, 160])
@pytest.mark.parametrize('Cout', [80, 160])
def test_wide_equals_shape0_bit_for_bit(H, W, Cin, Cout):
    from var_amd.engine import wino_filter
    # Shape 0 needs whole groups of 32 channels, so it has no Cout = 80.  An output channel depends on its own filter, bias and residual
    # alone: there shape 0 runs the same problem padded to 160 channels and its first 80 channels (output and partials) are the twin.
    C0 = 160
    for B in (1, 3):
        x, wt0, bias0, resid0 = _data(B, H, Cin, C0, seed=H + W + Cin + Cout + B, W=W)
        wt, bias, resid = wt0[:Cout].contiguous(), bias0[:Cout].contiguous(), resid0[..., :Cout].contiguous()
        u, u0 = wino_filter(wt), wino_filter(wt0)
        for with_resid in (False, True):
            for with_part in (False, True):
                rs, rs0 = (resid, resid0) if with_resid else (None, None)
                y1, p1, ran1 = _run(1, x, u, bias, rs, B, H, W, Cin, Cout, with_part)
                y0, p0, ran0 = _run(0, x, u0, bias0, rs0, B, H, W, Cin, C0, with_part)
                y0, p0 = y0[..., :Cout], (p0[:, :, :Cout] if with_part else None)
                what = f'B={B} {H}x{W} {Cin}->{Cout} resid={with_resid} part={with_part}'
                assert (ran1, ran0) == (1, 0), what
                assert not torch.isnan(y1).any() and torch.equal(y1, y0), what
                if with_part:
                    assert not torch.isnan(p1).any() and torch.equal(p1, p0), what


@pytest.mark.parametrize('Cout', [96, 32])
def test_forced_wide_falls_back_where_cout_is_no_multiple_of_80(Cout):
    from var_amd.engine import wino_filter
    B, H, Cin = 2, 32, 64
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=Cout)
    u = wino_filter(wt)
    y1, p1, ran1 = _run(1, x, u, bias, resid, B, H, H, Cin, Cout)
    y0, p0, ran0 = _run(0, x, u, bias, resid, B, H, H, Cin, Cout)
    assert (ran1, ran0) == (0, 0)
    assert not torch.isnan(y1).any() and torch.equal(y1, y0) and torch.equal(p1, p0)


@pytest.mark.parametrize('H,W,Cin,Cout', [(32, 16, 64, 160), (32, 32, 160, 80)])
def test_wide_batch_invariant(H, W, Cin, Cout):
    """image i of B = 3 equals the B = 1 run of that image, output and partials"""
    from var_amd.engine import wino_filter
    B = 3
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=5, W=W)
    u = wino_filter(wt)
    yb, pb, ran = _run(1, x, u, bias, resid, B, H, W, Cin, Cout)
    assert ran == 1
    for i in range(B):
        y1, p1, _ = _run(1, x[i:i + 1].contiguous(), u, bias, resid[i:i + 1].contiguous(), 1, H, W, Cin, Cout)
        assert torch.equal(y1[0], yb[i]) and torch.equal(p1[0], pb[i]), i


@pytest.mark.parametrize('H,W,Cin,Cout', [(32, 32, 160, 160), (48, 16, 64, 80), (16, 16, 640, 640)])
@pytest.mark.parametrize('with_resid', [False, True])
def test_wide_vs_float64(H, W, Cin, Cout, with_resid):
    """the wide kernel's own error against a float64 convolution, next to the direct kernel's on the same input: at most 2x (the bar of
    tests/test_winograd_gpu.py), and the partials are the block sums of the output it wrote"""
    from var_amd.engine import wino_filter
    B = 2
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=7, W=W)
    rs = resid if with_resid else None
    yw, part, ran = _run(1, x, wino_filter(wt), bias, rs, B, H, W, Cin, Cout)
    assert ran == 1
    yd = _direct(x, wt, bias, rs, B, H, W, Cin, Cout)
    r = _ref64(x, wt, bias, rs)
    ew, ed = (yw.double() - r).abs().max().item(), (yd.double() - r).abs().max().item()
    print(f'wide B={B} {H}x{W} {Cin}->{Cout} resid={with_resid}: |wide - f64| {ew:.3g}, |direct - f64| {ed:.3g}, ratio {ew / ed:.3f}')
    assert ed > 0 and ew <= 2 * ed
    blk = yw.double().view(B, H // 16, 2, 8, W // 16, 16, Cout).permute(0, 1, 4, 2, 3, 5, 6).reshape(B, -1, 128, Cout)
    torch.testing.assert_close(part[..., 0], blk.sum(2), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(part[..., 1], (blk * blk).sum(2), rtol=1e-12, atol=1e-9)
