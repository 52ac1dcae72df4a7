"""varhip_conv3x3_wino_nhwc_f32 under its pipelined schedule (var_amd/csrc/winograd.hip): what a K loop with counted
waits, a peeled last K tile and early epilogue loads puts at risk and tests/test_winograd_gpu.py does not exercise.

Bars are that file's: against float64 the Winograd error is at most 2x the direct kernel's on the same data, and the two kernels differ by at
most 3x the direct error.  Everything else here is bit-for-bit (torch.equal): the K order is fixed, so an image's result depends neither on
the batch, nor on how many workgroups a launch has, nor on when its workgroups run.
"""
import pytest

torch = pytest.importorskip('torch')

from tests import util
from tests.test_winograd_gpu import _data, _direct, _ref64

pytestmark = pytest.mark.gpu


def _wino_nan(x, u, bias, resid, B, H, W, Cin, Cout, with_part=True):
    """output and partials prefilled with NaN: whatever the launch does not write stays visible"""
    from var_amd import hip
    out = torch.full((B, H, W, Cout), float('nan'), device='cuda')
    part = torch.full((B, hip.conv_gn_blocks(H, W, Cout), Cout, 2), float('nan'), dtype=torch.float64, device='cuda') if with_part else None
    util.guarded_call('conv3x3_wino_nhwc_f32', x, u, bias, resid, out, part, B, H, W, Cin, Cout)
    return out, part


@pytest.mark.parametrize('Cin,Cout', [(32, 32), (32, 320), (64, 32), (64, 640)])
@pytest.mark.parametrize('with_resid', [False, True])
@pytest.mark.parametrize('with_part', [False, True])
def test_shortest_k_loops(Cin, Cout, with_resid, with_part):
    """Cin = 32 is two K tiles (the peeled last pair alone: prologue and epilogue of the pipeline meet), Cin = 64 one trip of the loop before it;
    Cout = 32 is one channel group per patch, 320 / 640 many"""
    from var_amd.engine import wino_filter
    B, H = 2, 32
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=Cin + Cout)
    rs = resid if with_resid else None
    yw, part = _wino_nan(x, wino_filter(wt), bias, rs, B, H, H, Cin, Cout, with_part)
    yd = _direct(x, wt, bias, rs, B, H, H, Cin, Cout)
    r = _ref64(x, wt, bias, rs)
    assert not torch.isnan(yw).any()
    ew, ed = (yw.double() - r).abs().max().item(), (yd.double() - r).abs().max().item()
    print(f'{H}x{H} {Cin}->{Cout} resid={with_resid} part={with_part}: |wino - f64| {ew:.3g}, |direct - f64| {ed:.3g}')
    assert ed > 0 and ew <= 2 * ed
    assert (yw - yd).abs().max().item() <= 3 * ed
    if with_part:
        assert not torch.isnan(part).any()
        # block 2 t + h = 8-row half h of 16 x 16 patch t: every block's channel sums and sums of squares against the output itself
        blk = yw.double().view(B, H // 16, 2, 8, H // 16, 16, Cout).permute(0, 1, 4, 2, 3, 5, 6).reshape(B, -1, 128, Cout)
        torch.testing.assert_close(part[..., 0], blk.sum(2), rtol=1e-12, atol=1e-9)
        torch.testing.assert_close(part[..., 1], (blk * blk).sum(2), rtol=1e-12, atol=1e-9)


# one workgroup in the launch; a count that is neither a multiple of the resident workgroups nor of the 8 XCDs (3 * 9 * 5 = 135); many rounds
@pytest.mark.parametrize('B,H,W,Cin,Cout,alone', [(1, 16, 16, 64, 32, (0,)), (3, 48, 48, 64, 160, (0, 1, 2)), (64, 64, 64, 160, 320, (0, 31, 63))])
def test_work_item_count_against_resident_workgroups(B, H, W, Cin, Cout, alone):
    """every output element and every (block, channel) partial is written, and the values are those of each image run alone"""
    from var_amd.engine import wino_filter
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=B + H, W=W)
    u = wino_filter(wt)
    yb, pb = _wino_nan(x, u, bias, resid, B, H, W, Cin, Cout)
    assert not torch.isnan(yb).any() and not torch.isnan(pb).any()
    for i in alone:
        y1, p1 = _wino_nan(x[i:i + 1].contiguous(), u, bias, resid[i:i + 1].contiguous(), 1, H, W, Cin, Cout)
        assert torch.equal(y1[0], yb[i]), i
        assert torch.equal(p1[0], pb[i]), i


@pytest.mark.parametrize('H,Cin,Cout', [(256, 160, 160), (16, 640, 640)])
def test_batch_invariant_at_the_end_levels(H, Cin, Cout):
    """B = 64 against images 0, 17 and 63 alone, bit for bit, at the two levels tests/test_winograd_gpu.py::test_wino_batch_invariant leaves out"""
    from var_amd.engine import wino_filter
    B = 64
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=2)
    u = wino_filter(wt)
    yb, pb = _wino_nan(x, u, bias, resid, B, H, H, Cin, Cout)
    for i in (0, 17, 63):
        y1, p1 = _wino_nan(x[i:i + 1].contiguous(), u, bias, resid[i:i + 1].contiguous(), 1, H, H, Cin, Cout)
        assert torch.equal(y1[0], yb[i]), i
        assert torch.equal(p1[0], pb[i]), i


def test_same_call_twice_same_bits():
    """256^2, 160 -> 160, residual and partials, B = 8 (81 920 / 8 workgroups: 20 rounds over the chip): the same inputs into a fresh NaN-filled
    output give the same bits.  A workgroup's epilogue exchange reuses the LDS of its K-loop stages and its neighbour on the CU is in another
    phase on every run, so a read ahead of its wait or a DMA into LDS still being read shows up as a difference here"""
    from var_amd.engine import wino_filter
    B, H, Cin, Cout = 8, 256, 160, 160
    x, wt, bias, resid = _data(B, H, Cin, Cout, seed=3)
    u = wino_filter(wt)
    y0, p0 = _wino_nan(x, u, bias, resid, B, H, H, Cin, Cout)
    y1, p1 = _wino_nan(x, u, bias, resid, B, H, H, Cin, Cout)
    assert not torch.isnan(y0).any() and not torch.isnan(p0).any()
    assert torch.equal(y0, y1) and torch.equal(p0, p1)
