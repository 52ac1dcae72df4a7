"""varhip_token_lens_f32 on the MI355X: bit for bit its host twin and, for nll / pred / rank, varhip_token_eval_f32, on the planted rows of
tests/lensref.py, written into slices of larger sentinel-filled outputs; the exact zero of kl on equal rows; the refusals.  Every call is guarded."""
import pytest
import torch

from tests import lensref as LR
from tests import util
from var_amd import hip

pytestmark = pytest.mark.gpu

R_, L_ = 3, 7
# (N, L, r0, tok0) of the (N, L) outputs the (R_, L_) slice is written into; the last one ends the allocation
LAYOUTS = [(5, 19, 1, 4), (R_ + 2, L_ + 6, 2, 6)]
_C = {}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _outs(N, L, dev='cuda'):
    return [torch.full((N, L), LR.SENT_F, device=dev), torch.full((N, L), LR.SENT_F, device=dev), torch.full((N, L), LR.SENT_F, device=dev),
            torch.full((N, L), LR.SENT_I, dtype=torch.int64, device=dev), torch.full((N, L), LR.SENT_I, dtype=torch.int32, device=dev)]


def _case(V):
    """the planted rows, the twin's outputs (computed once per V) and the rows on the device"""
    if V not in _C:
        z, zf, gt = LR.rows(V, R_, L_, V)
        _C[V] = (z, zf, gt, LR.run_host(z, zf, gt, R_, L_, V), z.cuda(), zf.cuda())
    return _C[V]


@pytest.mark.parametrize('layout', LAYOUTS, ids=['inside', 'ends the allocation'])
@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
def test_kernel_is_its_host_twin_and_token_eval(V, layout):
    N, L, r0, tok0 = layout
    z, zf, gt_rows, want, zd, zfd = _case(V)
    gt = torch.randint(0, V, (N, L), generator=torch.Generator().manual_seed(1)).cuda()
    gt[r0:r0 + R_, tok0:tok0 + L_] = gt_rows.cuda()
    o = _outs(N, L)
    util.guarded_call('token_lens_f32', zd, zfd, gt[r0:, tok0:], L, R_, L_, V, *[t[r0:, tok0:] for t in o], L)
    torch.cuda.synchronize()
    for name, got, ref, w in zip(('nll', 'entropy', 'kl', 'pred', 'rank'), o, _outs(N, L), want):
        assert torch.equal(bits(got[r0:r0 + R_, tok0:tok0 + L_]).cpu(), bits(w)), f'{name} differs from the host twin'
        got = got.clone()
        got[r0:r0 + R_, tok0:tok0 + L_] = ref[r0:r0 + R_, tok0:tok0 + L_]
        assert torch.equal(got, ref), f'{name}: written outside the slice'
    e = _outs(N, L)
    util.guarded_call('token_eval_f32', zd, gt[r0:, tok0:], L, R_, L_, V, e[0][r0:, tok0:], e[1][r0:, tok0:], e[3][r0:, tok0:], e[4][r0:, tok0:], L)
    torch.cuda.synchronize()
    for name, i in (('nll', 0), ('pred', 3), ('rank', 4)):
        assert torch.equal(bits(o[i]), bits(e[i])), f'{name} differs from varhip_token_eval_f32'


@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
def test_equal_rows_give_exactly_zero(V):
    z, zf, gt_rows, want, zd, zfd = _case(V)
    gt = gt_rows.cuda()
    same, copy = _outs(R_, L_), _outs(R_, L_)
    util.guarded_call('token_lens_f32', zd, zd, gt, L_, R_, L_, V, *same, L_)
    util.guarded_call('token_lens_f32', zd, zd.clone(), gt, L_, R_, L_, V, *copy, L_)
    torch.cuda.synchronize()
    keep = torch.ones(R_ * L_, dtype=torch.bool)
    keep[LR.NAN_ROW] = False
    for o in (same, copy):
        k = o[2].view(-1).cpu()
        assert bool(torch.isnan(k[LR.NAN_ROW])) and torch.equal(bits(k[keep]), torch.zeros(R_ * L_ - 1, dtype=torch.int32)), 'kl is not +0.0'
        for i in (0, 1, 3, 4):                                 # everything of the layer row is what the distinct-buffer call gives
            assert torch.equal(bits(o[i]).cpu(), bits(want[i]))


def test_refusals_leave_the_outputs_untouched():
    V = 1000
    z, zf, gt_rows, want, zd, zfd = _case(V)
    gt = gt_rows.cuda()
    good = dict(ld_gt=L_, R=R_, l=L_, V=V, ld_out=L_)
    for bad in (dict(R=0), dict(l=0), dict(V=0), dict(R=-1), dict(ld_gt=L_ - 1), dict(ld_out=L_ - 1), *[dict(null=i) for i in range(8)]):
        a = dict(good, **{k: v for k, v in bad.items() if k != 'null'})
        o = _outs(R_, L_)
        ops = [zd, zfd, gt] + o
        if 'null' in bad:
            ops[bad['null']] = None
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('token_lens_f32', *ops[:3], a['ld_gt'], a['R'], a['l'], a['V'], *ops[3:], a['ld_out'])
        torch.cuda.synchronize()
        for t, ref in zip(o, _outs(R_, L_)):
            assert torch.equal(t, ref), bad
