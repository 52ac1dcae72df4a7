"""varhip_dla_target_f32, varhip_dla_direction_f32 and varhip_rowdot_seg_f64 on the MI355X: bit for bit their host twins (pinned against the numpy
restatement by tests/test_dla_cpu.py) on the same deck, padded leading dimensions included, and the refusals.  Every call is guarded.
(varhip_adaln_block_f32 leaves the stream behind the attention residual in x2 and the proj input in att when it returns, so
VAR.logit_attribution needs no tapped block and there is none to pin.)"""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_dla_cpu import SENT, direction_case, host, same, target_case
from var_amd import hip

pytestmark = pytest.mark.gpu

cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('V', [5, 4096, 4100])
@pytest.mark.parametrize('R, l', [(1, 1), (3, 4), (3, 9), (2, 256)])
def test_target_is_its_host_twin(R, l, V):
    z, gt, ag = target_case(R, l, V, V + l)
    ld = l + 3
    pad = lambda a: np.concatenate([a.astype(np.int64), np.full((R, 3), -1, np.int64)], 1)
    gtp, agp = pad(gt), pad(ag)
    for mode in (0, 1, 2):
        rival, value = np.full((R, ld), -9, np.int64), np.full((R, ld), SENT, np.float32)
        assert host('dla_target_host_f32', z, gtp, agp if mode == 2 else None, ld, mode, R, l, V, rival, value, ld) == 0
        for zd in (cu(z), cu(np.concatenate([np.zeros(1, np.float32), z.reshape(-1)]))[1:].view(R, l, V)):          # 16-byte aligned and not
            rd, vd = cu(np.full((R, ld), -9, np.int64)), cu(np.full((R, ld), SENT, np.float32))
            util.guarded_call('dla_target_f32', zd, cu(gtp), cu(agp) if mode == 2 else None, ld, mode, R, l, V, rd, vd, ld)
            assert np.array_equal(rd.cpu().numpy(), rival) and same(vd.cpu().numpy(), value), (mode, zd.data_ptr() % 16)


@pytest.mark.parametrize('C', [128, 1024])
@pytest.mark.parametrize('R, l, V', [(1, 1, 5), (3, 4, 4100), (3, 9, 5), (2, 256, 4096)])
def test_direction_is_its_host_twin(R, l, C, V):
    x, hn, W, b, a, r = direction_case(R, l, C, V, C + l)
    ld, ldo = l + 2, l + 1
    pad = lambda t: np.concatenate([t, np.full((R, 2), -1, np.int64)], 1)
    hnd = cu(hn)
    for rival in (None, r):
        ghat, konst, gx = np.full((R * l, C), SENT, np.float32), np.full((R, ldo), -3.0), np.full((R, ldo), -3.0)
        assert host('dla_direction_host_f32', x, hn, hn[:, C:], hn.shape[1], W, b, pad(a), None if rival is None else pad(rival), ld, R, l, C, V,
                    1e-6, ghat, konst, gx, ldo) == 0
        gd, kd, xd = cu(np.full((R * l, C), SENT, np.float32)), cu(np.full((R, ldo), -3.0)), cu(np.full((R, ldo), -3.0))
        util.guarded_call('dla_direction_f32', cu(x), hnd, hnd[:, C:], hn.shape[1], cu(W), cu(b), cu(pad(a)), None if rival is None else cu(pad(rival)),
                          ld, R, l, C, V, 1e-6, gd, kd, xd, ldo)
        assert same(gd.cpu().numpy(), ghat) and same(kd.cpu().numpy(), konst) and same(xd.cpu().numpy(), gx), rival is None


@pytest.mark.parametrize('C, nseg', [(128, 1), (128, 2), (1024, 1), (1024, 16), (1024, 4), (24, 2), (12, 1), (4, 1)])
@pytest.mark.parametrize('M', [1, 9, 257, 768])
def test_rowdot_is_its_host_twin(M, C, nseg):
    g = np.random.default_rng(M + C + nseg)
    lda, ldb = C + 4, C + 8
    a, b = np.full((M, lda), np.nan, np.float32), np.full((M, ldb), np.nan, np.float32)
    a[:, :C] = (g.standard_normal((M, C)) * 1e3).astype(np.float32)
    b[:, :C] = g.standard_normal((M, C)).astype(np.float32)
    for bb, ld in ((b, ldb), (b[0, :C].copy(), 0)):
        want = np.full((M, nseg), -3.0)
        assert host('rowdot_seg_host_f64', a, lda, bb, ld, M, C, nseg, want) == 0
        got = cu(np.full((M, nseg), -3.0))
        util.guarded_call('rowdot_seg_f64', cu(a), lda, cu(bb), ld, M, C, nseg, got)
        assert same(got.cpu().numpy(), want), ld


def test_refusals_leave_the_outputs_untouched():
    M, C = 3, 128
    a, b = torch.ones(M, C, device='cuda'), torch.ones(M, C, device='cuda')
    shifted = torch.ones(M * C + 4, device='cuda')[1:1 + M * C].view(M, C)
    for bad in (dict(M=0), dict(C=0), dict(nseg=0), dict(nseg=3), dict(C=126, nseg=1), dict(lda=C - 4), dict(ldb=C + 2), dict(null=0), dict(null=1),
                dict(null=2), dict(odd=0), dict(odd=1)):
        k = dict(dict(lda=C, ldb=C, M=M, C=C, nseg=2), **{key: v for key, v in bad.items() if key not in ('null', 'odd')})
        out = torch.full((M, 2), -3.0, dtype=torch.float64, device='cuda')
        ops = [a, b, out]
        if 'null' in bad:
            ops[bad['null']] = None
        if 'odd' in bad:
            ops[bad['odd']] = shifted
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('rowdot_seg_f64', ops[0], k['lda'], ops[1], k['ldb'], k['M'], k['C'], k['nseg'], ops[2])
        assert bool((out == -3.0).all()), bad
    R, l, V = 2, 3, 8
    z, gt = torch.zeros(R, l, V, device='cuda'), torch.zeros(R, l, dtype=torch.int64, device='cuda')
    for bad in (dict(R=0), dict(V=0), dict(mode=3), dict(ld=l - 1), dict(null=0), dict(null=1), dict(null=3), dict(null=4), dict(mode=2)):
        k = dict(dict(R=R, V=V, mode=1, ld=l), **{key: v for key, v in bad.items() if key != 'null'})
        rival, value = torch.full((R, l), -9, dtype=torch.int64, device='cuda'), torch.full((R, l), float(SENT), device='cuda')
        ops = [z, gt, None, rival, value]
        if 'null' in bad:
            ops[bad['null']] = None
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('dla_target_f32', ops[0], ops[1], ops[2], k['ld'], k['mode'], k['R'], l, k['V'], ops[3], ops[4], k['ld'])
        assert bool((rival == -9).all()) and bool((value == float(SENT)).all()), bad
    C = 128
    x, hn, W, b_ = torch.zeros(R * l, C, device='cuda'), torch.zeros(R, 2 * C, device='cuda'), torch.zeros(V, C, device='cuda'), torch.zeros(V, device='cuda')
    for bad in (dict(C=126), dict(R=0), dict(ld_hn=C - 4), dict(eps=-1.0), dict(null=0), dict(null=3), dict(null=5), dict(null=7), dict(null=9)):
        k = dict(dict(R=R, C=C, ld_hn=2 * C, eps=1e-6), **{key: v for key, v in bad.items() if key != 'null'})
        ghat = torch.full((R * l, C), float(SENT), device='cuda')
        konst, gx = torch.full((R, l), -3.0, dtype=torch.float64, device='cuda'), torch.full((R, l), -3.0, dtype=torch.float64, device='cuda')
        ops = [x, hn, hn[:, C:], W, b_, gt, None, ghat, konst, gx]
        if 'null' in bad:
            ops[bad['null']] = None
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('dla_direction_f32', *ops[:3], k['ld_hn'], *ops[3:7], l, k['R'], l, k['C'], V, k['eps'], *ops[7:], l)
        assert bool((ghat == float(SENT)).all()) and bool((konst == -3.0).all()) and bool((gx == -3.0).all()), bad
