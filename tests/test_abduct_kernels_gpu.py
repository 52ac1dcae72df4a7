"""varhip_exp1_posterior_f32 on the MI355X: bit-equal to its host twin (pinned by tests/test_abduct_cpu.py) with every operand
between guard bands and the outputs pre-filled with sentinels; its noise, fed to varhip_cfg_sample_rows_f32 on the device, returns the given
tokens on every unflagged row under both settings of varhip_sampler_force_walk; flagged rows and refused calls as on the host."""
import numpy as np
import pytest

from tests import util
from tests.test_abduct_cpu import TS, V_REPAIR, _profiles, _twin, candidates, clamp_case, repair_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

F = np.float32
SHAPES = [(3, 1, 4096), (5, 169, 4096), (2, 16, 8192), (4, 9, 256)]
FLAG_SENTINEL = -9


def _hip():
    from var_amd import hip
    return hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outputs(rows, V):
    noise = torch.empty(rows, V, device='cuda'); _bits(noise).fill_(-1)                  # 0xFF bytes: a NaN the kernel never produces
    logp = torch.empty(rows, device='cuda'); _bits(logp).fill_(-1)
    flag = torch.full((rows,), FLAG_SENTINEL, dtype=torch.int32, device='cuda')
    return noise, logp, flag


def _kernel(logits, t, gt, seeds, B, l, V, scale, ld_gt=None, ld_out=None):
    ld_gt, ld_out = ld_gt or l, ld_out or l
    noise, logp, flag = _outputs(B * ld_out, V)
    util.guarded_call('exp1_posterior_f32', _dev(np.asarray(logits, F)), _dev(np.asarray(t, np.float64)), _dev(np.asarray(gt, np.int64)), ld_gt,
                      _dev(np.asarray(seeds, np.int64)), B, l, V, scale, noise, logp, flag, ld_out)
    return noise, logp, flag


def _case(B, l, V, seed):
    """random rows with per-image t; the first rows of image 0 are test_abduct_cpu's profiles (ties, constant, arg-max, least likely)"""
    rng = np.random.default_rng(seed)
    lg = (3.0 * rng.standard_normal((2, B, l, V))).astype(F)
    t = [TS[b % 3] * (1 + b // 3) for b in range(B)]
    gt = np.empty((B, l), np.int64)
    for b in range(B):
        x = ((F(1.0 + t[b]) * lg[0, b]).astype(F) - (F(t[b]) * lg[1, b]).astype(F)).astype(F)
        for j in range(l):
            gt[b, j] = int(rng.choice(np.flatnonzero(x[j] - x[j].max() > -60.0)))
    plg, pgt, _ = _profiles(V, seed)
    n = min(l, plg.shape[2])
    lg[:, 0, :n] = plg[:, 0, :n]                                            # (image 0 of the profiles has t = TS[0] = t[0])
    gt[0, :n] = pgt[0, :n]
    return lg.reshape(2 * B * l, V), t, gt


def _same(dev, host):
    for d, h, what in zip(dev, host, ('noise', 'logp', 'flag')):
        got = d.cpu().numpy()
        assert np.array_equal(got.view(np.uint32).reshape(-1), h.view(np.uint32).reshape(-1)), what


def _replay(logits, noise, gt, flag, t, B, l, V):
    hip = _hip()
    lg, td = _dev(logits), _dev(np.asarray(t, np.float64))
    k0, p0 = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.float64, device='cuda')
    keep = torch.from_numpy(flag == 0).cuda()
    want = _dev(gt.reshape(-1))
    try:
        for walk in (0, 1):
            hip.lib().so.varhip_sampler_force_walk(walk)
            idx = torch.full((B * l,), -7, dtype=torch.int64, device='cuda')
            util.guarded_call('cfg_sample_rows_f32', lg, noise, idx, None, B, l, V, td, k0, p0, V)
            assert torch.equal(idx[keep], want[keep]), (walk, int((idx[keep] != want[keep]).sum()))
    finally:
        hip.lib().so.varhip_sampler_force_walk(0)


@pytest.mark.parametrize('B, l, V', SHAPES)
def test_kernel_equals_the_host_twin_and_the_sampler_replays_gt(B, l, V):
    logits, t, gt = _case(B, l, V, seed=B + l + V)
    seeds = [17 + 7919 * b for b in range(B)]
    host = _twin(logits, t, gt.reshape(-1), seeds, B, l, V, 4)
    assert not host[2].any()
    dev = _kernel(logits, t, gt.reshape(-1), seeds, B, l, V, 4)
    _same(dev, host)
    _replay(logits, dev[0], gt, host[2], t, B, l, V)


def test_v_below_a_wave_of_float4_lanes():
    """V = 8: two of the 256 lanes hold a float4, every other lane adds nothing to the row sum (the sampler itself takes V % 256 == 0 only)"""
    B, l, V = 2, 3, 8
    logits, t, gt = _case(B, l, V, seed=8)
    host = _twin(logits, t, gt.reshape(-1), [1, 2], B, l, V, 0)
    _same(_kernel(logits, t, gt.reshape(-1), [1, 2], B, l, V, 0), host)


def test_five_scales_with_per_image_t_and_leading_dimensions():
    B, V, L = 3, 4096, 57
    pns = (1, 2, 3, 4, 5)
    seeds, cfg = [3, 1 << 40, (1 << 62) + 5], [1.5, 0.0, 4.0]
    cur = 0
    for si, pn in enumerate(pns):
        l = pn * pn
        t = [c * (si / (len(pns) - 1)) for c in cfg]
        logits, _, gts = _case(B, l, V, seed=100 + si)
        # (the case's tokens were chosen for its own t: rows whose token has probability 0 under this t are flagged, on both sides alike)
        gt = np.full((B, L), -3, np.int64); gt[:, cur:cur + l] = gts
        gflat = gt.reshape(-1)[cur:cur + (B - 1) * L + l]                  # the scale's slice of the (B, L) tokens: image b's at b * L
        host = _twin(logits, t, gflat, seeds, B, l, V, si, ld_gt=L, ld_out=L - cur)
        dev = _kernel(logits, t, gflat, seeds, B, l, V, si, ld_gt=L, ld_out=L - cur)
        rows = np.zeros((B, L - cur), bool); rows[:, :l] = True
        for d, h, sentinel in zip(dev, host, (-1, -1, FLAG_SENTINEL)):
            got = d.cpu().numpy().view(np.int32).reshape(B, L - cur, -1)
            assert np.array_equal(got[rows], h.view(np.int32).reshape(B, L - cur, -1)[rows])
            assert bool((got[~rows] == sentinel).all())                   # the rows between the images' slices: not written
        flag = host[2].reshape(B, L - cur)[:, :l].reshape(-1)
        noise = dev[0].view(B, L - cur, V)[:, :l].reshape(B * l, V).contiguous()
        _replay(logits, noise, gts, flag, t, B, l, V)
        cur += l


def test_repaired_entries_and_clamped_winners_on_the_device():
    """test_abduct_cpu's rows built to need the one-ulp raises, and its rows whose winner's noise is clamped at FLT_MIN: the kernel equals the
    twin on them, entries do sit above their candidates, and the device sampler returns gt from the repaired noise under both walk settings"""
    for (logits, t, gt, seeds), scale, least in ((repair_case()[:4], 0, 100), (clamp_case(), 2, 200)):
        B, V = len(gt), V_REPAIR
        host = _twin(logits, t, gt, seeds, B, 1, V, scale)
        assert not host[2].any()
        dev = _kernel(logits, t, gt, seeds, B, 1, V, scale)
        _same(dev, host)
        cand = candidates(logits, t, seeds, B, V, scale)[0]
        losers = np.ones((B, V), bool); losers[np.arange(B), gt] = False
        assert int((dev[0].cpu().numpy()[losers] > cand[losers]).sum()) >= least
        _replay(logits, dev[0], gt, host[2], t, B, 1, V)


def test_flagged_rows_hold_the_prior_fill():
    V, B, l = 4096, 1, 6
    rng = np.random.default_rng(9)
    lg = (2.0 * rng.standard_normal((2, l, V))).astype(F)
    gt = rng.integers(0, V, size=l)
    lg[0, 1, gt[1]] = -np.inf; lg[1, 1, gt[1]] = 0.0
    lg[0, 2, 17] = np.nan
    gt[3], gt[4] = -1, V
    logits = lg.reshape(2 * l, V)
    host = _twin(logits, [0.0], gt, [3], B, l, V, 1)
    dev = _kernel(logits, [0.0], gt, [3], B, l, V, 1)
    assert dev[2].tolist() == [0, 1, 1, 1, 1, 0]
    _same(dev, host)
    fill = torch.empty(l, V, device='cuda')
    util.guarded_call('exp1_philox_f32', _dev(np.asarray([3], np.int64)), B, l, V, 1, 2, fill)
    bad = dev[2] == 1
    assert torch.equal(_bits(dev[0][bad]), _bits(fill[bad])) and bool(torch.isneginf(dev[1][bad]).all())
    _replay(logits, dev[0], gt, host[2], [0.0], B, l, V)


def test_refused_calls_write_nothing():
    hip = _hip()
    from var_amd import abi
    B, l, V = 2, 3, 256
    lg = torch.zeros(2 * B * l * V + 4, device='cuda')
    t64 = torch.zeros(B, dtype=torch.float64, device='cuda')
    gt = torch.zeros(B * l, dtype=torch.int64, device='cuda')
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    noise, logp, flag = _outputs(B * l + 1, V)
    fn, st = hip.lib().fn['exp1_posterior_f32'], hip.current_stream()
    invoke = lambda *a: fn(*a, st)
    #       0                    1    2   3  4   5  6  7  8  9                 10             11             12
    good = [lg[:2 * B * l * V], t64, gt, l, sd, B, l, V, 0, noise[:B * l], logp[:B * l], flag[:B * l], l]
    bad = [(0, lg[1:2 * B * l * V + 1]), (9, noise.view(-1)[1:B * l * V + 1]), (7, V - 2), (7, 0), (7, 8196), (5, 0), (6, 0), (8, -1), (3, l - 1),
           (12, l - 1), (0, None), (1, None), (2, None), (4, None), (9, None), (10, None), (11, None)]
    for pos, val in bad:
        a = list(good); a[pos] = val
        rc = util.guarded_invoke('varhip_exp1_posterior_f32', a, invoke, torch.cuda.synchronize)
        assert rc == abi.EINVAL, (pos, val, rc)
        assert bool((_bits(noise) == -1).all()) and bool((_bits(logp) == -1).all()) and bool((flag == FLAG_SENTINEL).all()), (pos, val)
    assert util.guarded_invoke('varhip_exp1_posterior_f32', good, invoke, torch.cuda.synchronize) == 0
    assert bool((flag[:B * l] == 0).all()) and not bool((_bits(noise[:B * l]) == -1).any())
