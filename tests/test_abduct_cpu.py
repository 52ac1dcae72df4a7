"""varhip_exp1_posterior_host_f32, the parts that need no GPU:
  (a) the host twin equals tests/abductref.py's numpy restatement bit for bit (noise, logp, flags)
  (b) its noise, replayed through the oracle's sampler (varref_cfg_sample_f32, the scalar entry, image by image), returns the given tokens
  (c) flags are raised for exactly the planted cases, their rows hold the draw-2 fill, a refused call writes nothing
  (d) the law: with g itself drawn by the sampler from the prior fill, every coordinate of the posterior noise is Exp(1) again
      (Kolmogorov-Smirnov at the 0.1 % critical value 1.95 / sqrt(n)), and two planted faults in the restatement are caught by the same bar
  (e) raising the winner's logit keeps the winner under the abducted noise (Gumbel-max monotonicity) and grows its odds

The oracle's sampler takes V % 256 == 0, so the law test's row of 8 codes is a row of 256 whose other 248 codes have probability exactly 0
(vm_exp gives 0 below -87); their coordinates must be the fresh fill itself."""
import numpy as np
import pytest

from tests import abductref as R
from tests import util

F = np.float32
TS = (0.0, 0.75, 4.0)


def _host(name, *args):
    from var_amd import hip
    hip.call_host(name, *args)


def _twin(logits, t, gt, seeds, B, l, V, scale, ld_gt=None, ld_out=None):
    ld_gt, ld_out = ld_gt or l, ld_out or l
    gt = np.ascontiguousarray(gt, np.int64)
    noise = np.full((B * ld_out, V), np.nan, F)
    logp = np.full(B * ld_out, np.nan, F)
    flag = np.full(B * ld_out, -9, np.int32)
    _host('exp1_posterior_host_f32', np.ascontiguousarray(logits, F), np.ascontiguousarray(t, np.float64), gt, ld_gt,
          np.ascontiguousarray(seeds, np.int64), B, l, V, scale, noise, logp, flag, ld_out)
    return noise, logp, flag


def _oracle_sample(logits, noise, B, l, V, t):
    """the oracle's sampler without filters, image by image (its entry takes one t): -> (B * l,) tokens"""
    from oracle import var_oracle as O
    util.ensure_oracle_built()
    fn = O.lib()['cfg_sample_f32']
    lg = np.asarray(logits, F).reshape(2, B, l, V)
    out = np.full(B * l, -5, np.int64)
    for b in range(B):
        pair = np.ascontiguousarray(lg[:, b].reshape(2 * l, V))
        idx = np.full(l, -5, np.int64)
        assert fn(O._p(pair), O._p(np.ascontiguousarray(noise[b * l:(b + 1) * l])), O._p(idx), None, 1, l, V, float(t[b]), 0, 0.0) == 0
        out[b * l:(b + 1) * l] = idx
    return out


def _profiles(V, seed):
    """one image per t in TS; rows: random; a tie crowd (> 1000 exact ties at the top); constant; g = the arg-max; g = the least likely code
    with p_g near 1e-30; random with g random -> (logits (2, B, l, V), gt (B, l), what each row is)"""
    rng = np.random.default_rng(seed)
    B, l = len(TS), 6
    lg = (3.0 * rng.standard_normal((2, B, l, V))).astype(F)
    gt = rng.integers(0, V, size=(B, l))
    for b, t in enumerate(TS):
        lg[:, b, 1] = rng.integers(0, 3, size=V).astype(F)                 # three values in both halves: the guided row has crowds of exact ties
        lg[:, b, 2] = F(0.5)
        x = R.guided(np.ascontiguousarray(lg[:, b]).reshape(2 * l, V), 1, l, [t])
        gt[b, 3] = int(np.argmax(x[3]))
        for j in (0, 5):                                                   # random among the codes whose probability is not exactly 0 (vm_exp: 0 below -87)
            gt[b, j] = int(rng.choice(np.flatnonzero(x[j] - x[j].max() > -60.0)))
        lg[:, b, 4] = 0.0
        lg[0, b, 4, 7] = F(-69.0 / (1.0 + t))                             # guided: about -69 below the rest: p = e^-69 / (V - 1), near 1e-30 / V
        gt[b, 4] = 7
        gt[b, 1] = int(np.flatnonzero(x[1] == x[1].max())[-1])             # the LAST of the tied maxima: an index tie would go to an earlier one
    ties = int((R.guided(np.ascontiguousarray(lg[:, 0]).reshape(2 * l, V), 1, l, [TS[0]])[1] == 2.0).sum())
    assert ties > 1000 or V < 4096, ties
    return lg, gt, ('random', 'ties', 'constant', 'argmax', 'least likely', 'random')


@pytest.mark.parametrize('V', [4096, 256, 8192, 8])
def test_host_twin_equals_the_numpy_restatement_and_replays_to_gt(V):
    lg, gt, _ = _profiles(V, seed=V)
    B, l = gt.shape
    seeds = [11 + 1000003 * b for b in range(B)]
    logits = lg.reshape(2 * B * l, V)
    noise, logp, flag = _twin(logits, TS, gt.reshape(-1), seeds, B, l, V, 3)
    rn, rl, rf = R.posterior(logits, TS, gt.reshape(-1), seeds, B, l, V, 3)
    assert np.array_equal(flag, rf) and not flag.any(), (flag, rf)
    assert np.array_equal(noise.view(np.uint32), rn.view(np.uint32)), np.argwhere(noise.view(np.uint32) != rn.view(np.uint32))[:5]
    assert np.array_equal(logp.view(np.uint32), rl.view(np.uint32))
    p = R.probabilities(R.guided(logits, B, l, TS))[0]
    pg = p[np.arange(B * l), gt.reshape(-1)].astype(np.float64)
    assert np.allclose(logp, np.log(pg), rtol=0, atol=2e-5 * np.maximum(1.0, np.abs(np.log(pg))))
    assert V < 256 or pg.reshape(B, l)[:, 4].max() < 1e-29
    assert bool((noise > 0).all()) and bool(np.isfinite(noise).all())
    if V % 256 == 0:                                                       # (b) the oracle's sampler takes these V
        back = _oracle_sample(logits, noise, B, l, V, TS)
        assert np.array_equal(back, gt.reshape(-1)), (back.reshape(B, l), gt)


def test_a_leading_dimension_and_a_scale_address_the_documented_rows():
    """gt and the outputs with leading dimensions above l: the rows between are neither read nor written; another scale, another noise"""
    V, B, l = 256, 2, 3
    rng = np.random.default_rng(5)
    logits = (2.0 * rng.standard_normal((2 * B * l, V))).astype(F)
    gt = rng.integers(0, V, size=(B, 7)); gt[:, l:] = -77
    seeds, t = [5, 6], [0.3, 1.1]
    noise, logp, flag = _twin(logits, t, gt, seeds, B, l, V, 2, ld_gt=7, ld_out=5)
    rn, rl, rf = R.posterior(logits, t, gt[:, :l].reshape(-1), seeds, B, l, V, 2)
    nz = noise.reshape(B, 5, V)
    assert np.array_equal(nz[:, :l].reshape(B * l, V).view(np.uint32), rn.view(np.uint32)) and bool(np.isnan(nz[:, l:]).all())
    assert np.array_equal(logp.reshape(B, 5)[:, :l].reshape(-1).view(np.uint32), rl.view(np.uint32)) and bool(np.isnan(logp.reshape(B, 5)[:, l:]).all())
    assert np.array_equal(flag.reshape(B, 5)[:, :l].reshape(-1), rf) and bool((flag.reshape(B, 5)[:, l:] == -9).all())
    other = _twin(logits, t, gt, seeds, B, l, V, 3, ld_gt=7, ld_out=5)[0]
    assert not np.array_equal(other.reshape(B, 5, V)[:, :l], nz[:, :l])


def test_flags_are_raised_for_exactly_the_planted_rows_and_refused_calls_write_nothing():
    from var_amd import hip
    V, B, l = 256, 1, 6
    rng = np.random.default_rng(9)
    lg = (2.0 * rng.standard_normal((2, l, V))).astype(F)
    gt = rng.integers(0, V, size=l)
    lg[0, 1, gt[1]] = -np.inf; lg[1, 1, gt[1]] = 0.0                      # a planted -inf at g (the unconditional entry finite: no NaN)
    lg[0, 2, 17] = np.nan                                                  # a NaN row
    gt[3], gt[4] = -1, V
    logits = lg.reshape(2 * l, V)
    noise, logp, flag = _twin(logits, [0.0], gt, [3], B, l, V, 1)
    rn, rl, rf = R.posterior(logits, [0.0], gt, [3], B, l, V, 1)
    assert flag.tolist() == [0, 1, 1, 1, 1, 0] == rf.tolist()
    fill = R.stream([3], l, V, 1, R.DRAW_FILL)
    bad = flag == 1
    assert np.array_equal(noise[bad].view(np.uint32), fill[bad].view(np.uint32)) and bool(np.isneginf(logp[bad]).all())
    assert np.array_equal(noise.view(np.uint32), rn.view(np.uint32)) and np.array_equal(logp.view(np.uint32), rl.view(np.uint32))
    assert not np.array_equal(noise[0], fill[0]) and np.isfinite(logp[[0, 5]]).all()
    # refused: V % 4 != 0, V = 0, V > 8192, B / l < 1, a negative scale, leading dimensions below l, NULL operands
    t64, sd = np.zeros(1, np.float64), np.array([3], np.int64)
    out = dict(n=np.full((l, V), np.nan, F), p=np.full(l, np.nan, F), f=np.full(l, -9, np.int32))
    good = [logits, t64, gt.astype(np.int64), l, sd, B, l, V, 1, out['n'], out['p'], out['f'], l]
    for pos, val in [(7, V - 2), (7, 0), (7, 8196), (5, 0), (6, 0), (8, -1), (3, l - 1), (12, l - 1), (0, None), (1, None), (2, None), (4, None),
                     (9, None), (10, None), (11, None)]:
        a = list(good); a[pos] = val
        with pytest.raises(hip.VarHipError, match='EINVAL'):
            _host('exp1_posterior_host_f32', *a)
        assert bool(np.isnan(out['n']).all()) and bool(np.isnan(out['p']).all()) and bool((out['f'] == -9).all()), (pos, val)
    _host('exp1_posterior_host_f32', *good)
    assert np.array_equal(out['n'].view(np.uint32), noise.view(np.uint32))


# ---- the fp32 repair and the FLT_MIN clamp ----------------------------------------------------------------------------------------------
# (seed, v): the stream's draw-2 value E_v at (seed, scale 0, t 0, v) is one of its two smallest, 2^-24 or 3 * 2^-24, and the draw-3 minimum T
# of that row is above 0.3 — the 60 such pairs among the seeds 1 .. 1.5 million at V = 256, found by a scan of the host fill (the test below
# checks both properties of every pair).  With a large p_v, fl(fl(T * p_v) + E_v) then rounds back onto, or within an ulp or two of, T * p_v,
# and the candidate does not lose the sampler's strict comparison: the entries that need the repair.
REPAIR_HITS = [(19018, 12), (26388, 92), (62609, 28), (128815, 246), (161616, 143), (192404, 54), (283848, 252), (283869, 28), (294644, 35),
               (304523, 67), (323084, 18), (323239, 0), (338330, 112), (343386, 123), (365301, 91), (378247, 194), (445806, 137), (470228, 228),
               (508251, 70), (579691, 80), (581236, 71), (630388, 18), (664946, 228), (673328, 43), (691607, 45), (712897, 51), (714392, 89),
               (719591, 201), (838202, 143), (908983, 43), (947761, 161), (974470, 99), (986057, 176), (1042108, 66), (1065780, 19), (1079865, 221),
               (1081316, 25), (1118930, 170), (1133866, 237), (1144636, 161), (1195286, 27), (1203195, 69), (1226251, 128), (1238734, 235),
               (1254819, 243), (1264638, 157), (1287899, 171), (1328274, 218), (1360571, 37), (1362412, 71), (1378781, 100), (1397077, 145),
               (1452838, 7), (1456110, 139), (1456290, 73), (1461441, 149), (1465010, 216), (1479827, 255), (1489102, 75), (1494160, 225)]
REPAIR_LOGITS = (3, 4, 5, 6, 8, 10, 12, 14, 17, 20)
V_REPAIR = 256


def repair_case():
    """one image (l = 1, t = 0, scale 0) per (pair, A): the row is 0 but for cond[v] = A, so p_v = e^A / (e^A + 255) runs from 0.07 to 1, and
    g = v + 1 -> (logits (2 * B, V), t (B,), gt (B,), seeds (B,), v (B,))"""
    rows = [(seed, v, A) for seed, v in REPAIR_HITS for A in REPAIR_LOGITS]
    B = len(rows)
    lg = np.zeros((2, B, V_REPAIR), F)
    for i, (_, v, A) in enumerate(rows):
        lg[0, i, v] = A
    v = np.array([r[1] for r in rows])
    return lg.reshape(2 * B, V_REPAIR), np.zeros(B), (v + 1) % V_REPAIR, np.array([r[0] for r in rows], np.int64), v


def candidates(logits, t, seeds, B, V, scale):
    """fl(fl(T * p_v) + E_v) of every entry, the value the repair starts from, and the row's T"""
    p = R.probabilities(R.guided(logits, B, 1, t))[0]
    E = R.stream(seeds, 1, V, scale, R.DRAW_FILL)
    T = R.stream(seeds, 1, V, scale, R.DRAW_MIN)[:, 0]
    return ((T[:, None] * p).astype(F) + E).astype(F), T, E, p


def clamp_case():
    """rows whose winner is so unlikely that fl(T * p_g) is below FLT_MIN: noise_g is clamped, r_g = p_g / FLT_MIN is far below 1 / T, and every
    other entry's closed-form start p_v / r_g lies far above its candidate.  cond[g] = -86.5 / -86.9 (vm_exp still gives about 2.7e-38 /
    1.8e-38; below -87 it gives 0 and the row is flagged), the rest 0 or random -> (logits, t, gt, seeds).  Whatever the row, the start is
    p_v / r_g = FLT_MIN * exp(x_v - x_g), about 0.4 to 0.65 for the codes at the maximum: above the candidate T * p_v + E_v wherever E_v is
    below that, a fifth to a half of the entries"""
    rng = np.random.default_rng(77)
    B, V = 6, V_REPAIR
    lg = np.zeros((2, B, V), F)
    lg[0, 3:] = rng.standard_normal((3, V)).astype(F)
    gt = np.array([5, 200, 0, 17, 255, 100])
    for b in range(B):
        lg[0, b, gt[b]] = lg[0, b].max() - F(86.5 if b % 2 else 86.9)
    return lg.reshape(2 * B, V), np.zeros(B), gt, np.arange(B, dtype=np.int64) + 4242


def test_the_repair_is_needed_and_made_on_rows_built_to_need_it():
    logits, t, gt, seeds, v = repair_case()
    B, V = len(gt), V_REPAIR
    cand, T, E, p = candidates(logits, t, seeds, B, V, 0)
    r = np.arange(B)
    assert bool((E[r, v] < 2.5e-7).all()) and bool((T > 0.3).all())          # the committed pairs are what the comment says
    noise, logp, flag = _twin(logits, t, gt, seeds, B, 1, V, 0)
    assert not flag.any()
    rn, rl, rf = R.posterior(logits, t, gt, seeds, B, 1, V, 0)
    assert np.array_equal(noise.view(np.uint32), rn.view(np.uint32)) and np.array_equal(logp.view(np.uint32), rl.view(np.uint32)) and not rf.any()
    losers = np.ones((B, V), bool); losers[r, gt] = False
    raised = (noise.view(np.uint32).astype(np.int64) - cand.view(np.uint32).astype(np.int64))[losers]
    counts = {k: int((raised == k).sum()) for k in range(1, 6)}
    print('entries raised above the candidate, by ulps:', counts)
    assert int((raised < 0).sum()) == 0 and int((raised > 4).sum()) == 0                  # never below the candidate; at most four steps are ever needed
    assert counts[1] >= 20 and counts[2] >= 5 and counts[1] + counts[2] + counts[3] + counts[4] == int((raised != 0).sum())
    # every raised entry is one of the planted ones, and without the raise it would not lose: its candidate's score is not below the winner's
    where = np.argwhere((noise.view(np.uint32) != cand.view(np.uint32)) & losers)
    assert bool((where[:, 1] == v[where[:, 0]]).all())
    pg = p[r, gt]
    rg = (pg / np.maximum((T * pg).astype(F), R.FLT_MIN)).astype(F)
    i, j = where[:, 0], where[:, 1]
    assert bool(((p[i, j] / cand[i, j]).astype(F) >= rg[i]).all()) and bool(((p[i, j] / noise[i, j]).astype(F) < rg[i]).all())
    prev = (noise.view(np.uint32)[i, j] - np.uint32(1)).view(F)
    assert bool(((p[i, j] / prev).astype(F) >= rg[i]).all())                                # ... and the float below the result still would not
    back = _oracle_sample(logits, noise, B, 1, V, t)
    assert np.array_equal(back, gt)
    wrong = _oracle_sample(logits, np.where(losers, cand, noise), B, 1, V, t)             # the unrepaired candidates replay another token on some rows
    assert int((wrong != gt).sum()) >= 10


def test_the_clamped_winner_still_wins():
    logits, t, gt, seeds = clamp_case()
    B, V = len(gt), V_REPAIR
    cand, T, E, p = candidates(logits, t, seeds, B, V, 2)
    r = np.arange(B)
    pg = p[r, gt]
    assert bool((pg > 0).all()) and bool(((T * pg).astype(F) < R.FLT_MIN).all())          # the clamp is reached on every row
    noise, logp, flag = _twin(logits, t, gt, seeds, B, 1, V, 2)
    assert not flag.any() and bool((noise[r, gt] == R.FLT_MIN).all())
    rn, rl, rf = R.posterior(logits, t, gt, seeds, B, 1, V, 2)
    assert np.array_equal(noise.view(np.uint32), rn.view(np.uint32)) and np.array_equal(logp.view(np.uint32), rl.view(np.uint32))
    losers = np.ones((B, V), bool); losers[r, gt] = False
    up = noise[losers] > cand[losers]
    print(f'clamped rows: {int(up.sum())} of {up.size} losers start from the closed-form bound')
    assert int(up.sum()) >= 200                                                           # (1 - exp(-0.4) = 0.33 of the three constant rows alone: 250)
    assert np.array_equal(_oracle_sample(logits, noise, B, 1, V, t), gt)


# ---- (d) the law ------------------------------------------------------------------------------------------------------------------
N_LAW, V_LAW, LIVE = 20000, 256, 8
KS_BAR = 1.95 / np.sqrt(N_LAW)              # the 0.1 % critical value of Kolmogorov's distribution (1.9495) over sqrt(n): derived, not measured


def _ks_exp1(x):
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    cdf = 1.0 - np.exp(-x)
    return float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max()))


@pytest.fixture(scope='module')
def law():
    """one fixed row, probabilities from about 1e-3 to 0.5 on 8 live codes; per seed: g drawn by the oracle's sampler from the prior fill"""
    from oracle import var_oracle as O
    util.ensure_oracle_built()
    pr = np.array([0.5, 0.25, 0.12, 0.07, 0.04, 0.015, 0.004, 0.001])
    row = np.full(V_LAW, -200.0, F)
    row[:LIVE] = np.log(pr).astype(F)
    logits = np.concatenate((np.broadcast_to(row, (N_LAW, V_LAW)), np.zeros((N_LAW, V_LAW), F))).astype(F)
    seeds = np.arange(N_LAW, dtype=np.int64) * 7919 + 12345
    prior = R.stream(seeds, 1, V_LAW, 0, 0)
    g = np.full(N_LAW, -5, np.int64)
    assert O.lib()['cfg_sample_f32'](O._p(logits), O._p(prior), O._p(g), None, N_LAW, 1, V_LAW, 0.0, 0, 0.0) == 0
    assert int(g.min()) >= 0 and int(g.max()) < LIVE
    return logits, seeds, g, pr


def test_the_posterior_noise_is_exp1_in_every_coordinate(law):
    logits, seeds, g, pr = law
    noise, _, flag = _twin(logits, np.zeros(N_LAW), g, seeds, N_LAW, 1, V_LAW, 0)
    assert not flag.any()
    freq = np.bincount(g, minlength=LIVE) / N_LAW
    assert np.abs(freq - pr / pr.sum()).max() < 4.0 * 0.5 / np.sqrt(N_LAW)             # the sampler drew g from p (4 sigma of the widest binomial)
    ds = [_ks_exp1(noise[:, v]) for v in range(LIVE)]
    print('KS D per coordinate:', ' '.join(f'{d:.5f}' for d in ds), f'bar {KS_BAR:.5f}')
    assert max(ds) < KS_BAR, (ds, KS_BAR)
    fill = R.stream(seeds, 1, V_LAW, 0, R.DRAW_FILL)
    assert np.array_equal(noise[:, LIVE:].view(np.uint32), fill[:, LIVE:].view(np.uint32))  # probability 0: the candidate is the fill, and it loses
    back = np.full(N_LAW, -5, np.int64)
    from oracle import var_oracle as O
    assert O.lib()['cfg_sample_f32'](O._p(logits), O._p(noise), O._p(back), None, N_LAW, 1, V_LAW, 0.0, 0, 0.0) == 0
    assert np.array_equal(back, g)


@pytest.mark.parametrize('fault', ['T_zero', 'drop_E'])
def test_the_bar_catches_planted_faults_in_the_restatement(law, fault):
    logits, seeds, g, _ = law
    # the restatement takes any V % 4 == 0: the 8 live codes alone give the same S (the other 248 exponentials are exactly 0) and the same
    # stream values (the counter does not depend on V), so the fault is planted on the (n, 8) problem
    small = np.ascontiguousarray(logits[:, :LIVE])
    good = R.posterior(small, np.zeros(N_LAW), g, seeds, N_LAW, 1, LIVE, 0)[0]
    twin = _twin(logits, np.zeros(N_LAW), g, seeds, N_LAW, 1, V_LAW, 0)[0]
    assert np.array_equal(good.view(np.uint32), twin[:, :LIVE].view(np.uint32))
    assert max(_ks_exp1(good[:, v]) for v in range(LIVE)) < KS_BAR
    bad = R.posterior(small, np.zeros(N_LAW), g, seeds, N_LAW, 1, LIVE, 0, **{fault: True})[0]
    ds = [_ks_exp1(bad[:, v]) for v in range(LIVE)]
    print(fault, 'KS D per coordinate:', ' '.join(f'{d:.5f}' for d in ds))
    assert max(ds) > KS_BAR, (fault, ds)


# ---- (e) stability under a raised logit -------------------------------------------------------------------------------------------
def test_raising_the_winners_logit_keeps_the_winner():
    V, B, l = 256, 3, 40
    rng = np.random.default_rng(21)
    lg = (2.0 * rng.standard_normal((2, B, l, V))).astype(F)
    lg[1] = 0.0                                                            # t = 0 on every image: the guided logit is the conditional one, the raise below moves it by exactly 4
    t = [0.0, 0.0, 0.0]
    logits = lg.reshape(2 * B * l, V)
    p = R.probabilities(R.guided(logits, B, l, t))[0]
    gt = np.array([rng.choice(V, p=(row.astype(np.float64) / row.astype(np.float64).sum())) for row in p])
    pg = p[np.arange(B * l), gt]
    keep = pg >= 2.0 ** -10
    assert keep.sum() >= 30
    seeds = [101, 102, 103]
    noise, _, flag = _twin(logits, t, gt, seeds, B, l, V, 4)
    assert not flag.any()
    up = lg.copy().reshape(2, B * l, V)
    up[0, np.arange(B * l), gt] += F(4.0)
    up = up.reshape(2 * B * l, V)
    back0 = _oracle_sample(logits, noise, B, l, V, t)
    back1 = _oracle_sample(up, noise, B, l, V, t)
    assert np.array_equal(back0, gt)
    assert np.array_equal(back1[keep], gt[keep])
    p1 = R.probabilities(R.guided(up, B, l, t))[0][np.arange(B * l), gt].astype(np.float64)
    p0 = pg.astype(np.float64)
    odds0, odds1 = p0 / (1 - p0), p1 / (1 - p1)
    assert bool((odds1[keep] >= 1.05 * odds0[keep]).all()), (odds1[keep] / odds0[keep]).min()
