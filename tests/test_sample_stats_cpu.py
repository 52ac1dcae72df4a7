"""varhip_sample_stats_host_f32, the host twin of the scored-sampling reduction (include/var_hip.h; no GPU needed), against the numpy float64
evaluation of its definitions in tests/samplestatsref.py.

Bounds: derived in the docstring of tests/samplestatsref.py from the unit roundoff of fp32, the documented accuracy of vm_exp / vm_log and the
kernel's summation order (V / 64 sequential additions per lane, six butterfly levels): lp within 2 u |lp| + dlog(V), entropy within
ent_bound(H, V); kept is exact.  At V = 8192 that is 1.1e-5 for a log-probability near -10 and 9e-5 for an entropy near 8 nats."""
import numpy as np
import pytest

from tests import samplestatsref as R
from tests import util


def host_stats(logits, masked, idx, B, l, V, t, ld_out=None, t_rows=None, expect=0):
    """-> dict of (B, ld_out) arrays prefilled with a sentinel, the call made through guard arenas"""
    from var_amd import hip
    ld = l if ld_out is None else ld_out
    out = {k: np.full((B, ld), -77, dt) for k, dt in R.FIELDS}
    fn = hip.lib().host['sample_stats_host_f32']
    tr = None if t_rows is None else np.asarray(t_rows, np.float64)
    rc = util.guarded_invoke('varhip_sample_stats_host_f32',
                             [logits, masked, idx, B, l, V, float(t), tr, out['lp_cond'], out['lp_guided'], out['lp_drawn'], out['kept'],
                              out['entropy'], ld], lambda *a: fn(*a))
    assert rc == expect, rc
    return out


@pytest.mark.parametrize('V', [256, 4096, 8192])
@pytest.mark.parametrize('keep', [1, 2, None])
def test_host_twin_against_float64(V, keep):
    """rows whose `masked` keeps 1, 2 and V entries; B = 3, l = 4: more than one image, rows beyond one workgroup's four"""
    B, l, t = 3, 4, 1.25
    logits, masked, idx = R.make_case(B, l, V, t, V if keep is None else keep, seed=V + (keep or 0))
    out = host_stats(logits, masked, idx, B, l, V, t)
    ref = R.reference(logits, masked, idx, B, l, t)
    R.check_against_reference(out, ref, V, f'V={V} keep={keep}: ')
    assert (ref['kept'] == (V if keep is None else keep)).all()
    if keep == 1:
        assert (out['lp_drawn'] == 0.0).all() and (out['kept'] == 1).all()
    if keep is None:                                                    # nothing filtered: the drawn distribution IS the guided one, the same code on the same floats
        assert np.array_equal(out['lp_drawn'].view(np.uint32), out['lp_guided'].view(np.uint32))


@pytest.mark.parametrize('V', [256, 4096, 8192])
def test_t_zero_tie_and_peaked_rows(V):
    """t = 0: z = 1 * cond - 0 * uncond = cond, so lp_guided is lp_cond bit for bit; a tie at the maximum; a row so peaked that most exponentials
    are exactly 0 (the 0 * log 0 = 0 branch of the entropy)"""
    B, l = 1, 4
    logits, _, idx = R.make_case(B, l, V, 0.0, V, seed=5)
    logits[0, 7] = logits[0, 100] = logits[0].max() + 1.0               # an exact tie at the maximum, token on one of the two
    idx[0] = 100
    logits[1] = -200.0; logits[1, 9] = 3.0; logits[1, 11] = 2.0         # every other code: exp(-203) == 0 in vm_exp
    idx[1] = 11
    masked = R.guided_rows(logits, B, l, 0.0)
    out = host_stats(logits, masked, idx, B, l, V, 0.0)
    assert np.array_equal(out['lp_guided'].view(np.uint32), out['lp_cond'].view(np.uint32))
    R.check_against_reference(out, R.reference(logits, masked, idx, B, l, 0.0), V, f'V={V}: ')


def test_refused_image_and_ld_out():
    """an idx of -1 (and one of V): never dereferenced, the log-probabilities are NaN, kept and entropy are the row's own; ld_out > l: only the
    (B, l) corner is written"""
    B, l, V, t, ld = 3, 4, 256, 0.75, 7
    logits, masked, idx = R.make_case(B, l, V, t, 5, seed=1)
    idx[4:8] = -1
    idx[9] = V
    out = host_stats(logits, masked, idx, B, l, V, t, ld_out=ld)
    ref = R.reference(logits, masked, idx, B, l, t)
    assert np.isnan(ref['lp_cond'][1]).all() and np.isnan(ref['lp_cond'][2, 1]) and np.isfinite(ref['entropy']).all()
    R.check_against_reference({k: v[:, :l] for k, v in out.items()}, ref, V)
    for k, v in out.items():
        assert (v[:, l:] == -77).all(), f'{k}: written beyond the row of l outputs'


def test_device_array_form_equals_the_scalar_form_per_image():
    B, l, V = 3, 4, 4096
    ts = [0.0, 1.5, 0.3333333333333333]
    logits, _, idx = R.make_case(B, l, V, 0.0, V, seed=2)
    masked = R.filtered(R.guided_rows(logits, B, l, ts), 40)
    idx = np.array([np.flatnonzero(r != -np.inf)[3] for r in masked], np.int64)
    out = host_stats(logits, masked, idx, B, l, V, 99.0, t_rows=ts)      # (the scalar is not read)
    R.check_against_reference(out, R.reference(logits, masked, idx, B, l, ts), V)
    lg = logits.reshape(2, B, l, V)
    for b in range(B):
        one = host_stats(np.ascontiguousarray(lg[:, b]).reshape(2 * l, V), masked[b * l:(b + 1) * l].copy(), idx[b * l:(b + 1) * l].copy(), 1, l, V, ts[b])
        for k, _ in R.FIELDS:
            assert np.array_equal(one[k][0].view(np.uint32), out[k][b].view(np.uint32)), (b, k)


@pytest.mark.parametrize('V', [256, 8192])
def test_nan_rows(V):
    """a NaN in a row: the entropy of a guided row holding one is NaN and `kept` counts it (it is not -inf); the log-probabilities are what
    varhip_token_loglik_f32 gives: NaN where the token is the NaN; elsewhere its register path (V <= 4096) drops the NaN from max and sum —
    the value of the row without that entry — and its memory path (V > 4096) returns NaN"""
    B, l, t = 1, 4, 0.5
    logits, _, idx = R.make_case(B, l, V, t, V, seed=3)
    clean = logits.copy()
    logits[0, 5] = np.nan; idx[0] = 5                                   # the token itself
    logits[1, 6] = np.nan; idx[1] = 17                                  # another entry of the conditional row
    masked = R.guided_rows(logits, B, l, t)
    out = host_stats(logits, masked, idx, B, l, V, t)
    assert np.isnan(out['lp_cond'][0, 0]) and np.isnan(out['lp_guided'][0, 0]) and np.isnan(out['lp_drawn'][0, 0])
    assert np.isnan(out['entropy'][0, :2]).all() and np.isfinite(out['entropy'][0, 2:]).all()
    assert (out['kept'] == V).all()
    if V <= 4096:
        clean[1, 6] = -np.inf
        cm = R.guided_rows(clean, B, l, t)
        cm[1, 6] = -np.inf                                              # (-inf * ca - cb * uncond stays -inf for finite uncond; pinned here for clarity)
        ref = R.reference(clean, cm, idx, B, l, t)
        for k in ('lp_cond', 'lp_guided', 'lp_drawn'):
            assert abs(float(out[k][0, 1]) - ref[k][0, 1]) <= R.lp_bound(ref[k][0, 1], V), k
    else:
        assert np.isnan(out['lp_cond'][0, 1]) and np.isnan(out['lp_guided'][0, 1]) and np.isnan(out['lp_drawn'][0, 1])
    R.check_against_reference({k: v[:, 2:] for k, v in out.items()},
                              {k: v[:, 2:] for k, v in R.reference(logits, masked, idx, B, l, t).items()}, V)


def test_einval():
    from var_amd import abi
    B, l, V = 1, 2, 256
    logits, masked, idx = R.make_case(B, l, V, 1.0, V, seed=4)
    E = abi.EINVAL
    host_stats(logits, masked, idx, B, l, 255, 1.0, expect=E)           # V % 256
    host_stats(logits, masked, idx, B, l, 0, 1.0, expect=E)
    host_stats(logits, masked, idx, B, l, 8192 + 256, 1.0, expect=E)    # V > 8192
    host_stats(logits, masked, idx, 0, l, V, 1.0, expect=E)
    host_stats(logits, masked, idx, B, 0, V, 1.0, expect=E)
    out = host_stats(logits, masked, idx, B, l, V, 1.0, ld_out=3)       # fine
    assert (out['kept'][:, :l] == V).all()
    from var_amd import hip
    fn = hip.lib().host['sample_stats_host_f32']
    o = {k: np.zeros((B, l), dt) for k, dt in R.FIELDS}
    p = lambda a: a.ctypes.data
    good = [p(logits), p(masked), p(idx), B, l, V, 1.0, None, p(o['lp_cond']), p(o['lp_guided']), p(o['lp_drawn']), p(o['kept']), p(o['entropy']), l]
    assert fn(*good) == 0
    for pos in (0, 1, 2, 8, 9, 10, 11, 12):                            # a NULL operand
        bad = list(good); bad[pos] = None
        assert fn(*bad) == E, pos
    bad = list(good); bad[13] = l - 1                                   # ld_out < l
    assert fn(*bad) == E
