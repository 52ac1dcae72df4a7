"""Stages 2, 3 and 5 of varhip_ctl_sample_rows_f32 (include/var_hip.h) restated from the header's text in numpy float32, and the builders of the
cases its tests share.  No line here is taken from sampler.hip; the exponential is tests/codecref.py's restatement of include/var_math.h."""
import numpy as np

from tests import codecref

F = np.float32


def bias_temper(x, bias=None, tau=1.0):
    """stages 2 and 3 on fp32 rows x (..., V): x + bias (one fp32 add; skipped for bias None), then x / tau (one fp32 division, skipped for
    tau == 1)"""
    x = np.asarray(x, F)
    with np.errstate(all='ignore'):
        if bias is not None:
            x = (x + np.asarray(bias, F)).astype(F)
        if F(tau) != F(1.0):
            x = (x / F(tau)).astype(F)
    return x


def min_p_cut(x, min_p):
    """stage 5 on fp32 rows x (..., V) (after top-k: -inf entries stay -inf): m = the row's maximum, e = vm_exp(x - m), x = -inf where
    e < min_p, compared in fp32; min_p <= 0: the stage does not run"""
    x = np.asarray(x, F)
    if not F(min_p) > F(0.0):
        return x.copy()
    with np.errstate(all='ignore'):
        m = x.max(axis=-1, keepdims=True)
        e = codecref.vm_exp((x - m).astype(F))
    return np.where(e < F(min_p), F(-np.inf), x).astype(F)


def guided(cond, uncond, t):
    """stage 1 per image: cond, uncond (B, l, V) fp32, t (B,) float64 -> (B, l, V) fp32, three roundings"""
    return np.stack([codecref.guided(c, u, tb) for c, u, tb in zip(cond, uncond, t)])


def rows_with_known_survivors(n, V, js, seed):
    """n rows of 3 * randn and, for row i, the min_p that leaves exactly js[i % len(js)] codes: the geometric midpoint between the j-th and
    the (j + 1)-th largest probability ratio p_v / p_max of the row.  Asserts that the two neighbours' log-ratios differ by more than 1e-4,
    so no case sits near the threshold (the float32 exponential is good to ~1e-7 relative) and none is skipped
    -> (rows (n, V) fp32, min_p (n,) float64, survivors (n,) int)"""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((n, V))).astype(F)
    mp, want = np.empty(n), np.empty(n, np.int64)
    for i in range(n):
        j = js[i % len(js)]
        d = np.sort(x[i].astype(np.float64) - float(x[i].max()))[::-1]              # log-ratios, descending: d[0] = 0
        assert d[j - 1] - d[j] > 1e-4, (i, j, d[j - 1], d[j])
        mp[i], want[i] = np.exp(0.5 * (d[j - 1] + d[j])), j
    return x, mp, want
