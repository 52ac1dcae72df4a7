"""What the sample-stats tests share: the definitions of varhip_sample_stats_f32 (include/var_hip.h) evaluated independently in numpy float64 on
the fp32 rows, the error bounds of the fp32 kernel against that evaluation, and the builders of the kernel-level cases.

The bounds (u = 2^-24, the unit roundoff of fp32; V the row length; ln V <= 9.02).  None of them is fitted to what the code returns.

  s, the row's sum of exponentials.  Every term e_v = vm_exp(z_v - m) carries the rounding of its argument, |d_v| u absolute in the exponent
  (d_v = z_v - m <= 0), and the error of vm_exp itself, documented as about 1 ulp (include/var_math.h); we allow 4 ulp = 8 u.  Weighted by
  p_v = e_v / s the argument roundings add up to u * E_p|d|, and E_p|d| = H - ln s <= ln V (H <= ln V is the entropy, s >= 1 because the
  maximum contributes e^0).  The terms are positive and are added as V / 64 sequential additions per lane and six butterfly levels, each one
  rounding: (V / 64 + 6) u relative.  Together
      ds(V) = (8 + ln V + V / 64 + 6) u                         relative error of s.
  ln s: a relative error ds of s is an absolute ds of ln s; vm_log adds about 1 ulp of |ln s| <= ln V, we allow 2 ulp = 4 u ln V:
      dlog(V) = ds(V) + 4 u ln V.
  lp = (z_g - m) - ln s: the two subtractions round by u |z_g - m| and u |lp|, and |z_g - m| <= |lp| (both parts of lp are <= 0):
      lp_bound(lp, V) = 2 u |lp| + dlog(V).
  entropy = -(sum_v e_v lp_v) / s, summed in float64 (its own rounding, V * 2^-53, is dropped): e_v is off by (8 u + |d_v| u) relative, lp_v by
  2 u |lp_v| + dlog absolute, s by ds relative, and the result is rounded once more (u H).  With sum_v p_v |lp_v| = H, sum_v p_v = 1 and
  sum_v p_v |lp_v| |d_v| <= sum_v p_v d_v^2 + ln V * E_p|d| <= (2 ln^2 V + 2) + ln^2 V   [codes with |d| <= 2 ln V: d^2 <= 2 ln V |d|;
  the others: p_v <= e^{d_v}, and V * x^2 e^{-x} at x = 2 ln V is 4 ln^2 V / V <= 2 for V >= 256]:
      ent_bound(H, V) = H (8 u + 2 u + ds(V) + u) + u (3 ln^2 V + 2) + dlog(V).
"""
import numpy as np

U = 2.0 ** -24


def ds(V):
    return (8 + np.log(V) + V / 64 + 6) * U


def dlog(V):
    return ds(V) + 4 * U * np.log(V)


def lp_bound(lp, V):
    return 2 * U * np.abs(lp) + dlog(V)


def ent_bound(H, V):
    return np.abs(H) * (11 * U + ds(V)) + U * (3 * np.log(V) ** 2 + 2) + dlog(V)


def guided_rows(logits, B, l, t):
    """z = (float)(1 + t) * cond - (float)t * uncond with each product and the difference rounded to fp32; logits (2B*l, V) fp32, t a scalar
    or B values (float64) -> (B*l, V) fp32"""
    logits = np.asarray(logits, np.float32).reshape(2 * B * l, -1)
    t = np.broadcast_to(np.asarray(t, np.float64), (B,))
    ca = (1.0 + t).astype(np.float32).repeat(l)[:, None]
    cb = t.astype(np.float32).repeat(l)[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        a = (ca * logits[:B * l]).astype(np.float32)
        b = (cb * logits[B * l:]).astype(np.float32)
        return (a - b).astype(np.float32)


def _logp_rows(z, idx):
    """float64 log_softmax(z)[idx] per row; -inf entries add 0; an idx outside [0, V) gives NaN"""
    z64 = np.asarray(z, np.float64)
    out = np.full(z64.shape[0], np.nan)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i, (row, g) in enumerate(zip(z64, idx)):
            if 0 <= g < row.shape[0]:
                m = row.max()
                out[i] = (row[g] - m) - np.log(np.exp(row - m).sum())
    return out


def _entropy_rows(z):
    z64 = np.asarray(z, np.float64)
    out = np.empty(z64.shape[0])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i, row in enumerate(z64):
            if np.isnan(row).any():
                out[i] = np.nan
                continue
            d = row - row.max()
            e = np.exp(d)
            s = e.sum()
            nz = e > 0
            out[i] = -(e[nz] / s * (d[nz] - np.log(s))).sum()
    return out


def reference(logits, masked, idx, B, l, t):
    """-> dict(lp_cond, lp_guided, lp_drawn, entropy float64 (B, l); kept int64 (B, l)) from a float64 evaluation of the fp32 rows"""
    logits = np.asarray(logits, np.float32).reshape(2 * B * l, -1)
    masked = np.asarray(masked, np.float32).reshape(B * l, -1)
    idx = np.asarray(idx, np.int64).reshape(-1)
    z = guided_rows(logits, B, l, t)
    return dict(lp_cond=_logp_rows(logits[:B * l], idx).reshape(B, l), lp_guided=_logp_rows(z, idx).reshape(B, l),
                lp_drawn=_logp_rows(masked, idx).reshape(B, l), entropy=_entropy_rows(z).reshape(B, l),
                kept=(masked != -np.inf).sum(-1).astype(np.int64).reshape(B, l))


def filtered(z, keep):
    """a masked_out row set as the sampler leaves it: the `keep` largest entries of every row of z (ties: every entry equal to the keep-th), the
    rest -inf"""
    z = np.asarray(z, np.float32)
    if keep >= z.shape[-1]:
        return z.copy()
    kth = np.sort(z, -1)[:, -keep][:, None]
    return np.where(z >= kth, z, np.float32(-np.inf)).astype(np.float32)


def make_case(B, l, V, t, keep, seed, scale=3.0):
    """random logits (2B*l, V), the guided rows filtered to `keep` entries, a token among the kept ones per row"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((2 * B * l, V)) * scale).astype(np.float32)
    masked = filtered(guided_rows(logits, B, l, t), keep)
    idx = np.array([rng.choice(np.flatnonzero(row != -np.inf)) for row in masked], np.int64)
    return logits, masked, idx


def check_against_reference(got, ref, V, what=''):
    """got: dict of (B, l) arrays as the kernel wrote them; every value within its bound of the float64 reference, kept exact; NaN where NaN"""
    for k in ('lp_cond', 'lp_guided', 'lp_drawn'):
        g, r = np.asarray(got[k], np.float64), ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)), f'{what}{k}: NaN pattern differs'
        ok = ~np.isnan(r)
        with np.errstate(invalid='ignore'):
            same = g[ok] == r[ok]                                       # (-inf on both sides)
            err = np.where(same, 0.0, np.abs(g[ok] - r[ok]))
        bound = lp_bound(np.where(np.isfinite(r[ok]), r[ok], 0.0), V)
        print(f'{what}{k}: max |diff| {err.max() if err.size else 0:.3e}, smallest bound {bound.min() if bound.size else 0:.3e}')
        assert (err <= bound).all(), f'{what}{k}: {err.max():.3e} beyond the bound {bound[err.argmax()]:.3e}'
    g, r = np.asarray(got['entropy'], np.float64), ref['entropy']
    assert np.array_equal(np.isnan(g), np.isnan(r)), f'{what}entropy: NaN pattern differs'
    ok = ~np.isnan(r)
    err, bound = np.abs(g[ok] - r[ok]), ent_bound(r[ok], V)
    print(f'{what}entropy: max |diff| {err.max() if err.size else 0:.3e}, smallest bound {bound.min() if bound.size else 0:.3e}')
    assert (err <= bound).all(), f'{what}entropy: {err.max():.3e} beyond the bound'
    assert np.array_equal(np.asarray(got['kept'], np.int64), ref['kept']), f'{what}kept differs'


FIELDS = (('lp_cond', np.float32), ('lp_guided', np.float32), ('lp_drawn', np.float32), ('kept', np.int32), ('entropy', np.float32))
