"""What the class-information tests share: the definitions of varhip_class_mix_f32 (include/var_hip.h) evaluated independently in numpy float64
on the fp32 rows, the error bounds of the fp32 kernel (and of its host twin, which gives the kernel's bits) against that evaluation, and the
builders of the kernel-level cases.

The bounds (u = 2^-24, the unit roundoff of fp32; ds, dlog and ent_bound are those of tests/samplestatsref.py, derived there).  None of them
is fitted to what the code returns.

  entropy[k] = H_k: the rule of varhip_sample_stats_f32 on the same row, so its bound: ent_bound(H_k, V).
  p_v = e_v / s.  e_v carries the rounding of its argument (|d_v| u in the exponent, d_v = z_v - m) and vm_exp's own error (8 u allowed, as
    there), s is off by ds(V) relative, the division rounds once (u):   rel_p(v) = (9 + |d_v|) u + ds(V).
  mix_q[v] = sum_k rint(p_v pi_k 2^48): the product is exact in float64, so against the real number M_v = 2^48 sum_k pi_k p_kv
      mixq_bound[v] = 2^48 sum_k pi_k p_kv rel_p(k, v) + K / 2 + 1       (one rint per class: 1/2 each; 1 for results of the division that are
                                                                          subnormal: 2^-149 * 2^48 per class, far below 1 in sum)
  hcond_q = sum_k rint(pi_k H_k 2^40), h_cond = (float)(hcond_q 2^-40):
      hcond_bound = sum_k pi_k ent_bound(H_k, V) + K 2^-41 + u |h_cond|
  q_v = (float)(mix_q[v] 2^-48) is off M_v 2^-48 by dq_v = mixq_bound[v] 2^-48 + u q_v.  With f(q) = -sum q ln q, df/dq_v = -(ln q_v + 1):
      hmix_bound = (1 + 1e-3) sum_v dq_v (|ln q_v| + 1)      first order; the factor covers the second-order term: dq_v / q_v stays below 1e-3
                                                             wherever q_v >= 2^-30 (dq_v <= 1e-5 q_v + (K / 2 + 1) 2^-48), and smaller q_v add
                                                             at most dq_v (|ln dq_v| + 1) each, which the term with |ln q_v| >= 20 dominates
                   + 4 u sum_v q_v |ln q_v|                  vm_log, 2 ulp allowed as in dlog
                   + u |h_mix|                               the final rounding (the float64 sum's own rounding, V 2^-53, is dropped)
  mi = (float)((0 - A) - hcond_q 2^-40):   mi_bound = hmix_bound + hcond_bound (each without its final rounding is smaller) + u |mi|
  logp_mix = vm_log(q_g):   logp_bound = (1 + 1e-3) dq_g / q_g + 4 u max(|ln q_g|, 1)
"""
import numpy as np

from tests.samplestatsref import U, ds, ent_bound

MIX_ONE = float(2 ** 48)
H_ONE = float(2 ** 40)
FIELDS = ('h_mix', 'h_cond', 'mi', 'logp_mix')


def synth_logits(rows, V, seed, scale=3.0):
    """tests/test_distance_profile_gpu.synth_logits (restated here: that module needs a GPU to import): NaN-free rows with |z| <= 5.6"""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((rows, V)) * scale, -5.6, 5.6).astype(np.float32)


def guided(logits, images, classes, l, V, u, ca, cb):
    """the fp32 z of the pass layout: a = ca * cond; b = cb * uncond; a - b (each rounded) -> (images, classes, l, V) fp32"""
    lg = np.asarray(logits, np.float32).reshape(-1, V)
    cond = lg[:images * classes * l].reshape(images, classes, l, V)
    if not u:
        return cond.copy()
    unc = lg[images * classes * l:images * (classes + 1) * l].reshape(images, 1, l, V)
    with np.errstate(invalid='ignore', over='ignore'):
        a = (np.float32(ca) * cond).astype(np.float32)
        b = (np.float32(cb) * unc).astype(np.float32)
        return (a - b).astype(np.float32)


def make_prior(images, classes, seed=None):
    """(images, classes) fp32: uniform float32(1 / K), or random rows that sum to 1 within 1e-6 after the rounding to fp32"""
    if seed is None:
        return np.full((images, classes), np.float32(1.0 / classes), np.float32)
    p = np.random.default_rng(seed).random((images, classes)) + 0.05
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    assert (np.abs(p.astype(np.float64).sum(-1) - 1) <= 1e-6).all()
    return p


def reference(z, prior, gt):
    """z: (images, classes, l, V) fp32 guided logits, prior: (images, classes) fp32, gt: (images, l) int64 -> dict of float64 arrays:
    entropy (images, classes, l), mix (images, l, V) = sum_k pi_k p_k, h_mix, h_cond, mi, logp_mix (images, l), and the bounds of the module
    docstring: entropy_bound, mixq_bound (in units of 2^-48), hmix_bound, hcond_bound, mi_bound, logp_bound.  A token with a NaN in any class
    row: NaN in the four (images, l) values; a row with a NaN: NaN entropy; a gt outside [0, V): NaN logp_mix."""
    z64 = np.asarray(z, np.float64)
    images, K, l, V = z64.shape
    pi = np.asarray(prior, np.float64).reshape(images, K, 1, 1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        nanrow = np.isnan(z64).any(-1)                                      # (images, K, l)
        zc = np.where(np.isnan(z64), -np.inf, z64)
        d = zc - zc.max(-1, keepdims=True)
        e = np.exp(d)
        s = e.sum(-1, keepdims=True)
        p = e / s
        lp = np.where(e > 0, d - np.log(s), 0.0)
        H = -(p * lp).sum(-1)
        H[nanrow] = np.nan
        dabs = np.where(e > 0, -d, 0.0)
        rel_p = (9 + dabs) * U + ds(V)
        mix = (pi * p).sum(1)                                               # (images, l, V)
        mixq_bound = MIX_ONE * (pi * p * rel_p).sum(1) + K / 2 + 1
        hb = ent_bound(np.where(nanrow, 0.0, H), V)
        h_cond = (pi[..., 0] * H).sum(1)
        hcond_bound = (pi[..., 0] * hb).sum(1) + K * 2.0 ** -41 + U * np.abs(h_cond)
        pos = mix > 0
        lnq = np.where(pos, np.log(np.where(pos, mix, 1.0)), 0.0)
        h_mix = -(mix * lnq).sum(-1)
        dq = mixq_bound / MIX_ONE + U * mix
        hmix_bound = (1 + 1e-3) * (np.where(pos, dq * (np.abs(lnq) + 1), 0.0)).sum(-1) + 4 * U * (mix * np.abs(lnq)).sum(-1) + U * np.abs(h_mix)
        mi = h_mix - h_cond
        mi_bound = hmix_bound + hcond_bound + U * np.abs(mi)
        g = np.asarray(gt, np.int64)
        valid = (g >= 0) & (g < V)
        gi = np.where(valid, g, 0)[..., None]
        qg = np.take_along_axis(mix, gi, -1)[..., 0]
        dqg = np.take_along_axis(dq, gi, -1)[..., 0]
        logp = np.log(qg)
        logp_bound = (1 + 1e-3) * dqg / qg + 4 * U * np.maximum(np.abs(logp), 1.0)
        bad = nanrow.any(1)                                                 # (images, l)
        for a in (h_mix, h_cond, mi, logp):
            a[bad] = np.nan
        logp[~valid] = np.nan
    return dict(entropy=H, entropy_bound=hb, mix=mix, mixq_bound=mixq_bound, h_mix=h_mix, hmix_bound=hmix_bound, h_cond=h_cond,
                hcond_bound=hcond_bound, mi=mi, mi_bound=mi_bound, logp_mix=logp, logp_bound=logp_bound, bad=bad)


BOUND_OF = dict(h_mix='hmix_bound', h_cond='hcond_bound', mi='mi_bound', logp_mix='logp_bound', entropy='entropy_bound')


def check_against_reference(got, ref, what='', factor=1.0, mix_q=None):
    """got: dict(entropy (images, classes, l), h_mix, h_cond, mi, logp_mix (images, l)) as the code wrote them; each within `factor` times its
    bound of the float64 reference, NaN exactly where the reference has NaN.  mix_q (images, l, V) int64, if given, is held to mixq_bound on
    the tokens without a NaN row.  Prints every figure before it asserts."""
    for k in ('entropy',) + FIELDS:
        g, r, b = np.asarray(got[k], np.float64), ref[k], ref[BOUND_OF[k]] * factor
        assert g.shape == r.shape, f'{what}{k}: shape {g.shape} != {r.shape}'
        assert np.array_equal(np.isnan(g), np.isnan(r)), f'{what}{k}: NaN pattern differs'
        ok = ~np.isnan(r)
        with np.errstate(invalid='ignore'):
            err = np.where(g[ok] == r[ok], 0.0, np.abs(g[ok] - r[ok]))
        print(f'{what}{k}: max |diff| {err.max() if err.size else 0:.3e}, smallest bound {b[ok].min() if err.size else 0:.3e}, '
              f'largest diff / bound {(err / b[ok]).max() if err.size else 0:.3f}')
        assert (err <= b[ok]).all(), f'{what}{k}: {err.max():.3e} beyond the bound {b[ok][err.argmax()]:.3e}'
    if mix_q is not None:
        ok = ~ref['bad']
        err = np.abs(np.asarray(mix_q, np.float64)[ok] - ref['mix'][ok] * MIX_ONE)
        b = ref['mixq_bound'][ok] * factor
        print(f'{what}mix_q: largest diff / bound {(err / b).max() if err.size else 0:.3f}')
        assert (err <= b).all(), f'{what}mix_q: {err.max():.3e} (2^-48 units) beyond its bound'
