"""A float64 dense restatement of varhip_attn_rowstats_f32 / varhip_attn_flow_f32 (include/var_hip.h) and the bars their outputs must meet, plus
the cases the CPU and GPU tests of VAR.attention_maps / VAR.attention_rollout share.

The restatement knows nothing of fma chains, tiles or vm_exp_le0: scores in float64, an explicit (Lq, Lq) block-causal softmax P per (row, head),
and R @ P (per head), or (1 - alpha) R + alpha R @ mean_h P.

THE BARS (derived here, not fitted).  All are L1 distances over a row of Lq keys, so they bound every entry and every row sum too.
  (a) one row of p.  attnprofref's (a)-(c) hold for the numerators e_j = vm_exp_le0(s_j - m): every e_j is its real value times a factor in
      [1 / G, G], G^2 = F of attnprofref (F is stated there for a RATIO of two such sums).  Here the denominator is an fp32 sum of n <= Lq
      positive terms in two partial sums (relative error <= gamma_n), then 1 / sum (u), then e * rinv (u): p_tj = pi_tj * f with f in [1 / Fq, Fq],
          Fq = F * (1 + (n + 3) u) / (1 - (n + 3) u),      u = 2^-24,
      so sum_j |p_tj - pi_tj| <= (Fq - 1) sum_j pi_tj = Fq - 1 =: eps_t  (per row, head, query).  The clamp of the exponential at e^-87 adds at most
      Lq * 2^-125, which is added.
  (b) one per-head product.  out_sj = sum_t r_st p_tj is one fma chain of n_t <= 32 ceil(Lq / 32) terms: |fl - exact| <= gamma_{n_t} sum_t |r_st| p_tj
      (Higham §3.1).  Summed over j, with sum_j p_tj <= 1 + eps_t:
          E1[s] = sum_t |r_st| eps_t  +  gamma_{n_t} ||r_s||_1 (1 + max eps).
  (c) one rollout layer.  The heads are added in fp32 (H - 1 adds), scaled by 1 / H (two roundings), and combined with (1 - alpha) r (three
      roundings): a relative error of at most gamma_{H + 6} on values whose L1 norm is at most ||r_s||_1 (1 + max eps):
          E0[s] = alpha * mean_h E1_h[s]  +  gamma_{H + 6} ||r_s||_1 (1 + max eps).
  (d) a rollout over D' layers.  Every (1 - alpha) I + alpha Pbar is row-stochastic and non-negative, so r -> r M never increases ||.||_1: the
      error an earlier layer left is carried through the later ones with a factor <= 1, and ||r||_1 stays 1 for a one-hot start (the computed r: at
      most 1 + the error so far).  A D'-layer rollout therefore errs by at most  D' * E0(||r||_1 = 1) * (1 + D' * E0),  with eps = max over
      all layers, heads and queries.
  (e) against varhip_attn_cached_f32.  That kernel's probabilities carry (a) as well (same numerators, an fp32 row sum), and its P V product is an
      fma chain of Lq terms: |sum_j row_sj v_jc - out_tc| <= (2 eps_t + gamma_{2 Lq + 4}) max_j |v_jc|.

TOLERANCE OF THE HIP ROUTE AGAINST THE TORCH TWINS (tests/test_attention_rollout_gpu.py), attnprofref's procedure: measured once, on a CPU, from
PyTorch code alone (no library call): the largest deviation of an entry of rows / flow between the twins on the tiny fixture with float32 modules
and with float64 modules (tests/test_attn_flow_cpu.py::test_torch_twins_f32_against_f64 prints them).  The GPU test allows 8x: the HIP GEMMs sum
in another order than PyTorch's."""
import numpy as np

U = 2.0 ** -24
EXP_EPS = 2.0 ** -22

# measured by tests/test_attn_flow_cpu.py::test_torch_twins_f32_against_f64 (which prints them) on t_pn12345's model (depth 2, patch_nums (1, 2, 3, 4,
# 5), with and without attn_l2_norm, 3 images, 5 targets): the largest |f32 - f64| of an entry of rows: 1.192e-07, of flow: 2.980e-08
TORCH_F32_VS_F64_ROWS = 2.0 ** -23
TORCH_F32_VS_F64_FLOW = 2.0 ** -25
HIP_VS_TORCH_FACTOR = 8

ENDS = ((1, 5, 14), (1, 5, 14, 30, 55, 91), (1, 32, 33, 64, 97))


def gamma(n):
    return n * U / (1 - n * U)


def limits(ends, Lq):
    """(Lq,) one past the last key each query sees"""
    ends = np.asarray(ends)
    return ends[np.searchsorted(ends, np.arange(Lq), side='right')]


def make_case(ends, B=2, H=3, seed=0, pad=7, qnorm=(0.5, 100.0)):
    """q [B][Lq][H*64] with norms spread over qnorm (the model's: temperature <= 100 times a unit vector), kcache [B][H][Lq + pad][64] with unit keys
    and a NaN-filled tail"""
    Lq = int(ends[-1])
    rng = np.random.default_rng(seed * 7919 + Lq * 131 + len(ends))
    k = rng.standard_normal((B, H, Lq, 64))
    k /= np.linalg.norm(k, axis=-1, keepdims=True)
    q = rng.standard_normal((B, Lq, H, 64))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= rng.uniform(qnorm[0], qnorm[1], size=(B, Lq, H, 1))
    kc = np.full((B, H, Lq + pad, 64), np.nan, dtype=np.float32)
    kc[:, :, :Lq] = k.astype(np.float32)
    return dict(q=np.ascontiguousarray(q.reshape(B, Lq, H * 64).astype(np.float32)), kc=kc, ends=np.asarray(ends, dtype=np.int32), B=B, H=H, Lq=Lq,
                Lmax=Lq + pad)


def make_r(case, T, seed=0, onehot=None):
    """r [B][T][Lq]: one-hot rows at `onehot` (T token indices), or non-negative rows of L1 norm 1 with a third of the entries exactly 0"""
    B, Lq = case['B'], case['Lq']
    r = np.zeros((B, T, Lq), np.float32)
    if onehot is not None:
        r[:, np.arange(T), np.asarray(onehot)] = 1.0
        return r
    rng = np.random.default_rng(seed + 17 * T)
    x = rng.uniform(0, 1, (B, T, Lq)) * (rng.uniform(0, 1, (B, T, Lq)) > 1 / 3)
    x[..., 0] += 1e-3
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def dense(case):
    """-> (P (B, H, Lq, Lq) float64 block-causal softmax, eps (B, H, Lq) the L1 bar (a) of every row)"""
    q, kc, B, H, Lq = case['q'], case['kc'], case['B'], case['H'], case['Lq']
    qq = q.astype(np.float64).reshape(B, Lq, H, 64).transpose(0, 2, 1, 3)
    kk = kc[:, :, :Lq].astype(np.float64)
    s = np.einsum('bhtc,bhjc->bhtj', qq, kk)
    sabs = np.einsum('bhtc,bhjc->bhtj', np.abs(qq), np.abs(kk))
    lim = limits(case['ends'], Lq)
    vis = np.arange(Lq)[None, :] < lim[:, None]
    s = np.where(vis, s, -np.inf)
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    D = gamma(64) * np.where(vis, sabs, 0).max(-1) + 87 * U
    F = np.exp(2 * D) * (1 + EXP_EPS) / (1 - EXP_EPS)
    n = lim[None, None, :] + 3
    eps = F * (1 + n * U) / (1 - n * U) - 1 + Lq * 2.0 ** -125
    return P, eps


def reference(case, r, per_head, alpha=0.0):
    """-> (out float64, bar float64 of out's shape without the key axis: the L1 bar of every output row, (b) or (c))"""
    P, eps = dense(case)
    H, Lq = case['H'], case['Lq']
    r64 = r.astype(np.float64)
    nt = 32 * ((Lq + 31) // 32)
    norm = np.abs(r64).sum(-1)                                                           # (B, T)
    E1 = np.einsum('bst,bht->bhs', np.abs(r64), eps) + gamma(nt) * norm[:, None, :] * (1 + eps.max())
    ph = np.einsum('bst,bhtj->bhsj', r64, P)
    if per_head:
        return ph, E1
    return (1 - alpha) * r64 + alpha * ph.mean(1), alpha * E1.mean(1) + gamma(H + 6) * norm * (1 + eps.max())


def rollout_bar(layers, one_layer_bar):
    """(d): the bar of a `layers`-layer rollout from a one-hot start, from the largest one-layer bar E0 at ||r||_1 = 1"""
    return layers * one_layer_bar * (1 + layers * one_layer_bar)


def run(case, r, per_head, alpha=0.0, device=False, rowstats=None, out_fill=np.nan):
    """the twins (device False) or the kernels through guarded_call (True) -> dict(m, rinv, nan (B, H), out).  rowstats: (m, rinv) to use instead
    of the first call's"""
    from var_amd import hip
    B, H, Lq, T = case['B'], case['H'], case['Lq'], r.shape[1]
    m, rinv = (np.full((B, H, Lq), out_fill, np.float32) for _ in range(2))
    nan = np.zeros((B, H), np.int32)
    out = np.full((B, H, T, Lq) if per_head else (B, T, Lq), out_fill, np.float32)
    ends = case['ends']
    if not device:
        hip.call_host('attn_rowstats_host_f32', case['q'], case['kc'], B, Lq, H, case['Lmax'], ends, len(ends), m, rinv, nan)
        ms, ri = (m, rinv) if rowstats is None else rowstats
        hip.call_host('attn_flow_host_f32', case['q'], case['kc'], ms, ri, r, out, B, Lq, H, case['Lmax'], ends, len(ends), T, int(per_head), float(alpha))
        return dict(m=m, rinv=rinv, nan=nan, out=out)
    import torch
    from tests import util
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(q=case['q'], kc=case['kc'], m=m, rinv=rinv, nan=nan, out=out, r=r).items()}
    et = torch.from_numpy(np.asarray(ends, np.int32).copy())
    util.guarded_call('attn_rowstats_f32', d['q'], d['kc'], B, Lq, H, case['Lmax'], et, len(ends), d['m'], d['rinv'], d['nan'])
    ms, ri = (d['m'], d['rinv']) if rowstats is None else (torch.from_numpy(rowstats[0]).cuda(), torch.from_numpy(rowstats[1]).cuda())
    util.guarded_call('attn_flow_f32', d['q'], d['kc'], ms, ri, d['r'], d['out'], B, Lq, H, case['Lmax'], et, len(ends), T, int(per_head), float(alpha))
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in ('m', 'rinv', 'nan', 'out')}


def same_bits(a, b):
    """the same bits, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
