"""A float64 restatement of varhip_attn_profile_f32 (include/var_hip.h) and the bound its fixed-point shares must meet, plus the cases the CPU
and GPU tests of VAR.attention_profile share.

The restatement knows nothing of fma chains, vm_exp_le0 or fixed point: scores in float64, the exact softmax, the bins by their definition, the
shares as real numbers in [0, 1].

THE BOUND (derived here, not fitted): share_q / 2^21 against the real share of a bin, per query.
  (a) score.  The kernel's s_j is one fp32 fma chain of 64 terms: |s_j - q.k_j| <= gamma_64 * sum_i |q_i k_ji|, gamma_n = n u / (1 - n u),
      u = 2^-24 (Higham, Accuracy and Stability, §3.1; an fma chain has one rounding per term).  D = max_j of that, per query.
  (b) argument.  x_j = s_j - m is one fp32 subtraction: relative error u; only |x| <= 87 matters (below -87 the function is clamped at e^-87 <
      2^-125, an absolute error the other terms dwarf), so |dx| <= 87 u.
  (c) exponential.  var_math.h states vm_exp_le0's relative error as "~1 ulp"; read as at most 2 ulp of a binary32 value, eps = 2^-22.
  A softmax does not change when all its scores move together, so (a)-(c) multiply every numerator by a factor in [e^-(D + 87u) (1 - eps),
  e^(D + 87u) (1 + eps)]: a ratio W_b / Z of such sums moves by a factor in [1 / F, F], F = e^(2 (D + 87u)) (1 + eps) / (1 - eps), i.e. by at
  most (F - 1) in absolute terms because the share is <= 1.
  (d) quantisation.  w_j = rint(e_j 2^30) is off by at most 1/2: W_b and Z by at most curL / 2 units of 2^-30 each = curL 2^-31.  Z >= 2^30 (the
      maximal key has e = 1 exactly), so the quotient moves by at most (curL 2^-31 + share * curL 2^-31) / 1 <= curL 2^-30.
  (e) truncation.  The integer division drops less than one unit of 2^-21.
  bound = (F - 1) + curL 2^-30 + 2^-21.
For the model's ranges (unit keys, |q| <= 100: D <= 64 * 2^-24 * 100 = 3.8e-4) the bound is about 8e-4, dominated by (a).

TOLERANCE OF THE HIP ROUTE AGAINST attention_profile_torch (tests/test_attention_profile_gpu.py): measured once, on a CPU, from PyTorch code alone
(no library call): the largest deviation of a per-query share (tokens / SHARE_ONE) between attention_profile_torch on the tiny fixtures with
float32 modules and with float64 modules.  TORCH_F32_VS_F64 holds that figure (one unit of the fixed point), the GPU test allows 8x: the HIP GEMMs
sum in another order than PyTorch's, and 8 covers that with room."""
import numpy as np

SHARE_ONE = 2 ** 21
D16_ENDS = (1, 5, 14, 30, 55, 91, 155, 255, 424, 680)          # the key-scale ends of patch_nums (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
U = 2.0 ** -24
EXP_EPS = 2.0 ** -22

# measured by tests/test_attention_profile_cpu.py::test_torch_twin_f32_against_f64 (which prints it): the largest |f32 - f64| of a per-query share
# on the tiny fixtures (t_pn12345's model: depth 2, patch_nums (1, 2, 3, 4, 5), with and without attn_l2_norm, 3 images): 4.768e-07
TORCH_F32_VS_F64 = 2.0 ** -21
HIP_VS_TORCH_FACTOR = 8


def case_ends(l, curL):
    """the ends array of a (l, curL) case: d16's scale ends up to the queries' first key, then curL"""
    own0 = curL - l
    if own0 == 0:
        return np.asarray([curL], dtype=np.int32)
    assert own0 in D16_ENDS, (l, curL)
    return np.asarray([e for e in D16_ENDS if e <= own0] + [curL], dtype=np.int32)


def make_case(l, curL, rows=3, H=2, seed=0, pad=7, qnorm=(0.5, 100.0), dtype=np.float32):
    """q [rows][l][H*64] with norms spread over qnorm (the model's: temperature <= 100 times a unit vector), kcache [rows][H][curL + pad][64] with unit
    keys and a NaN-filled tail -> dict(q, kc, ends, pn, l, curL, Lmax, rows, H)"""
    rng = np.random.default_rng(seed * 7919 + l * 131 + curL)
    pn = int(round(l ** 0.5))
    assert pn * pn == l
    Lmax = curL + pad
    k = rng.standard_normal((rows, H, curL, 64))
    k /= np.linalg.norm(k, axis=-1, keepdims=True)
    q = rng.standard_normal((rows, l, H, 64))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= rng.uniform(qnorm[0], qnorm[1], size=(rows, l, H, 1))
    kc = np.full((rows, H, Lmax, 64), np.nan, dtype=dtype)
    kc[:, :, :curL] = k.astype(dtype)
    return dict(q=np.ascontiguousarray(q.reshape(rows, l, H * 64).astype(dtype)), kc=kc, ends=case_ends(l, curL), pn=pn, l=l, curL=curL, Lmax=Lmax,
                rows=rows, H=H)


def bin_masks(l, curL, ends, pn, radius):
    """(S1 + 1, l, curL) bool: key j of query t in bin b (the last row: the near bin)"""
    S1 = len(ends)
    j = np.arange(curL)
    m = np.zeros((S1 + 1, l, curL), dtype=bool)
    lo = 0
    for b, e in enumerate(ends):
        m[b] = ((j >= lo) & (j < e))[None, :]
        lo = int(e)
    own0 = curL - l
    t = np.arange(l)
    tk = j - own0
    dy = np.abs((tk // pn)[None, :] - (t // pn)[:, None])
    dx = np.abs((tk % pn)[None, :] - (t % pn)[:, None])
    m[S1] = (tk >= 0)[None, :] & (dy <= radius) & (dx <= radius)
    return m


def reference(case, radius):
    """-> (share (rows, H, l, S1 + 1) float64 real shares, bound (rows, H, l) float64 per query)"""
    q, kc, l, curL, H = case['q'], case['kc'], case['l'], case['curL'], case['H']
    rows = q.shape[0]
    qq = q.astype(np.float64).reshape(rows, l, H, 64).transpose(0, 2, 1, 3)             # (rows, H, l, 64)
    kk = kc[:, :, :curL].astype(np.float64)                                            # (rows, H, curL, 64)
    s = np.einsum('bhtc,bhjc->bhtj', qq, kk)
    sabs = np.einsum('bhtc,bhjc->bhtj', np.abs(qq), np.abs(kk))
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    masks = bin_masks(l, curL, case['ends'], case['pn'], radius).astype(np.float64)     # (S1 + 1, l, curL)
    share = np.einsum('bhtj,stj->bhts', p, masks)
    gamma = 64 * U / (1 - 64 * U)
    D = gamma * sabs.max(-1) + 87 * U
    F = np.exp(2 * D) * (1 + EXP_EPS) / (1 - EXP_EPS)
    bound = (F - 1) + curL * 2.0 ** -30 + 2.0 ** -21
    return share, bound


def run_host(case, radius, tokens=True, call=None, share=None, nan=None):
    """varhip_attn_profile_host_f32 on a case -> (share_sum (rows, H, S1 + 1) int64, nan_count (rows, H) int32, tokens (rows, H, l, S1 + 1) int32 or
    None).  call: the function to run instead (same arguments), share / nan: accumulate into these instead of fresh zeros"""
    from var_amd import hip
    rows, H, l, S1 = case['rows'], case['H'], case['l'], len(case['ends'])
    share = np.zeros((rows, H, S1 + 1), dtype=np.int64) if share is None else share
    nan = np.zeros((rows, H), dtype=np.int32) if nan is None else nan
    tok = np.full((rows, H, l, S1 + 1), -7, dtype=np.int32) if tokens else None
    fn = call or (lambda *a: hip.call_host('attn_profile_host_f32', *a))
    fn(case['q'], case['kc'], rows, l, H, case['curL'], case['Lmax'], case['ends'], S1, case['pn'], radius,
       share, H * (S1 + 1), S1 + 1, nan, tok, H * l * (S1 + 1), l * (S1 + 1))
    return share, nan, tok
