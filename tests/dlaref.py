"""Direct logit attribution in numpy float64: the three kernels of var_amd/csrc/dla.hip restated with their stated
summation orders (the host twins must give these bits), the decomposition of a token's logit by an independent algebraic route (every head's
full vector gamma1 * (W[:, 64h:64h+64] att_h) dotted with the unrounded float64 direction: no transposed u, no rounded ghat), and the bars
the GPU route is held to, derived from the fp32 GEMM bound K * 2^-24 * sum |a| |w| the way tests/gemmcases.py derives its own."""
import numpy as np

U = 2.0 ** -24          # the unit roundoff of fp32
SAFETY = 4.0            # every bar below is SAFETY times a worst-case bound; stated in DESIGN.md section 40


# ---- the stated orders -----------------------------------------------------------------------------------------------------------------
def _butterfly(acc):
    """acc (rows, P) -> (rows,): the xor butterfly P / 2 .. 1"""
    P = acc.shape[1]
    off = P >> 1
    while off >= 1:
        acc = acc + acc[:, np.arange(P) ^ off]
        off >>= 1
    return acc[:, 0]


def seg_lanes(q):
    P = 1
    while P * 2 <= q and P < 64:
        P *= 2
    return P


def lane_sum(terms, P=64):
    """terms (rows, n) float64, n % 4 == 0 -> (rows,): lane i of P adds its groups of four i, i + P, ... in ascending order from +0.0, the
    lanes by the butterfly.  P = 64 is the order of varhip_dla_direction_f32 (element j * 256 + 4 i + c)."""
    rows, n = terms.shape
    q = n // 4
    acc = np.zeros((rows, P), dtype=np.float64)
    lanes = np.arange(P)
    for k0 in range(0, q, P):
        on = lanes[k0 + lanes < q]
        for c in range(4):
            acc[:, on] = acc[:, on] + terms[:, 4 * (k0 + on) + c]
    return _butterfly(acc)


def rowdot(a, b, nseg):
    """varhip_rowdot_seg_f64: a (M, C) fp32, b (M, C) or (C,) fp32 -> (M, nseg) float64"""
    M, C = a.shape
    w = C // nseg
    prod = a.astype(np.float64) * np.broadcast_to(b, a.shape).astype(np.float64)          # exact
    P = seg_lanes(w // 4)
    return np.stack([lane_sum(prod[:, s * w:(s + 1) * w], P) for s in range(nseg)], 1)


def target(logits, gt, against, mode):
    """varhip_dla_target_f32: logits (R, l, V) fp32, gt / against (R, l) int64 -> rival (R, l) int64, value (R, l) fp32"""
    R, l, V = logits.shape
    rival = np.full((R, l), -1, dtype=np.int64)
    value = np.full((R, l), np.nan, dtype=np.float32)
    for r in range(R):
        for t in range(l):
            z, a = logits[r, t], int(gt[r, t])
            b = int(against[r, t]) if mode == 2 else -1
            if not 0 <= a < V or (mode == 2 and not 0 <= b < V) or np.isnan(z).any():
                continue
            if mode == 1:
                if V == 1:
                    continue
                b = int(np.argmax(np.delete(z, a)))                # the first of the greatest: the lowest index
                b += b >= a
            if mode == 0:
                value[r, t] = z[a]
            else:
                rival[r, t] = b
                value[r, t] = np.float32(z[a] - z[b])
    return rival, value


def direction(x, s, sh, W, bias, tok_a, tok_b, l, eps):
    """varhip_dla_direction_f32: x (R * l, C), s / sh (R, C), W (V, C), bias (V,) fp32, tok_a / tok_b (R, l) int64 (tok_b None: no rival)
    -> ghat (R * l, C) fp32, konst, gx (R, l) float64"""
    M, C = x.shape
    R, V = M // l, W.shape[0]
    a = tok_a.reshape(-1)
    b = np.zeros_like(a) if tok_b is None else tok_b.reshape(-1)
    ok = (a >= 0) & (a < V) & (b >= 0) & (b < V)
    a, b = np.where(ok, a, 0), np.where(ok, b, 0)
    f64 = lambda t: t.astype(np.float64)
    row = np.arange(M) // l
    r = f64(W[a]) if tok_b is None else f64(W[a]) - f64(W[b])
    g = r * (1.0 + f64(s)[row])
    xd = f64(x)
    S1, S2, G, K = lane_sum(xd), lane_sum(xd * xd), lane_sum(g), lane_sum(r * f64(sh)[row])
    mu = S1 / C
    var = np.maximum(S2 / C - mu * mu, 0.0)
    sigma = np.sqrt(var + np.float64(np.float32(eps)))
    mg = G / C
    ghat = ((g - mg[:, None]) / sigma[:, None]).astype(np.float32)
    gx = lane_sum(f64(ghat) * xd)
    konst = K + (f64(bias[a]) - (0.0 if tok_b is None else f64(bias[b])))
    ghat[~ok] = np.nan
    return ghat, np.where(ok, konst, np.nan).reshape(R, l), np.where(ok, gx, np.nan).reshape(R, l)


# ---- the decomposition, by another route -------------------------------------------------------------------------------------------------
def ghat64(x, s, sh, W, bias, a, b, l, eps):
    """the unrounded direction and konst in plain float64 (numpy's own mean and variance): x (M, C), a / b (M,) (b None: no rival)"""
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    row = np.arange(x.shape[0]) // l
    r = f64(W[a]) - (0.0 if b is None else f64(W[b]))
    g = r * (1.0 + f64(s)[row])
    xd = f64(x)
    sigma = np.sqrt(xd.var(-1) + np.float64(np.float32(eps)))
    gh = (g - g.mean(-1, keepdims=True)) / sigma[:, None]
    konst = (r * f64(sh)[row]).sum(-1) + f64(bias[a]) - (0.0 if b is None else f64(bias[b]))
    return gh, konst


def decompose(gh, e, x_in, x_mid, x_out, att, g1, proj_w, proj_b, l, H):
    """the terms of one block from its tapped activations, all float64: gh (M, C) the direction; x_in, x_mid, x_out, att (M, C); g1 (R, C);
    proj_w (C, C), proj_b (C,).  The head term is gh . (gamma1 * (W[:, 64h:64h+64] att_h)): the head's whole vector, not u.
    -> dict(attn, mlp, attn_bias (M,), head (M, H)) and the bars' ingredients Q (M, H) = sum_ij |gh_i g1_i| |W_ij| |att_j| over the head's j"""
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    M, C = gh.shape
    row = np.arange(M) // l
    g1r = f64(g1)[row]
    w, at = f64(proj_w), f64(att)
    hw = C // H
    head = np.stack([(gh * (g1r * (at[:, h * hw:(h + 1) * hw] @ w[:, h * hw:(h + 1) * hw].T))).sum(-1) for h in range(H)], 1)
    Q = ((np.abs(gh * g1r) @ np.abs(w)) * np.abs(at)).reshape(M, H, hw).sum(-1)
    return dict(attn=(gh * (f64(x_mid) - f64(x_in))).sum(-1), mlp=(gh * (f64(x_out) - f64(x_mid))).sum(-1),
                attn_bias=(gh * g1r * f64(proj_b)).sum(-1), head=head, Q=Q,
                mag_attn=(np.abs(gh) * (np.abs(f64(x_mid)) + np.abs(f64(x_in)))).sum(-1),
                mag_mlp=(np.abs(gh) * (np.abs(f64(x_out)) + np.abs(f64(x_mid)))).sum(-1),
                mag_bias=(np.abs(gh * g1r) * np.abs(f64(proj_b))).sum(-1))


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
def bar_dot(mag, ref):
    """a float64 dot of fp32 vectors against a direction rounded to fp32 once (U * sum |gh| |v|, which also covers the one rounding of
    gh * gamma1) and rounded to fp32 once at the end (U * |term|), times SAFETY"""
    return SAFETY * U * (2.0 * mag + np.abs(ref)) + 1e-30


def bar_head(Q, ref, C):
    """the head term reads u from the fp32 GEMM over K = C: |u_j - exact| <= C * U * sum_i |gg_i| |W_ij|, so the term is within C * U * Q;
    the roundings of gg, of ghat and of the result add 3 U Q at most"""
    return SAFETY * U * ((C + 3.0) * Q + np.abs(ref)) + 1e-30


def bar_heads_sum(Q, mag_attn, C):
    """sum_h head + attn_bias - attn: the u GEMM's bound, once more for the proj GEMM that made x_mid (the same Q: the same operands in the
    other order), and the residual add's rounding of x_mid"""
    return SAFETY * U * (2.0 * (C + 3.0) * Q.sum(-1) + 2.0 * mag_attn) + 1e-30


def bar_residual(xn_abs_w, mag_x, C):
    """value - (konst + gh . x): the head GEMM's bound over K = C on the one or two logits read, xn_abs_w = sum_c |xn_c| (|W[a]_c| + |W[b']_c|),
    plus the fp32 LayerNorm in front of it (a few U relative per element, inside the same sum) and the rounded direction"""
    return SAFETY * U * ((C + 8.0) * xn_abs_w + 2.0 * mag_x) + 1e-30
