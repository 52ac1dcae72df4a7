"""Decks, float64 references and derived bars for the VAE's row and element-wise kernels (var_amd/csrc/rowops.hip, rowops16.hip): GroupNorm
statistics (from the map and from a convolution's partials), the scale/shift table, GroupNorm apply (+ SiLU) in fp32 / fp16 / bf16, the row softmax,
the layout copies and the casts.  Shared by tests/test_rowops_cpu.py (references against torch, seam coverage, emulations inside the bars, planted
slips outside them) and tests/test_rowops_gpu.py (the kernels, every operand in a guard arena).

REFERENCES are written from the definitions of the reference model, in float64 numpy, not from the kernels:
  GroupNorm(G, C, eps) of basic_vae.py: per sample and group, mean and BIASED variance over (HW, C / G), y = (x - mean) / sqrt(var + eps) gamma + beta;
  SiLU y sigmoid(y); the attention's softmax(x scale) over the last axis; permute(0, 2, 1) for the layout copies; torch's CPU casts.

SEAMS.  A flavour (f32: vec = 4, C <= 1024; f16 / bf16: vec = 8, C <= 2048) gives every thread one vector of `vec` channels (column q = tid % (C / vec))
and row prow = tid / (C / vec) of rpp = 256 / (C / vec) pixel rows; a block walks one chunk of 256 pixels.  seams_of() restates, from (B, HW, C, G)
alone, which side of every seam a case is on: idle threads (256 - rpp (C / vec) > 0), a vector that straddles two groups (cpg % vec != 0), the fp32
kernels' 4-way unrolled pixel loop `p + 3 rpp < p1` (not entered at HW = 3 rpp, entered at 3 rpp + 1, a scalar tail behind it), the partial last
chunk, G above the 256 threads that fold the groups.  GN_SEAMS / PART_SEAMS / SOFTMAX_SEAMS list what each deck must reach; the CPU test recomputes
the table from the deck and refuses an empty row.

BARS.  u = 2^-24 (fp32 rounding), v = 2^-53 (float64), h = 2^-11 / 2^-8 (fp16 / bf16 rounding: 11 / 8 significant bits), one function per kernel, docstring = derivation.
Nothing in them is measured; profiles/rowops_bar_margins.txt records the room they leave on an MI355X and is not an input.
"""
import functools
import zlib

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
EPS = float(np.float32(1e-6))            # the engines pass 1e-6f: the float32 value is what every kernel adds
GN_PIX = 256
FLAVOURS = {
    'f32': dict(vec=4, cmax=1024, fmax=float(np.finfo(np.float32).max), h=0.0, tiny=0.0, unrolled=True),
    'f16': dict(vec=8, cmax=2048, fmax=65504.0, h=2.0 ** -11, tiny=2.0 ** -25, unrolled=False),                      # tiny: half the smallest subnormal
    'bf16': dict(vec=8, cmax=2048, fmax=float((2 - 2.0 ** -7) * 2.0 ** 127), h=2.0 ** -8, tiny=2.0 ** -134, unrolled=False),
}
E_EXP = 4e-7                             # vm_exp, include/var_math.h: "relative error ~1 ulp"; the bound the project asserts for it (test_vm_log_exp_accuracy)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def torch_dtype(flav):
    import torch
    return {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[flav]


def round_to(flav, a):
    """float array -> the flavour's nearest value (torch's CPU cast, round to nearest even), as float64"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch_dtype(flav)).double().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
def gn_moments64(x, G):
    """x [B][HW][C] -> (mean, biased variance) [B][G] in float64, two passes (the definition)"""
    B, HW, C = x.shape
    xg = np.asarray(x, np.float64).reshape(B, HW, G, C // G)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return mean, var


def gn_stats64(x, G, eps=EPS):
    """-> (mean, rstd) [B][G] float64, rstd = (var + eps)^-1/2"""
    mean, var = gn_moments64(x, G)
    return mean, 1.0 / np.sqrt(var + eps)


def silu64(y):
    y = np.asarray(y, np.float64)
    with np.errstate(over='ignore'):
        return y / (1.0 + np.exp(-y))


def per_channel(st, C):
    """[B][G] -> [B][1][C]: every channel's group value"""
    G = st.shape[1]
    return np.repeat(np.asarray(st, np.float64), C // G, axis=1)[:, None, :]


def gn_apply64(x, mean, rstd, gamma, beta, silu):
    """y = (x - mean) rstd gamma + beta per element of x [B][HW][C] (mean, rstd [B][G]), then SiLU; float64"""
    C = x.shape[2]
    y = (np.asarray(x, np.float64) - per_channel(mean, C)) * per_channel(rstd, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return silu64(y) if silu else y


def gn_part_stats64(part, HW, G, eps=EPS):
    """part [B][nblk][C][2] (sum, sum of squares per block and channel) -> (mean, rstd) [B][G] of the map the blocks tile"""
    B, nblk, C, _ = part.shape
    s = np.asarray(part, np.float64).sum(axis=1).reshape(B, G, C // G, 2).sum(axis=2)
    n = float(HW) * (C // G)
    mean = s[..., 0] / n
    var = np.maximum(s[..., 1] / n - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def softmax_rows64(x, scale):
    """softmax(x scale) over the last axis; scale is the fp32 value the kernel receives"""
    e = np.asarray(x, np.float64) * float(np.float32(scale))
    p = np.exp(e - e.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def nchw_to_nhwc(a):
    """[B][C][HW] -> [B][HW][C]"""
    return np.ascontiguousarray(a.transpose(0, 2, 1))


def nhwc_to_nchw(a):
    """[B][HW][C] -> [B][C][HW]"""
    return np.ascontiguousarray(a.transpose(0, 2, 1))


def nchw_to_nhwc_pad(a, Cpad):
    B, C, HW = a.shape
    out = np.zeros((B, HW, Cpad), a.dtype)
    out[:, :, :C] = a.transpose(0, 2, 1)
    return out


def cast_to16(flav, a32):
    """float32 numpy -> the 16-bit patterns (uint16) of torch's CPU cast"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a32)).to(torch_dtype(flav)).view(torch.int16).numpy().view(np.uint16)


def cast_from16(flav, bits16):
    """uint16 patterns -> float32 numpy by torch's CPU cast"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits16).view(np.int16)).view(torch_dtype(flav)).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# bars
def bar_stats(mean, var, n, eps=EPS):
    """-> (bar of mean, bar of rstd) [B][G] for (mean, var) the float64 moments of a group of n values.
    The kernels sum x and x^2 in float64 (any order: at most n - 1 additions each, relative v per addition and per square), form mean = s / n,
    var = s2 / n - mean^2 clamped at 0, and round mean and 1 / sqrt(var + eps) once to fp32.
      mean: u |mean| for the fp32 rounding, plus the float64 sum: (n - 1) v sum|x| / n <= n v sqrt(mean^2 + var) (Cauchy-Schwarz), plus half the
            smallest fp32 subnormal.
      rstd: s2 / n = mean^2 + var is a sum of n non-negative terms: absolute error (n + 1) v (mean^2 + var).  mean^2: 2 |mean| dmean + v mean^2
            <= (2 n + 1) v (mean^2 + var).  The subtraction rounds once more.  So the variance is off by at most (3 n + 3) v (mean^2 + var), a relative
            error (3 n + 3) v (mean^2 + var) / (var + eps) of var + eps and HALF that of rstd: the cancellation term, with the summation length n.
            sqrt, the division and the fp32 rounding: 2 v + u."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    m2 = mean * mean + var
    bm = U32 * np.abs(mean) + n * U64 * np.sqrt(m2) + 2.0 ** -150
    rstd = 1.0 / np.sqrt(var + eps)
    br = rstd * (U32 + 2 * U64 + 0.5 * (3 * n + 3) * U64 * m2 / (var + eps))
    return bm, br


def bar_apply_f32(x, mean, rstd, gamma, beta):
    """k_gn_apply: y = fl(fl(fl(fl(x - m) r) g) + b) on the fp32 stats it is given: four roundings.  With t = (x - m) r g the first three are each
    relative u of (what becomes) t, the last u of y: u (3 |t| + |y|), times (1 + 2^-20) for the second order, plus the smallest fp32 subnormal."""
    C = x.shape[2]
    t = (np.asarray(x, np.float64) - per_channel(mean, C)) * per_channel(rstd, C) * np.asarray(gamma, np.float64)
    y = t + np.asarray(beta, np.float64)
    return U32 * (3 * np.abs(t) + np.abs(y)) * (1 + 2.0 ** -20) + 2.0 ** -149


def bar_scale_shift(mean, rstd, gamma, beta, C):
    """k_gn_scale_shift / the per-channel constants of k_gn16_apply: sc = fl(r g) (one rounding: u |sc|); sh = fl(b - fl(m sc)) on the ROUNDED sc: two
    roundings, u |m sc| + u |sh|; each plus the smallest fp32 subnormal.  -> (bar of sc, bar of sh given sc) [B][1][C]"""
    sc = per_channel(rstd, C) * np.asarray(gamma, np.float64)
    msc = per_channel(mean, C) * sc
    sh = np.asarray(beta, np.float64) - msc
    return U32 * np.abs(sc) + 2.0 ** -149, U32 * (np.abs(msc) + np.abs(sh)) * (1 + 2.0 ** -20) + 2.0 ** -149


def bar_affine16(x, mean, rstd, gamma, beta):
    """the fp32 value y = fma(x, sc, sh) of k_gn16_apply before SiLU and the store, sc = fl(r g), sh = fl(b - fl(m sc)), against x r g + b - m r g:
       sc is off by u |r g|: u |x r g| through the product and u |m r g| through sh;   fl(m sc): u |m r g|;   the subtraction: u |sh|;   the fma: u |y|.
    bar = u (|x sc| + 2 |m sc| + |sh| + |y|) (1 + 2^-20) + 2^-149 (|x| + |m| + 1).  The |m sc| term is what grows with |mean| / std; the last term is
    the absolute rounding of a subnormal sc or m sc."""
    C = x.shape[2]
    x = np.asarray(x, np.float64)
    m = per_channel(mean, C)
    sc = per_channel(rstd, C) * np.asarray(gamma, np.float64)
    msc = m * sc
    sh = np.asarray(beta, np.float64) - msc
    y = x * sc + sh
    return U32 * (np.abs(x * sc) + 2 * np.abs(msc) + np.abs(sh) + np.abs(y)) * (1 + 2.0 ** -20) + 2.0 ** -149 * (np.abs(x) + np.abs(m) + 1)


def bar_propagated(x, mean, rstd, gamma, dmean, drstd):
    """what an error (dmean, drstd) [B][G] of the statistics moves y = (x - m) r g + b by: |r g| dmean + |x - m| |g| drstd (first order)"""
    C = x.shape[2]
    g = np.abs(np.asarray(gamma, np.float64))
    return per_channel(rstd, C) * g * per_channel(dmean, C) + np.abs(np.asarray(x, np.float64) - per_channel(mean, C)) * g * per_channel(drstd, C)


SILU_Z0 = -1.2784645427610738          # the minimum of SiLU: 1 + e^-z (1 + z) = 0


def bar_silu(y, by):
    """gn_fast_silu / gn16_silu: y rcp(1 + exp2(c y)), c = fl(-log2 e), on a y known to within by.
      * the error of y moves SiLU by at most max(|silu(y +- by) - silu(y)|): SiLU is monotone on either side of its one minimum silu(Z0), so the
        end points bound the interval, unless it holds Z0, where silu(y) - silu(Z0) is the third candidate;
      * relative, on |silu(y)|: c and the product c y round once each, an absolute error 2 u |c y| of the exponent, relative 2 u |y| of the power;
        exp2 itself 1 ulp = 2 u; 1 + e: u (the error of e enters with weight e / (1 + e) <= 1); rcp: 1 ulp = 2 u; the product: u.  (2 |y| + 6) u,
        times 1.001 for the second order;
      * absolute floor: where exp2 overflows (y below -88.7) the kernel returns y 0, and where 1 + e >= 2^126 the reciprocal is subnormal and may be
        returned as 0, as may a subnormal product: the sigmoid is then below 2^-126, the smallest normal fp32, and the result is off by at most
        (|y| + 1) 2^-126."""
    y = np.asarray(y, np.float64)
    s = silu64(y)
    prop = np.maximum(np.maximum(np.abs(silu64(y + by) - s), np.abs(silu64(y - by) - s)), np.where(np.abs(y - SILU_Z0) <= by, s - silu64(SILU_Z0), 0.0))
    return prop + 1.001 * (2 * np.abs(y) + 6) * U32 * np.abs(s) + (np.abs(y) + 1) * 2.0 ** -126


def bar_store(flav, ref, b):
    """the one rounding to the flavour at the store of a value within b of ref: h (|ref| + b) + half the smallest subnormal (nothing for f32)"""
    f = FLAVOURS[flav]
    return b + f['h'] * (np.abs(ref) + b) + f['tiny']


def bar_apply(flav, x, mean, rstd, gamma, beta, silu, extra=0.0):
    """the whole bar of varhip_gn_apply_<flav> on the fp32 statistics (mean, rstd) it is given; extra: an error of y from elsewhere (the composite:
    bar_propagated of the statistics' own bars).  -> float64 [B][HW][C]"""
    by = (bar_apply_f32 if flav == 'f32' else bar_affine16)(x, mean, rstd, gamma, beta) + extra
    if silu:
        by = bar_silu(gn_apply64(x, mean, rstd, gamma, beta, 0), by)
    return bar_store(flav, gn_apply64(x, mean, rstd, gamma, beta, silu), by) if flav != 'f32' else by


def bar_softmax(x, scale):
    """k_softmax_rows against softmax_rows64.  e_j = fl(x_j scale) (u |e_j|; exact when scale == 1), m = max e (one of them), d_j = fl(e_j - m) (u |d_j|):
    the exponent is off by a_j = u (|e_j| + |m| + |d_j|) (without the first two for scale == 1), a relative error a_j of p_j; vm_exp adds E_EXP, and
    returns exactly 0 below -87 where the true value is < 2^-125.  S sums n terms (canonical order, at most n - 1 roundings on any term), out = p / S
    rounds once.  With eta_j = E_EXP + a_j:
        bar_i = out_i (eta_i + sum_j out_j eta_j + n u) + 2^-125 (1 + n out_i)        (S >= 1)."""
    s = float(np.float32(scale))
    e = np.asarray(x, np.float64) * s
    n = e.shape[1]
    m = e.max(axis=1, keepdims=True)
    a = U32 * (np.abs(e - m) + (0.0 if s == 1.0 else np.abs(e) + np.abs(m)))
    out = softmax_rows64(x, scale)
    eta = np.where(out > 0, E_EXP + a, 0.0)                    # (a term that is exactly 0 carries no relative error; its floor is below)
    return out * (eta + (out * eta).sum(axis=1, keepdims=True) + n * U32) + 2.0 ** -125 * (1 + n * out)


# ---------------------------------------------------------------------------------------------------------------------
# geometry of the GroupNorm kernels, restated
def geom(flav, C):
    vec = FLAVOURS[flav]['vec']
    cv = C // vec
    rpp = 256 // cv
    return dict(vec=vec, cv=cv, rpp=rpp, idle=256 - rpp * cv)


def unroll_bound(flav, C):
    """the largest HW (<= 256) at which NO thread enters the 4-way unrolled loop `p + 3 rpp < p1`: prow = 0 enters at 3 rpp < HW"""
    return 3 * geom(flav, C)['rpp']


def thread_pixels(HW, rpp):
    """pixels each row prow of threads walks, per chunk: [(chunk length, [count per prow])]"""
    out = []
    for p0 in range(0, HW, GN_PIX):
        L = min(GN_PIX, HW - p0)
        out.append((L, [len(range(prow, L, rpp)) for prow in range(rpp)]))
    return out


def seams_of(flav, case):
    """the seam names (module docstring) the geometry (B, HW, C, G) reaches for that flavour"""
    B, HW, C, G = case
    f, g = FLAVOURS[flav], geom(flav, C)
    vec, rpp, cpg = g['vec'], g['rpp'], C // G
    s = {f'B={B}', f'HW={HW}', 'idle threads' if g['idle'] else 'no idle thread'}
    if C == vec: s.add('C minimal')
    if C == f['cmax']: s.add('C maximal')
    if cpg == 1: s.add('cpg=1')
    if cpg == 3: s.add('cpg=3')
    if cpg == vec: s.add('cpg=vec')
    if cpg > vec and cpg % vec == 0: s.add('cpg multiple of vec')
    if cpg % vec: s.add('vector straddles groups')
    if G == 1: s.add('G=1')
    if G == C: s.add('G=C')
    if G == 32: s.add('G=32')
    if G > 256: s.add('G above 256')
    if HW > GN_PIX and HW % GN_PIX: s.add('partial last chunk')
    if HW % GN_PIX == 0: s.add('whole chunks only')
    if HW < rpp: s.add('rows without a pixel')
    if f['unrolled']:
        if HW == unroll_bound(flav, C): s.add('unrolled loop: at the bound, not entered')
        if HW == unroll_bound(flav, C) + 1: s.add('unrolled loop: one past the bound, entered')
        if any(c >= 4 and c % 4 for _, counts in thread_pixels(HW, rpp) for c in counts): s.add('unrolled loop with a scalar tail')
        if any(c >= 4 and c % 4 == 0 for _, counts in thread_pixels(HW, rpp) for c in counts): s.add('unrolled loop without a tail')
    else:
        if HW == rpp: s.add('one pixel per thread')
        if HW == rpp + 1: s.add('a second pass for one row')
    return s


_COMMON_SEAMS = ['B=1', 'B=3', 'HW=1', 'HW=2', 'HW=255', 'HW=256', 'HW=257', 'HW=513', 'idle threads', 'no idle thread', 'C minimal', 'C maximal',
                 'cpg=1', 'cpg=3', 'cpg=vec', 'cpg multiple of vec', 'vector straddles groups', 'G=1', 'G=C', 'G=32', 'G above 256', 'partial last chunk',
                 'whole chunks only', 'rows without a pixel']
GN_SEAMS = {
    'f32': _COMMON_SEAMS + ['unrolled loop: at the bound, not entered', 'unrolled loop: one past the bound, entered', 'unrolled loop with a scalar tail',
                            'unrolled loop without a tail'],
    'f16': _COMMON_SEAMS + ['one pixel per thread', 'a second pass for one row'],
    'bf16': _COMMON_SEAMS + ['one pixel per thread', 'a second pass for one row'],
}


def gn_geometries(flav):
    """(B, HW, C, G) of the flavour's geometry deck; B HW C <= 2^21"""
    if flav == 'f32':
        ub = unroll_bound('f32', 96)                   # rpp = 10: 30
        deck = [(1, ub, 96, 32), (1, ub + 1, 96, 32), (3, 257, 96, 32), (1, 255, 1020, 1020), (1, 513, 1020, 4), (1, 256, 1024, 32), (3, 2, 4, 1),
                (1, 1, 4, 4), (1, 513, 32, 32), (1, 257, 640, 32), (1, 2, 1024, 512), (1, 255, 12, 4), (1, 256, 12, 4), (1, 513, 8, 1), (1, 256, 128, 32)]
    else:
        rpp = geom(flav, 104)['rpp']                   # 19
        deck = [(1, rpp, 104, 8), (1, rpp + 1, 104, 8), (3, 257, 104, 104), (1, 255, 1032, 344), (1, 256, 2048, 32), (1, 513, 2048, 256), (3, 2, 8, 1),
                (1, 1, 8, 8), (1, 513, 96, 32), (1, 257, 640, 32), (1, 2, 2048, 1024), (1, 256, 128, 1), (1, 255, 24, 8), (1, 256, 32, 32)]
    for B, HW, C, G in deck:
        assert B * HW * C <= 1 << 21 and C % G == 0 and C % FLAVOURS[flav]['vec'] == 0 and C <= FLAVOURS[flav]['cmax']
    return deck


REGIME_GEOMETRIES = [(1, 257, 96, 32), (3, 31, 640, 32)]          # the straddling cpg = 3, and the decoder's widest map


def regimes(flav):
    return ['const', 'mean300', 'outlier', 'silu_neg'] + (['mean1e4'] if flav == 'f32' else [])


def gn_cases(flav):
    """[(id, (B, HW, C, G), regime)]: every geometry on the plain values, the other value regimes on REGIME_GEOMETRIES"""
    out = [('randn %d-%d-%d-%d' % g, g, 'randn') for g in gn_geometries(flav)]
    out += [('%s %d-%d-%d-%d' % ((r,) + g), g, r) for r in regimes(flav) for g in REGIME_GEOMETRIES]
    return out


class Built:
    pass


@functools.lru_cache(maxsize=4)
def build_gn(flav, geometry, regime):
    """-> Built: x [B][HW][C] float64 holding values of the flavour exactly, gamma, beta float32.  Regimes (issue): randn 1.7 + 0.3; const: group 0 of
    every sample is the constant 0.75 (var = 0 exactly: 0.75 and 0.5625 n are exact in float64); mean300 / mean1e4: mean + randn; outlier: one value per
    group at the format's largest finite / 4; silu_neg: uniform(-1, 1) (|z| <= 1.8) with gamma = 16, beta = -90: y in [-120, -60]"""
    B, HW, C, G = geometry
    cpg = C // G
    rng = _rng('gn', flav, geometry, regime)
    b = Built()
    b.flav, b.geometry, b.regime = flav, geometry, regime
    x = rng.standard_normal((B, HW, C))
    b.gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    b.beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    if regime == 'randn':
        x = x * 1.7 + 0.3
    elif regime == 'const':
        x = x * 1.7 + 0.3
        x[:, :, :cpg] = 0.75
    elif regime == 'mean300':
        x = x + 300.0
    elif regime == 'mean1e4':
        x = x + 1e4
    elif regime == 'outlier':
        for bb in range(B):
            for g in range(G):
                x[bb, (HW - 1 - 7 * g - bb) % HW, g * cpg + g % cpg] = (-1) ** g * FLAVOURS[flav]['fmax'] / 4      # (sample 0, group 0: in the last pixel; the sign alternates, or all groups would share their statistics)
    elif regime == 'silu_neg':
        x = rng.uniform(-1, 1, (B, HW, C))
        b.gamma = np.full(C, 16.0, np.float32)
        b.beta = np.full(C, -90.0, np.float32)
    else:
        raise ValueError(regime)
    b.x = round_to(flav, x)
    return b


def group_of(C, G, slip=None):
    """channel -> group; slip 'group': the index off by one channel"""
    c = np.arange(C)
    return ((c + 1) // (C // G)) % G if slip == 'group' else c // (C // G)


# ---------------------------------------------------------------------------------------------------------------------
# emulations of the kernels' stated order in numpy fp32 / float64, with the planted slips
SLIPS = ('group', 'pixel', 'eps')        # a group index off by one channel; the last pixel dropped; rstd without eps


def _seq_sum(a):
    """sum over the last axis, one addition after the other in float64 (the longest chain a kernel's order can have)"""
    return np.cumsum(a, axis=-1)[..., -1] if a.shape[-1] else np.zeros(a.shape[:-1])


def emu_stats(x, G, eps=EPS, slip=None):
    """the kernels' statistics: float64 sums of x and x^2, mean = s / n, var = s2 / n - mean^2 clamped at 0, both results rounded to fp32.
    -> stats [B][G][2] float32"""
    B, HW, C = x.shape
    cpg = C // G
    xd = np.asarray(x, np.float64)
    if slip == 'group':
        xd = np.roll(xd, 1, axis=2)                      # group g collects channels g cpg - 1 .. (g + 1) cpg - 2
    if slip == 'pixel':
        xd = xd[:, :HW - 1]
    xg = xd.reshape(B, xd.shape[1], G, cpg).transpose(0, 2, 1, 3).reshape(B, G, -1)
    n = float(HW) * cpg
    mean = _seq_sum(xg) / n
    var = np.maximum(_seq_sum(xg * xg) / n - mean * mean, 0.0)
    with np.errstate(divide='ignore'):
        rstd = 1.0 / np.sqrt(var + (0.0 if slip == 'eps' else eps))
    return np.stack([mean, rstd], axis=-1).astype(np.float32)


def emu_part_stats(part, HW, G, eps=EPS, slip=None):
    """k_gn_final_part: lane j sums blocks j, j + 64, ... (channels of the group in order), butterfly over the lanes; float64; fp32 results.
    Slips: 'group' as above; 'pixel' here drops the last BLOCK; 'eps'."""
    B, nblk, C, _ = part.shape
    cpg = C // G
    p = np.asarray(part, np.float64)
    if slip == 'group':
        p = np.roll(p, 1, axis=2)
    if slip == 'pixel':
        p = p[:, :nblk - 1]
    lanes = np.zeros((B, G, 64, 2))
    for k in range(p.shape[1]):
        for c in range(cpg):
            lanes[:, :, k % 64] += p[:, k].reshape(B, G, cpg, 2)[:, :, c]
    w = 64
    while w > 1:
        lanes = lanes[:, :, :w // 2] + lanes[:, :, w // 2:w]
        w //= 2
    n = float(HW) * cpg
    mean = lanes[:, :, 0, 0] / n
    var = np.maximum(lanes[:, :, 0, 1] / n - mean * mean, 0.0)
    with np.errstate(divide='ignore'):
        rstd = 1.0 / np.sqrt(var + (0.0 if slip == 'eps' else eps))
    return np.stack([mean, rstd], axis=-1).astype(np.float32)


def _fast_silu32(y):
    F = np.float32
    with np.errstate(over='ignore'):
        return (y * (F(1) / (F(1) + np.exp2(F(-1.44269504088896341) * y)))).astype(F)


def emu_scale_shift(stats, gamma, beta, slip=None):
    """sc = fl(r g), sh = fl(b - fl(m sc)): SEPARATELY rounded product and difference (no fma; tests/test_rowops_gpu.py says where that was read).
    -> table [B][2][C] float32"""
    B, G, _ = stats.shape
    C = gamma.shape[0]
    gi = group_of(C, G, slip)
    m, r = stats[:, gi, 0].astype(np.float32), stats[:, gi, 1].astype(np.float32)
    sc = (r * gamma.astype(np.float32)[None]).astype(np.float32)
    sh = (beta.astype(np.float32)[None] - (m * sc).astype(np.float32)).astype(np.float32)
    return np.stack([sc, sh], axis=1)


def emu_apply(flav, x, stats, gamma, beta, silu, slip=None):
    """varhip_gn_apply_<flav> on stats [B][G][2] float32, in the kernel's order: f32 ((x - m) r) g + b rounded after every operation; 16-bit
    fma(x, sc, sh) (the product of a 16-bit x and an fp32 sc is exact in float64: one rounding) then the store's rounding.  SiLU as the kernels
    write it, in fp32.  slip 'pixel': the last pixel is not written (NaN, the tests' sentinel).  -> float64 [B][HW][C]"""
    F = np.float32
    B, HW, C = x.shape
    G = stats.shape[1]
    gi = group_of(C, G, slip)
    with np.errstate(over='ignore', invalid='ignore'):
        if flav == 'f32':
            m, r = stats[:, gi, 0][:, None, :], stats[:, gi, 1][:, None, :]
            y = ((x.astype(F) - m) * r) * gamma.astype(F) + beta.astype(F)
        else:
            t = emu_scale_shift(stats, gamma, beta, slip)
            y = (np.asarray(x, np.float64) * t[:, 0].astype(np.float64)[:, None, :] + t[:, 1].astype(np.float64)[:, None, :]).astype(F)
        y = y.astype(F)
        if silu:
            y = _fast_silu32(y)
    out = round_to(flav, y) if flav != 'f32' else y.astype(np.float64)
    if slip == 'pixel':
        out[:, HW - 1] = np.nan
    return out


def emu_softmax(x, scale, slip=None):
    """k_softmax_rows in fp32: lane j sums its entries j, j + 64, ... in order, then the butterfly.  slip 'last': the last entry is left out of the sum"""
    F = np.float32
    rows, n = x.shape
    e = (x.astype(F) * F(scale)).astype(F)
    m = e.max(axis=1, keepdims=True)
    d = (e - m).astype(F)
    with np.errstate(under='ignore'):
        p = np.where(d > F(-87), np.exp(d.astype(np.float64)).astype(F), F(0)).astype(F)
    q = np.zeros((rows, 16 * 64), F)
    q[:, :n - 1 if slip == 'last' else n] = p[:, :n - 1 if slip == 'last' else n]
    lanes = np.zeros((rows, 64), F)
    for t in range(16):
        lanes = (lanes + q[:, 64 * t:64 * t + 64]).astype(F)
    w = 64
    while w > 1:
        lanes = (lanes[:, :w // 2] + lanes[:, w // 2:w]).astype(F)
        w //= 2
    with np.errstate(divide='ignore', invalid='ignore'):
        return (p / lanes[:, :1]).astype(F)


def within(got, ref, bar):
    """every element within its bar (a NaN is outside)"""
    with np.errstate(invalid='ignore'):
        return bool((np.abs(np.asarray(got, np.float64) - ref) <= bar).all())


def margin(got, ref, bar):
    """max |got - ref| / bar (inf for a NaN or an error over a zero bar)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(err == 0, 0.0, err / bar)
    return float('inf') if not np.isfinite(q).all() else float(q.max())


# ---------------------------------------------------------------------------------------------------------------------
# gn_stats_part: partials of a random float64 map split into nblk blocks of pixels
PART_CASES = [('part B=%d nblk=%d HW=%d C=%d G=%d' % c, c) for c in
              [(1, 1, 7, 96, 32), (3, 2, 130, 64, 64), (1, 63, 200, 12, 4), (1, 64, 64, 32, 1), (2, 65, 257, 96, 32), (1, 130, 520, 640, 32)]]
PART_SEAMS = ['nblk=1', 'nblk=2', 'nblk=63', 'nblk=64', 'nblk=65', 'nblk=130', 'lanes without a block', 'a lane with two blocks', 'a lane with three blocks',
              'cpg=1', 'cpg=3', 'G=1', 'B=3']


def part_seams_of(case):
    B, nblk, HW, C, G = case
    s = {f'nblk={nblk}'}
    if nblk < 64: s.add('lanes without a block')
    if 64 < nblk <= 128: s.add('a lane with two blocks')
    if nblk > 128: s.add('a lane with three blocks')
    if C // G in (1, 3): s.add(f'cpg={C // G}')
    if G == 1: s.add('G=1')
    if B == 3: s.add('B=3')
    return s


@functools.lru_cache(maxsize=None)
def build_part(case):
    """-> (map [B][HW][C] float64, part [B][nblk][C][2] float64): blocks are consecutive runs of pixels (np.array_split: lengths differ by one)"""
    B, nblk, HW, C, G = case
    x = _rng('part', case).standard_normal((B, HW, C)) * 1.7 + 0.3
    part = np.zeros((B, nblk, C, 2))
    for k, idx in enumerate(np.array_split(np.arange(HW), nblk)):
        part[:, k, :, 0] = x[:, idx].sum(axis=1)
        part[:, k, :, 1] = (x[:, idx] ** 2).sum(axis=1)
    return x, part


# gn_scale_shift: (B, C, G); no constraint on C
SCALE_SHIFT_CASES = [(1, 96, 32), (3, 640, 32), (2, 12, 12), (1, 8, 1), (1, 1032, 344), (2, 6, 2), (1, 2048, 32)]


@functools.lru_cache(maxsize=None)
def build_scale_shift(case):
    """-> (stats [B][G][2], gamma, beta) float32: means of either sign up to |mean| rstd ~ 300 (sample 0, group 0: mean 300, rstd 1)"""
    B, C, G = case
    rng = _rng('ss', case)
    stats = np.stack([rng.standard_normal((B, G)) * 3, rng.uniform(0.1, 5, (B, G))], axis=-1).astype(np.float32)
    stats[0, 0] = (300.0, 1.0)
    return stats, (1 + 0.2 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# softmax: (rows, n, kind, scale)
S640 = 640 ** -0.5
SOFTMAX_CASES = [(5, 1, 'plain', 1.0), (1, 63, 'plain', S640), (5, 64, 'equal', 1.0), (5, 65, 'peak', S640), (1, 255, 'neg1e30', 1.0), (5, 1000, 'plain', S640),
                 (5, 1023, 'peak', 1.0), (4099, 1024, 'plain', S640), (1, 1024, 'equal', S640), (5, 1024, 'neg1e30', S640), (5, 1024, 'peak', S640),
                 (4099, 64, 'plain', 1.0), (5, 255, 'equal', S640)]
SOFTMAX_SEAMS = ['n=1', 'n=63', 'n=64', 'n=65', 'n=255', 'n=1000', 'n=1023', 'n=1024', 'rows=1', 'rows=5', 'rows=4099', 'plain', 'equal', 'peak', 'neg1e30',
                 'scale=1', 'scale=640^-0.5', 'rows not a multiple of 4']
SOFTMAX_REFUSED = [0, 1025]


def softmax_id(c):
    return 'rows=%d n=%d %s scale=%s' % (c[0], c[1], c[2], '1' if c[3] == 1.0 else '640^-0.5')


def softmax_seams_of(c):
    rows, n, kind, scale = c
    s = {f'n={n}', f'rows={rows}', kind, 'scale=1' if scale == 1.0 else 'scale=640^-0.5'}
    if rows % 4: s.add('rows not a multiple of 4')
    return s


@functools.lru_cache(maxsize=2)
def build_softmax(c):
    """-> x [rows][n] float32.  plain: randn of spread 3 after scaling; equal: one value per row; peak: one entry 90 (after scaling) above a spread of 0.1,
    at n - 1 in row 0 and (37 r) % n in row r: every other term is below e^-87 and the kernel's vm_exp returns exactly 0; neg1e30: every third entry
    near -1e30 (a masked score), the rest plain"""
    rows, n, kind, scale = c
    rng = _rng('softmax', c)
    if kind == 'plain':
        x = rng.standard_normal((rows, n)) * 3 / scale
    elif kind == 'equal':
        x = np.repeat(rng.standard_normal((rows, 1)) * 3 / scale, n, axis=1)
    elif kind == 'peak':
        x = rng.standard_normal((rows, n)) * 0.1 / scale
        for r in range(rows):
            x[r, n - 1 if r == 0 else (37 * r) % n] += 90.0 / scale
    elif kind == 'neg1e30':
        x = rng.standard_normal((rows, n)) * 3 / scale
        x[:, 1::3] = -1e30 * (1 + 0.01 * rng.standard_normal(x[:, 1::3].shape))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# layout copies: (B, C, HW), and the padded widths of each
LAYOUT_CASES = [(B, C, HW) for B in (1, 2) for C in (1, 3, 32, 33) for HW in (1, 255, 4097)]


def layout_pads(C):
    return sorted({p for p in (C, C + 1, 32) if p >= C})


def build_layout(c):
    """arbitrary bit patterns (NaN payloads, subnormals, infinities included): a copy moves bits.  -> uint32 [B][C][HW]"""
    B, C, HW = c
    return _rng('layout', c).integers(0, 1 << 32, (B, C, HW), dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# casts
CAST_NS = (4, 1028)


def _exact32(vals):
    a = np.asarray(vals, np.float64)
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a, equal_nan=True), 'a special value is not an fp32 number'
    return f


def cast_specials(flav):
    """fp32 values at every rounding edge of the 16-bit type: signed zeros; its subnormals (smallest, largest) and the ties between them, 0 and the
    smallest normal; ties between neighbours on both sides of even, at 1 and at -1, and the fp32 neighbours of a tie; the largest finite value, the
    overflow tie (rounds to inf: the even neighbour), its fp32 neighbours on both sides; +-inf; a NaN"""
    p, emin, emax = (10, -14, 15) if flav == 'f16' else (7, -126, 127)
    sub, one = 2.0 ** (emin - p), 2.0 ** -p
    maxfin, tie_over = (2 - one) * 2.0 ** emax, (2 - one / 2) * 2.0 ** emax
    F = np.float32
    nxt = lambda v, to: float(np.nextafter(F(v), F(to)))
    v = [0.0, -0.0, sub, -sub, 3 * sub, 2.0 ** emin - sub, 2.0 ** emin, sub / 2, -sub / 2, 1.5 * sub, 2.5 * sub, nxt(sub / 2, 1), nxt(sub / 2, 0),
         2.0 ** emin - sub / 2, 1 + one / 2, 1 + 3 * one / 2, -(1 + one / 2), -(1 + 3 * one / 2), nxt(1 + one / 2, 2), nxt(1 + one / 2, 0),
         nxt(1 + 3 * one / 2, 2), nxt(1 + 3 * one / 2, 0), maxfin, -maxfin, nxt(tie_over, 0), tie_over, nxt(tie_over, np.inf), -nxt(tie_over, 0), -tie_over,
         -nxt(tie_over, np.inf), np.inf, -np.inf, np.nan, 2.0 ** -149, -(2.0 ** -149), 1.0, -1.0]
    return _exact32(v)


def build_cast_to16(flav, n):
    """-> fp32 [n]: n = 4: -0, a tie, the overflow tie, NaN; else the specials and random values over the type's range"""
    sp = cast_specials(flav)
    if n == 4:
        return sp[[1, 14, 25, 32]].copy()
    rng = _rng('cast', flav, n)
    fill = (rng.standard_normal(n - len(sp)) * 10.0 ** rng.integers(-9, 5, n - len(sp))).astype(np.float32)
    return np.concatenate([sp, fill])


def build_cast_from16(flav, n):
    """-> uint16 [n]: zeros, smallest / largest subnormal, smallest normal, 1, largest finite, +-inf, NaNs; then random patterns"""
    sp = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01] if flav == 'f16' else \
         [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x7F81]
    if n == 4:
        return np.asarray([sp[1], sp[2], sp[7], sp[11]], np.uint16)
    return np.concatenate([np.asarray(sp, np.uint16), _rng('cast16', flav, n).integers(0, 1 << 16, n - len(sp), dtype=np.uint16)])
