// dla.hip — direct logit attribution (VAR.logit_attribution): the final logit of a token, read along one direction of the residual stream.
// VAR's stream is a plain sum (x <- x + gamma1 * proj(att), x <- x + gamma2 * fc2(hid)) and its head is W (LN(x) (1 + s) + sh) + b with an
// affine-free LayerNorm, so with the final token's sigma frozen the logit is linear in every summand of x:
//   r = W[a] - W[b'],  g = r (1 + s),  ghat = (g - mean(g)) / sigma   =>   r . (LN(x) (1 + s) + sh) + b_a - b_b' = ghat . x + konst
// Three kernels, each with a host twin in plain host code below it:
//   k_dla_target     the target of a token from its logits row: the rival (an exact arg-max with gt excluded) and the value z_a - z_b'
//   k_dla_direction  ghat, konst and ghat . x of a token; every sum float64, in an order that depends on C alone
//   k_rowdot_seg     segmented row dots in float64: ghat against a kept stream, u against the attention output per head, ghat gamma1 against a bias
// One wave per token (or per 64 / P segments of a row), no LDS, no barrier, no atomics.  All float64 operations are correctly rounded on both
// sides (adds, multiplies, the division and the square root) and this file is compiled with -ffp-contract=off, so the twins give the kernels' bits.
#include "common.h"
#include "detstats.h"

#define DLA_NONE (1 << 24)          // "no index": indices below 2^24 are exact in fp32 (ln_wave_min_index's trick)

__device__ __forceinline__ int dla_wave_min_index(int i) {
    return (int)-vh_wave_max(-(float)i);
}

// ---- the target ------------------------------------------------------------------------------------------------------------------------
// mode 0: no rival; 1: the rival is the arg-max over v != gt (lowest index on ties); 2: the rival is against[]
template <bool VEC>
__global__ void __launch_bounds__(256) k_dla_target(const float* __restrict__ logits, const int64_t* __restrict__ gt, const int64_t* __restrict__ against,
                                                    int64_t ld_gt, int mode, int64_t rows, int l, int V, int64_t* __restrict__ rival,
                                                    float* __restrict__ value, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t r = w / l;
    const int t = (int)(w - r * l);
    const float* row = logits + w * V;
    const int64_t g = gt[r * ld_gt + t];
    const int64_t bq = mode == 2 ? against[r * ld_gt + t] : -1;
    const bool valid = g >= 0 && g < V && (mode != 2 || (bq >= 0 && bq < V));      // a token outside [0, V) is never dereferenced
    const int gi = valid ? (int)g : -1;
    float best = -INFINITY, nan = 0.f;
    int ibest = DLA_NONE;
    auto take = [&](float x, int v) {
        nan = (x != x) ? 1.f : nan;
        if (v != gi && (ibest == DLA_NONE || x > best)) { best = x; ibest = v; }      // ascending v per lane: the lowest index of a lane's maximum
    };
    if constexpr (VEC) {
        for (int e = 4 * lane; e < V; e += 256) {
            const f32x4 z = *(const f32x4*)(row + e);
            take(z[0], e); take(z[1], e + 1); take(z[2], e + 2); take(z[3], e + 3);
        }
    } else {
        for (int v = lane; v < V; v += 64) take(row[v], v);
    }
    nan = vh_wave_max(nan);
    const float m = vh_wave_max(ibest == DLA_NONE ? -INFINITY : best);      // exact and order-free (no NaN reaches it where the result is used)
    int im = dla_wave_min_index((ibest != DLA_NONE && best == m) ? ibest : DLA_NONE);
    if (lane == 0) {
        const int64_t o = r * ld_out + t;
        int64_t rv = -1;
        float val = NAN;
        if (valid && nan == 0.f) {
            const float za = row[g];
            if (mode == 0) val = za;
            else if (mode == 2) { rv = bq; val = za - row[bq]; }
            else if (im < DLA_NONE) { rv = im; val = za - row[im]; }     // (V == 1: no rival exists, NaN)
        }
        rival[o] = rv;
        value[o] = val;
    }
}

static inline bool dla_target_ok(const void* logits, const void* gt, const void* against, int64_t ld_gt, int mode, int R, int l, int V,
                                 const void* rival, const void* value, int64_t ld_out) {
    if (!logits || !gt || !rival || !value || mode < 0 || mode > 2 || (mode == 2 && !against)) return false;
    return R > 0 && l > 0 && V > 0 && V < DLA_NONE && ld_gt >= l && ld_out >= l;
}

extern "C" int varhip_dla_target_f32(const float* logits, const int64_t* gt, const int64_t* against, int64_t ld_gt, int mode, int R, int l, int V,
                                     int64_t* rival, float* value, int64_t ld_out, varhip_stream_t stream) {
    if (!dla_target_ok(logits, gt, against, ld_gt, mode, R, l, V, rival, value, ld_out)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)R * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    VhScope sc(VH_FAM_OTHER, st, 0, 4.0 * V * (double)rows + 28.0 * rows);
    const dim3 grid((unsigned)blocks);
    if (V % 4 == 0 && (((uintptr_t)logits) & 15) == 0)
        hipLaunchKernelGGL((k_dla_target<true>), grid, dim3(256), 0, st, logits, gt, against, ld_gt, mode, rows, l, V, rival, value, ld_out);
    else
        hipLaunchKernelGGL((k_dla_target<false>), grid, dim3(256), 0, st, logits, gt, against, ld_gt, mode, rows, l, V, rival, value, ld_out);
    return vh_launch_status();
}

extern "C" int varhip_dla_target_host_f32(const float* logits, const int64_t* gt, const int64_t* against, int64_t ld_gt, int mode, int R, int l, int V,
                                          int64_t* rival, float* value, int64_t ld_out) {
    if (!dla_target_ok(logits, gt, against, ld_gt, mode, R, l, V, rival, value, ld_out)) return VARHIP_EINVAL;
    for (int64_t w = 0; w < (int64_t)R * l; ++w) {
        const int64_t r = w / l, t = w - r * l, o = r * ld_out + t;
        const float* row = logits + w * V;
        const int64_t g = gt[r * ld_gt + t];
        const int64_t bq = mode == 2 ? against[r * ld_gt + t] : -1;
        const bool valid = g >= 0 && g < V && (mode != 2 || (bq >= 0 && bq < V));
        bool nan = false;
        int64_t im = -1;
        for (int v = 0; v < V; ++v) {
            nan = nan || row[v] != row[v];
            if (valid && v != g && (im < 0 || row[v] > row[im])) im = v;
        }
        int64_t rv = -1;
        float val = NAN;
        if (valid && !nan) {
            if (mode == 0) val = row[g];
            else if (mode == 2) { rv = bq; val = row[g] - row[bq]; }
            else if (im >= 0) { rv = im; val = row[g] - row[im]; }
        }
        rival[o] = rv;
        value[o] = val;
    }
    return 0;
}

// ---- the direction -------------------------------------------------------------------------------------------------------------------
// g_c of the contract: ((double)W[a][c] - (double)W[b'][c]) * (1.0 + (double)s_c), and r_c beside it
__device__ __host__ __forceinline__ void dla_g(const float* wa, const float* wb, const float* s, int c, double& rc, double& gc) {
    rc = wb ? (double)wa[c] - (double)wb[c] : (double)wa[c];
    gc = rc * (1.0 + (double)s[c]);
}

__global__ void __launch_bounds__(256) k_dla_direction(const float* __restrict__ x, const float* __restrict__ hn_scale, const float* __restrict__ hn_shift,
                                                       int64_t ld_hn, const float* __restrict__ head_w, const float* __restrict__ head_b,
                                                       const int64_t* __restrict__ tok_a, const int64_t* __restrict__ tok_b, int64_t ld_tok,
                                                       int64_t rows, int l, int C, int V, double eps, float* __restrict__ ghat,
                                                       double* __restrict__ konst, double* __restrict__ gx, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t r = w / l;
    const int t = (int)(w - r * l);
    const int64_t a = tok_a[r * ld_tok + t];
    const int64_t b = tok_b ? tok_b[r * ld_tok + t] : 0;
    float* gh = ghat + w * C;
    const int64_t o = r * ld_out + t;
    if (a < 0 || a >= V || b < 0 || b >= V) {                            // never dereferenced: the token's outputs are NaN
        for (int e = 4 * lane; e < C; e += 256) *(f32x4*)(gh + e) = (f32x4)(NAN);
        if (lane == 0) { konst[o] = (double)NAN; gx[o] = (double)NAN; }
        return;
    }
    const float* xr = x + w * C;
    const float* s = hn_scale + r * ld_hn;
    const float* sh = hn_shift + r * ld_hn;
    const float* wa = head_w + a * C;
    const float* wb = tok_b ? head_w + b * C : nullptr;
    double S1 = 0.0, S2 = 0.0, G = 0.0, K = 0.0;
    for (int e = 4 * lane; e < C; e += 256) {
        const f32x4 xv = *(const f32x4*)(xr + e), sv = *(const f32x4*)(s + e), hv = *(const f32x4*)(sh + e), av = *(const f32x4*)(wa + e);
        const f32x4 bv = wb ? *(const f32x4*)(wb + e) : (f32x4)(0.f);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double xd = (double)xv[c];
            const double rc = wb ? (double)av[c] - (double)bv[c] : (double)av[c];
            const double gc = rc * (1.0 + (double)sv[c]);
            S1 = S1 + xd;
            S2 = S2 + xd * xd;
            G = G + gc;
            K = K + rc * (double)hv[c];
        }
    }
    S1 = vh_wave_sum_f64(S1);
    S2 = vh_wave_sum_f64(S2);
    G = vh_wave_sum_f64(G);
    K = vh_wave_sum_f64(K);
    const double mu = S1 / (double)C;
    double var = S2 / (double)C - mu * mu;
    var = var > 0.0 ? var : 0.0;
    const double sigma = sqrt(var + eps);
    const double mg = G / (double)C;
    double X = 0.0;
    for (int e = 4 * lane; e < C; e += 256) {
        const f32x4 xv = *(const f32x4*)(xr + e), sv = *(const f32x4*)(s + e), av = *(const f32x4*)(wa + e);
        const f32x4 bv = wb ? *(const f32x4*)(wb + e) : (f32x4)(0.f);
        f32x4 out;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double rc = wb ? (double)av[c] - (double)bv[c] : (double)av[c];
            const double gc = rc * (1.0 + (double)sv[c]);
            out[c] = (float)((gc - mg) / sigma);
            X = X + (double)out[c] * (double)xv[c];
        }
        *(f32x4*)(gh + e) = out;
    }
    X = vh_wave_sum_f64(X);
    if (lane == 0) {
        konst[o] = K + ((double)head_b[a] - (tok_b ? (double)head_b[b] : 0.0));
        gx[o] = X;
    }
}

static inline bool dla_direction_ok(const void* x, const void* s, const void* sh, int64_t ld_hn, const void* head_w, const void* head_b, const void* tok_a,
                                    int64_t ld_tok, int R, int l, int C, int V, float eps, const void* ghat, const void* konst, const void* gx,
                                    int64_t ld_out) {
    if (!x || !s || !sh || !head_w || !head_b || !tok_a || !ghat || !konst || !gx) return false;
    if (R < 1 || l < 1 || C < 1 || V < 1 || C % 4 != 0 || ld_hn < C || ld_hn % 4 != 0 || ld_tok < l || ld_out < l || !(eps >= 0.f)) return false;
    return ((((uintptr_t)x) | ((uintptr_t)s) | ((uintptr_t)sh) | ((uintptr_t)head_w) | ((uintptr_t)ghat)) & 15) == 0 &&
           ((((uintptr_t)konst) | ((uintptr_t)gx)) & 7) == 0;
}

extern "C" int varhip_dla_direction_f32(const float* x, const float* hn_scale, const float* hn_shift, int64_t ld_hn, const float* head_w,
                                        const float* head_b, const int64_t* tok_a, const int64_t* tok_b, int64_t ld_tok, int R, int l, int C, int V,
                                        float eps, float* ghat, double* konst, double* gx, int64_t ld_out, varhip_stream_t stream) {
    if (!dla_direction_ok(x, hn_scale, hn_shift, ld_hn, head_w, head_b, tok_a, ld_tok, R, l, C, V, eps, ghat, konst, gx, ld_out)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)R * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    VhScope sc(VH_FAM_OTHER, st, 0, 4.0 * C * 6.0 * (double)rows);
    hipLaunchKernelGGL(k_dla_direction, dim3((unsigned)blocks), dim3(256), 0, st, x, hn_scale, hn_shift, ld_hn, head_w, head_b, tok_a, tok_b, ld_tok,
                       rows, l, C, V, (double)eps, ghat, konst, gx, ld_out);
    return vh_launch_status();
}

namespace {
double dla_host_sum_f64(double* p, int P) {                          // the xor butterfly P / 2 .. 1 over P lanes
    for (int off = P >> 1; off >= 1; off >>= 1) {
        double q[64];
        for (int i = 0; i < P; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < P; ++i) p[i] = q[i];
    }
    return p[0];
}
}  // namespace

extern "C" int varhip_dla_direction_host_f32(const float* x, const float* hn_scale, const float* hn_shift, int64_t ld_hn, const float* head_w,
                                             const float* head_b, const int64_t* tok_a, const int64_t* tok_b, int64_t ld_tok, int R, int l, int C,
                                             int V, float eps, float* ghat, double* konst, double* gx, int64_t ld_out) {
    if (!dla_direction_ok(x, hn_scale, hn_shift, ld_hn, head_w, head_b, tok_a, ld_tok, R, l, C, V, eps, ghat, konst, gx, ld_out)) return VARHIP_EINVAL;
    for (int64_t w = 0; w < (int64_t)R * l; ++w) {
        const int64_t r = w / l, t = w - r * l, o = r * ld_out + t;
        const int64_t a = tok_a[r * ld_tok + t];
        const int64_t b = tok_b ? tok_b[r * ld_tok + t] : 0;
        float* gh = ghat + w * C;
        if (a < 0 || a >= V || b < 0 || b >= V) {
            for (int c = 0; c < C; ++c) gh[c] = NAN;
            konst[o] = (double)NAN; gx[o] = (double)NAN;
            continue;
        }
        const float* xr = x + w * C;
        const float* s = hn_scale + r * ld_hn;
        const float* sh = hn_shift + r * ld_hn;
        const float* wa = head_w + a * C;
        const float* wb = tok_b ? head_w + b * C : nullptr;
        double pS1[64], pS2[64], pG[64], pK[64], pX[64];
        for (int lane = 0; lane < 64; ++lane) {
            double S1 = 0.0, S2 = 0.0, G = 0.0, K = 0.0;
            for (int e = 4 * lane; e < C; e += 256)
                for (int c = e; c < e + 4; ++c) {
                    double rc, gc;
                    dla_g(wa, wb, s, c, rc, gc);
                    const double xd = (double)xr[c];
                    S1 = S1 + xd;
                    S2 = S2 + xd * xd;
                    G = G + gc;
                    K = K + rc * (double)sh[c];
                }
            pS1[lane] = S1; pS2[lane] = S2; pG[lane] = G; pK[lane] = K;
        }
        const double S1 = dla_host_sum_f64(pS1, 64), S2 = dla_host_sum_f64(pS2, 64), G = dla_host_sum_f64(pG, 64), K = dla_host_sum_f64(pK, 64);
        const double mu = S1 / (double)C;
        double var = S2 / (double)C - mu * mu;
        var = var > 0.0 ? var : 0.0;
        const double sigma = __builtin_sqrt(var + (double)eps);
        const double mg = G / (double)C;
        for (int lane = 0; lane < 64; ++lane) {
            double X = 0.0;
            for (int e = 4 * lane; e < C; e += 256)
                for (int c = e; c < e + 4; ++c) {
                    double rc, gc;
                    dla_g(wa, wb, s, c, rc, gc);
                    gh[c] = (float)((gc - mg) / sigma);
                    X = X + (double)gh[c] * (double)xr[c];
                }
            pX[lane] = X;
        }
        konst[o] = K + ((double)head_b[a] - (tok_b ? (double)head_b[b] : 0.0));
        gx[o] = dla_host_sum_f64(pX, 64);
    }
    return 0;
}

// ---- segmented row dots --------------------------------------------------------------------------------------------------------------
// the lanes a segment is summed over: the largest power of two <= min(64, q), q = the segment's float4 groups
static inline int dla_seg_lanes(int q) {
    int P = 1;
    while (P * 2 <= q && P < 64) P *= 2;
    return P;
}

__global__ void __launch_bounds__(256) k_rowdot_seg(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int64_t pairs,
                                                    int nseg, int q, int P, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int per = 64 / P;                                              // (row, segment) pairs per wave
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t pair = wave * per + lane / P;
    const int i = lane % P;
    const bool on = pair < pairs;                                        // (a lane past the last pair adds nothing and stores nothing)
    double acc = 0.0;
    if (on) {
        const int64_t m = pair / nseg;
        const int64_t c0 = (pair - m * nseg) * 4 * (int64_t)q;
        const float* ar = a + m * lda + c0;
        const float* br = b + m * ldb + c0;
        for (int k = i; k < q; k += P) {
            const f32x4 av = *(const f32x4*)(ar + 4 * k), bv = *(const f32x4*)(br + 4 * k);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = acc + (double)av[c] * (double)bv[c];
        }
    }
    for (int off = P >> 1; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    if (on && i == 0) out[pair] = acc;
}

static inline bool dla_rowdot_ok(const void* a, int64_t lda, const void* b, int64_t ldb, int M, int C, int nseg, const void* out) {
    if (!a || !b || !out || M < 1 || C < 1 || nseg < 1 || C % nseg != 0 || (C / nseg) % 4 != 0) return false;
    if (lda < C || lda % 4 != 0 || (ldb != 0 && (ldb < C || ldb % 4 != 0))) return false;
    return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0 && (((uintptr_t)out) & 7) == 0;
}

extern "C" int varhip_rowdot_seg_f64(const float* a, int64_t lda, const float* b, int64_t ldb, int M, int C, int nseg, double* out,
                                     varhip_stream_t stream) {
    if (!dla_rowdot_ok(a, lda, b, ldb, M, C, nseg, out)) return VARHIP_EINVAL;
    const int q = C / nseg / 4, P = dla_seg_lanes(q);
    const int64_t pairs = (int64_t)M * nseg;
    const int64_t waves = (pairs + 64 / P - 1) / (64 / P);
    const int64_t blocks = (waves + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    VhScope sc(VH_FAM_OTHER, st, 2.0 * C * (double)M, 4.0 * C * (double)M * (ldb ? 2.0 : 1.0) + 8.0 * pairs);
    hipLaunchKernelGGL(k_rowdot_seg, dim3((unsigned)blocks), dim3(256), 0, st, a, lda, b, ldb, pairs, nseg, q, P, out);
    return vh_launch_status();
}

extern "C" int varhip_rowdot_seg_host_f64(const float* a, int64_t lda, const float* b, int64_t ldb, int M, int C, int nseg, double* out) {
    if (!dla_rowdot_ok(a, lda, b, ldb, M, C, nseg, out)) return VARHIP_EINVAL;
    const int q = C / nseg / 4, P = dla_seg_lanes(q);
    for (int64_t pair = 0; pair < (int64_t)M * nseg; ++pair) {
        const int64_t m = pair / nseg, c0 = (pair - m * nseg) * 4 * (int64_t)q;
        const float* ar = a + m * lda + c0;
        const float* br = b + m * ldb + c0;
        double part[64];
        for (int i = 0; i < P; ++i) {
            double acc = 0.0;
            for (int k = i; k < q; k += P)
                for (int c = 4 * k; c < 4 * k + 4; ++c) acc = acc + (double)ar[c] * (double)br[c];
            part[i] = acc;
        }
        out[pair] = dla_host_sum_f64(part, P);
    }
    return 0;
}
