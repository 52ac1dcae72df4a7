// tokscore.hip — the fork's other teacher-forced class scores (eval_prob.py smooth_bayesian / fast_neighbor_bayesian, var_analysis.py
// l2_dist), reduced from the fp32 logits the head GEMM has just written, with the CFG combine of loglik.hip, and the codebook distance table.
//   p_v = softmax(z)_v, z as in loglik.hip; order: z descending, ties by ascending code index; d: the direct-form distance table
//   mode 1 (group_smoothed, G = param):  r = rank of gt, [lo, hi) = [r - r % G, min(lo + G, V)),  log(sum_{rank in [lo,hi)} p / (hi - lo) + 1e-10)
//   mode 2 (neighbor_max):               max_{v : d(gt, v) <= thr} log p_v
//   mode 3 (expected_distance, k = param): -sum_v p_v d(gt, v)  (k == 0),  else  -sum_{v in top k} p_v d(gt, v) / sum_{v in top k} p_v
// The pass layout, wave mapping, register-held row and the max / exponential sum are those of k_token_loglik.  Rank queries are a bisection
// over the 32 bits of vm_float_key(z): each step counts the row's elements at or above a candidate key (one compare per register, one wave
// sum), so the row stays in registers and no LDS is used.  Elements tied with a queried one are accounted by count (group sums) or resolved by
// a second bisection over code indices (the top-k boundary, where the tied codes have different distances).
#include "common.h"

// ---- distance table: out[v * V + u] = sqrt(sum_c (cb[v][c] - cb[u][c])^2), one fma chain over the channels in channel order —
// the arithmetic of k_neighbor_table (smooth.hip), so every entry equals that table's distance for the same pair bit for bit, the diagonal is 0
// and the table is exactly symmetric ((a - b)^2 and (b - a)^2 are the same float).
__global__ void __launch_bounds__(256) k_code_dist(const float* __restrict__ cb, int V, int D, float* __restrict__ out) {
    const int u = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (u >= V) return;
    const float* a = cb + (int64_t)v * D;
    const float* b = cb + (int64_t)u * D;
    float acc = 0.f;
    for (int c = 0; c < D; ++c) { const float d = a[c] - b[c]; acc = __builtin_fmaf(d, d, acc); }
    out[(int64_t)v * V + u] = vm_sqrt(acc);
}

extern "C" int varhip_code_dist_f32(const float* codebook, int V, int D, float* out, varhip_stream_t stream) {
    if (!codebook || !out || V <= 0 || V > 65535 || D <= 0) return VARHIP_EINVAL;
    VhScope sc(VH_FAM_OTHER, (hipStream_t)stream, 3.0 * V * (double)V * D, 4.0 * V * (double)V);
    hipLaunchKernelGGL(k_code_dist, dim3((V + 255) / 256, V), dim3(256), 0, (hipStream_t)stream, codebook, V, D, out);
    return vh_launch_status();
}

template <bool CFG>
__device__ __forceinline__ float ts_z(const float* lc, const float* lu, int64_t v, float ca, float cb) {
    if (!CFG) return lc[v];
    const float a = ca * lc[v];
    const float b = cb * lu[v];
    return a - b;
}

// the float whose vm_float_key is k (keys below that of -inf map to -inf: every element of a row is at or above it; keys above that of
// +inf map to NaN: no element compares >= it)
__device__ __forceinline__ float ts_key_float(unsigned k) {
    if (k <= 0x007fffffu) return -INFINITY;
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One row as NV float4 registers per lane (element j * 256 + 4 * lane + c; NV == 0: the row is re-read from memory at every visit)
template <int NV, bool CFG>
struct TsRow {
    f32x4 z[NV > 0 ? NV : 1];
    const float *lc, *lu;
    float ca, cb;
    int V, lane;
    // fills z (NV > 0) and gives the row's max m and exponential sum s (every lane gets them): statement for statement the row pass of
    // k_token_score below, which keeps its own inline copy so that its instantiations compile to what they were before this member existed
    __device__ __forceinline__ void load_max_sum(float& m, float& s) {
        m = -INFINITY; s = 0.f;
        if constexpr (NV > 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int e = j * 256 + 4 * lane;
                if (e < V) {
                    const f32x4 c = *(const f32x4*)(lc + e);
                    if constexpr (CFG) { const f32x4 u = *(const f32x4*)(lu + e); const f32x4 a = ca * c; const f32x4 b = cb * u; z[j] = a - b; }
                    else z[j] = c;
                } else {
                    z[j] = (f32x4)(-INFINITY);
                }
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(z[j][0], z[j][1]), fmaxf(z[j][2], z[j][3])));
            m = vh_wave_max(m);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f32x2 e0 = vh_exp_pair(f32x2{z[j][0] - m, z[j][1] - m});
                const f32x2 e1 = vh_exp_pair(f32x2{z[j][2] - m, z[j][3] - m});
                s = ((s + e0[0]) + e0[1]) + (e1[0] + e1[1]);
            }
        } else {
            for (int v = lane; v < V; v += 64) m = fmaxf(m, ts_z<CFG>(lc, lu, v, ca, cb));
            m = vh_wave_max(m);
            for (int v = lane; v < V; v += 64) s = s + vm_exp(ts_z<CFG>(lc, lu, v, ca, cb) - m);
        }
        s = vh_wave_sum(s);
    }
    // f(z_v, v) for every element v of this lane
    template <typename F> __device__ __forceinline__ void each(F f) const {
        if constexpr (NV > 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int e = j * 256 + 4 * lane;
                if (e < V) { f(z[j][0], e); f(z[j][1], e + 1); f(z[j][2], e + 2); f(z[j][3], e + 3); }
            }
        } else {
            for (int v = lane; v < V; v += 64) f(ts_z<CFG>(lc, lu, v, ca, cb), v);
        }
    }
    // f(z_v, d_v, v) with d_v = drow[v]; the NV path reads drow with the row's own float4 layout (16-byte aligned rows)
    template <typename F> __device__ __forceinline__ void each_d(const float* __restrict__ drow, F f) const {
        if constexpr (NV > 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int e = j * 256 + 4 * lane;
                if (e < V) {
                    const f32x4 d = *(const f32x4*)(drow + e);
                    f(z[j][0], d[0], e); f(z[j][1], d[1], e + 1); f(z[j][2], d[2], e + 2); f(z[j][3], d[3], e + 3);
                }
            }
        } else {
            for (int v = lane; v < V; v += 64) f(ts_z<CFG>(lc, lu, v, ca, cb), drow[v], v);
        }
    }
    // number of elements of the row with z >= t (every lane gets it; exact: counts < 2^24 are exact in fp32)
    __device__ __forceinline__ int count_ge(float t) const {
        int n = 0;
        each([&](float x, int) { n += x >= t ? 1 : 0; });
        return (int)vh_wave_sum((float)n);
    }
    __device__ __forceinline__ int count_gt(float t) const {
        int n = 0;
        each([&](float x, int) { n += x > t ? 1 : 0; });
        return (int)vh_wave_sum((float)n);
    }
    // the value at rank q (0-based) under z descending: the largest key K with count(key >= K) > q, built from the top bit down
    __device__ __forceinline__ float at_rank(int q) const {
        unsigned K = 0;
#pragma nounroll
        for (int b = 31; b >= 0; --b) {
            const unsigned cand = K | (1u << b);
            if (count_ge(ts_key_float(cand)) > q) K = cand;
        }
        return ts_key_float(K);
    }
};

template <int NV, bool CFG, int MODE>
__global__ void __launch_bounds__(256) k_token_score(const float* __restrict__ logits, const int64_t* __restrict__ gt, int64_t ld_gt,
                                                     int images, int classes, int l, int V, float ca, float cb, int param, float thr,
                                                     const float* __restrict__ dist, int64_t ld_dist,
                                                     float* __restrict__ out, int64_t ld_oi, int64_t ld_oc) {
    const int lane = threadIdx.x & 63;
    // wave w scores (image, token, class) in that order, as k_token_loglik
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t per_img = (int64_t)l * classes;
    if (w >= per_img * images) return;                                  // (wave-uniform)
    const int img = (int)(w / per_img);
    const int t = (int)((w - img * per_img) / classes);
    const int k = (int)(w - img * per_img - (int64_t)t * classes);
    float* o = out + (int64_t)img * ld_oi + (int64_t)k * ld_oc + t;
    const int64_t g = gt[(int64_t)img * ld_gt + t];                     // every lane reads it: wave-uniform
    if (g < 0 || g >= V) {                                              // never read: scores NaN (the host API rejects such tokens)
        if (lane == 0) *o = NAN;
        return;
    }
    TsRow<NV, CFG> row;
    row.lc = logits + (((int64_t)img * classes + k) * l + t) * V;
    row.lu = logits + (((int64_t)images * classes + img) * l + t) * V;  // unconditional rows follow the class rows
    row.ca = ca; row.cb = cb; row.V = V; row.lane = lane;
    // max and exponential sum: the operations and order of k_token_loglik
    float m = -INFINITY, s = 0.f;
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int e = j * 256 + 4 * lane;
            if (e < V) {
                const f32x4 c = *(const f32x4*)(row.lc + e);
                if constexpr (CFG) { const f32x4 u = *(const f32x4*)(row.lu + e); const f32x4 a = ca * c; const f32x4 b = cb * u; row.z[j] = a - b; }
                else row.z[j] = c;
            } else {
                row.z[j] = (f32x4)(-INFINITY);
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(row.z[j][0], row.z[j][1]), fmaxf(row.z[j][2], row.z[j][3])));
        m = vh_wave_max(m);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const f32x2 e0 = vh_exp_pair(f32x2{row.z[j][0] - m, row.z[j][1] - m});
            const f32x2 e1 = vh_exp_pair(f32x2{row.z[j][2] - m, row.z[j][3] - m});
            s = ((s + e0[0]) + e0[1]) + (e1[0] + e1[1]);
        }
    } else {
        for (int v = lane; v < V; v += 64) m = fmaxf(m, ts_z<CFG>(row.lc, row.lu, v, ca, cb));
        m = vh_wave_max(m);
        for (int v = lane; v < V; v += 64) s = s + vm_exp(ts_z<CFG>(row.lc, row.lu, v, ca, cb) - m);
    }
    s = vh_wave_sum(s);
    // the selection stages below use m through a scalar register: the compiler then cannot keep the 4 * NV values z - m (or their exponentials)
    // of the sum above alive across the bisection loops, which would double the row's register footprint
    m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    float res;
    if constexpr (MODE == 1) {
        const int G = param;
        const float zg = ts_z<CFG>(row.lc, row.lu, g, ca, cb);
        int n = 0;                                                      // rank of gt: larger z, or equal z at a smaller index
        const int gi = (int)g;
        row.each([&](float x, int v) { n += (x > zg || (x == zg && v < gi)) ? 1 : 0; });
        const int r = (int)vh_wave_sum((float)n);
        const int lo = r - r % G, hi = min(lo + G, V);
        // the band's multiset of values: the value at rank lo (zl, ranks [gtl, gel) hold it), the one at rank hi - 1 (zh), everything strictly
        // between them once, the tied ones by count.  Summed directly (never as the difference of two prefix sums).
        const float zl = (lo == r) ? zg : row.at_rank(lo);
        const int gel = row.count_ge(zl);
        float band;
        if (hi <= gel) {
            band = (float)(hi - lo) * vm_exp(zl - m);
        } else {
            const float zh = row.at_rank(hi - 1);
            const int gth = row.count_gt(zh);
            float b = 0.f;
            row.each([&](float x, int) { if (x > zh && x < zl) b = b + vm_exp(x - m); });
            b = vh_wave_sum(b);
            band = (b + (float)(gel - lo) * vm_exp(zl - m)) + (float)(hi - gth) * vm_exp(zh - m);
        }
        res = vm_log((band / s) / (float)(hi - lo) + 1e-10f);
    } else if constexpr (MODE == 2) {
        const float* drow = dist + g * ld_dist;
        float best = -INFINITY;
        row.each_d(drow, [&](float x, float d, int) { if (d <= thr) best = fmaxf(best, x); });
        best = vh_wave_max(best);
        res = (best - m) - vm_log(s);                                   // = k_token_loglik's value when the set is {gt}
    } else {
        const float* drow = dist + g * ld_dist;
        float num = 0.f, den;
        if (param == 0) {
            row.each_d(drow, [&](float x, float d, int) { num = num + vm_exp(x - m) * d; });
            den = s;
        } else {
            // the top-k set: z above the value at rank k - 1 (zt), and the first `need` codes by index among those equal to zt
            const float zt = row.at_rank(param - 1);
            const int gtt = row.count_gt(zt), get = row.count_ge(zt), need = param - gtt;
            int it = V;                                                 // codes equal to zt with index < it are in
            if (get - gtt > need) {                                     // the boundary splits a tie: smallest i with #{z == zt, v <= i} >= need
                int a = 0, b = V - 1;
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    int n = 0;
                    row.each([&](float x, int v) { n += (x == zt && v <= mid) ? 1 : 0; });
                    if ((int)vh_wave_sum((float)n) >= need) b = mid; else a = mid + 1;
                }
                it = a + 1;
            }
            den = 0.f;
            row.each_d(drow, [&](float x, float d, int v) {
                if (x > zt || (x == zt && v < it)) { const float e = vm_exp(x - m); num = num + e * d; den = den + e; }
            });
            den = vh_wave_sum(den);
        }
        num = vh_wave_sum(num);
        res = -(num / den);
    }
    if (lane == 0) *o = res;
}

template <int NV, int MODE>
static void ts_launch(bool cfg, dim3 grid, hipStream_t st, const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l,
                      int V, float ca, float cb, int param, float thr, const float* dist, int64_t ld_dist, float* out, int64_t ld_oi, int64_t ld_oc) {
    if (cfg) hipLaunchKernelGGL((k_token_score<NV, true, MODE>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb,
                                param, thr, dist, ld_dist, out, ld_oi, ld_oc);
    else hipLaunchKernelGGL((k_token_score<NV, false, MODE>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb,
                            param, thr, dist, ld_dist, out, ld_oi, ld_oc);
}

template <int MODE>
static void ts_dispatch(bool vec, bool cfg, dim3 grid, hipStream_t st, const float* logits, const int64_t* gt, int64_t ld_gt, int images,
                        int classes, int l, int V, float ca, float cb, int param, float thr, const float* dist, int64_t ld_dist, float* out,
                        int64_t ld_oi, int64_t ld_oc) {
    if (vec && V <= 1024) ts_launch<4, MODE>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_oi, ld_oc);
    else if (vec && V <= 4096) ts_launch<16, MODE>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_oi, ld_oc);
    else ts_launch<0, MODE>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_oi, ld_oc);
}

extern "C" int varhip_token_score_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                                      int with_uncond, float ca, float cb, int mode, int param, float thr, const float* dist, int64_t ld_dist,
                                      float* out, int64_t ld_out_img, int64_t ld_out_cls, varhip_stream_t stream) {
    if (!logits || !gt || !out || images <= 0 || classes <= 0 || l <= 0 || V <= 0 || V > (1 << 24) || ld_gt < l || ld_out_cls < l ||
        ld_out_img < (int64_t)classes * ld_out_cls)
        return VARHIP_EINVAL;
    if (mode == 1) {
        if (param < 1) return VARHIP_EINVAL;
    } else if (mode == 2 || mode == 3) {
        if (!dist || ld_dist < V) return VARHIP_EINVAL;
        if (mode == 2 && !(thr >= 0.f && thr <= 3.40282347e38f)) return VARHIP_EINVAL;      // finite, >= 0 (NaN fails both)
        if (mode == 3 && (param < 0 || param > V)) return VARHIP_EINVAL;
    } else {
        return VARHIP_EINVAL;
    }
    const int64_t rows = (int64_t)images * classes * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const bool dvec = mode == 1 || (((uintptr_t)dist & 15) == 0 && ld_dist % 4 == 0);
    const bool vec = V % 4 == 0 && ((uintptr_t)logits & 15) == 0 && dvec;
    // bytes: as varhip_token_loglik_f32, plus one distance-table row per scored row in the distance modes
    const double bytes = 4.0 * V * (double)(rows + (with_uncond ? (int64_t)images * l : 0) + (mode != 1 ? rows : 0)) + 12.0 * rows;
    VhScope sc(VH_FAM_SAMPLER, st, 0, bytes);
    const dim3 grid((unsigned)blocks);
    const bool cfg = with_uncond != 0;
    if (mode == 1) ts_dispatch<1>(vec, cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_out_img, ld_out_cls);
    else if (mode == 2) ts_dispatch<2>(vec, cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_out_img, ld_out_cls);
    else ts_dispatch<3>(vec, cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, param, thr, dist, ld_dist, out, ld_out_img, ld_out_cls);
    return vh_launch_status();
}

// ---- distance-probability profile (VAR.distance_profile; fork var_analysis.py:352-425 plot_dist_kde's (distance, probability) pairs, binned
// at :694-732 / :798-818) ---------------------------------------------------------------------------------------------------------------------
// Per element v of a scored row: p_v = vm_exp(z_v - m) / s (m, s: TsRow::load_max_sum, the row pass of k_token_score; the exponential and the
// denominator are those of mode 3 with param == 0, which divides its sum of vm_exp(z_v - m) * d_v by s: here each term is divided, one correctly
// rounded fp32 division), d_v = dist[gt][v]; bin b iff edges[b] <= d_v < edges[b + 1] and p_v > min_prob (fp32 compares: a NaN is in no bin).
// A workgroup owns one (image, class) and DP_CHUNK consecutive tokens of the scale, its four waves take them in turn (a wave without a token
// only meets the barriers).  Edges and one histogram (uint32 counts, uint64 fixed-point mass) live in LDS; every element costs a binary search
// over the edges and two LDS integer atomics; after the barrier the non-zero bins go out as 64-bit global integer atomics.  Integer sums only:
// the result does not depend on the order of execution.
#define DP_CHUNK 8
#define DP_MAXBINS 256

template <int NV, bool CFG>
__global__ void __launch_bounds__(256) k_dist_profile(const float* __restrict__ logits, const int64_t* __restrict__ gt, int64_t ld_gt,
                                                      int images, int classes, int l, int V, float ca, float cb,
                                                      const float* __restrict__ dist, int64_t ld_dist, const float* __restrict__ edges,
                                                      int nbins, int top, float min_prob, unsigned long long* __restrict__ mass_q,
                                                      unsigned long long* __restrict__ count, int64_t ld_img, int64_t ld_cls) {
    __shared__ float s_edge[DP_MAXBINS + 1];
    __shared__ unsigned s_cnt[DP_MAXBINS];
    __shared__ unsigned long long s_mass[DP_MAXBINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = (l + DP_CHUNK - 1) / DP_CHUNK;
    // workgroup -> (image, class, chunk), the chunk fastest
    const int64_t ic = blockIdx.x / chunks;
    const int t0 = (int)(blockIdx.x - ic * chunks) * DP_CHUNK;
    const int img = (int)(ic / classes), k = (int)(ic - (int64_t)img * classes);
    const int ne = nbins + 1;
    for (int i = threadIdx.x; i < ne; i += 256) s_edge[i] = edges[i];
    for (int i = threadIdx.x; i < nbins; i += 256) { s_cnt[i] = 0u; s_mass[i] = 0ull; }
    __syncthreads();
    const int t1 = min(t0 + DP_CHUNK, l);
    for (int t = t0 + wave; t < t1; t += 4) {                               // (wave-uniform)
        const int64_t g = gt[(int64_t)img * ld_gt + t];
        if (g < 0 || g >= V) continue;                                      // never dereferenced, contributes nothing (the host API rejects it)
        TsRow<NV, CFG> row;
        row.lc = logits + (((int64_t)img * classes + k) * l + t) * V;
        row.lu = logits + (((int64_t)images * classes + img) * l + t) * V;
        row.ca = ca; row.cb = cb; row.V = V; row.lane = lane;
        float m, s;
        row.load_max_sum(m, s);
        m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));     // as k_token_score: no second copy of the row kept alive
        row.each_d(dist + g * ld_dist, [&](float x, float d, int) {
            const float p = vm_exp(x - m) / s;
            // pos = |{i : edges[i] <= d}| by binary search (edges ascending; `top` = the largest power of two <= ne); a NaN d leaves pos = 0
            int pos = 0;
            for (int step = top; step > 0; step >>= 1) {
                const int c = pos + step;
                if (c <= ne && s_edge[c - 1] <= d) pos = c;
            }
            if (pos >= 1 && pos <= nbins && p > min_prob) {                 // pos == ne: d at or above the last edge
                atomicAdd(&s_cnt[pos - 1], 1u);
                atomicAdd(&s_mass[pos - 1], (unsigned long long)__double2ll_rn((double)p * 281474976710656.0));     // rint(p * 2^48)
            }
        });
    }
    __syncthreads();
    unsigned long long* mo = mass_q + (int64_t)img * ld_img + (int64_t)k * ld_cls;
    unsigned long long* co = count + (int64_t)img * ld_img + (int64_t)k * ld_cls;
    for (int i = threadIdx.x; i < nbins; i += 256) {
        const unsigned c = s_cnt[i];
        if (c) {
            atomicAdd(co + i, (unsigned long long)c);
            const unsigned long long q = s_mass[i];
            if (q) atomicAdd(mo + i, q);
        }
    }
}

template <int NV>
static void dp_launch(bool cfg, dim3 grid, hipStream_t st, const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l,
                      int V, float ca, float cb, const float* dist, int64_t ld_dist, const float* edges, int nbins, int top, float min_prob,
                      int64_t* mass_q, int64_t* count, int64_t ld_img, int64_t ld_cls) {
    if (cfg) hipLaunchKernelGGL((k_dist_profile<NV, true>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, dist, ld_dist,
                                edges, nbins, top, min_prob, (unsigned long long*)mass_q, (unsigned long long*)count, ld_img, ld_cls);
    else hipLaunchKernelGGL((k_dist_profile<NV, false>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, dist, ld_dist,
                            edges, nbins, top, min_prob, (unsigned long long*)mass_q, (unsigned long long*)count, ld_img, ld_cls);
}

extern "C" int varhip_dist_profile_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                                       int with_uncond, float ca, float cb, const float* dist, int64_t ld_dist,
                                       const float* edges, int nbins, float min_prob,
                                       int64_t* mass_q, int64_t* count, int64_t ld_img, int64_t ld_cls, varhip_stream_t stream) {
    if (!logits || !gt || !dist || !edges || !mass_q || !count || images <= 0 || classes <= 0 || l <= 0 || V <= 0 || V > (1 << 24) ||
        nbins < 1 || nbins > DP_MAXBINS || ld_gt < l || ld_dist < V || ld_cls < nbins || ld_img < (int64_t)classes * ld_cls ||
        !(min_prob >= 0.f && min_prob < 1.f))                               // (NaN fails both)
        return VARHIP_EINVAL;
    const int64_t rows = (int64_t)images * classes * l;
    const int64_t blocks = (int64_t)images * classes * ((l + DP_CHUNK - 1) / DP_CHUNK);
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    int top = 1;
    while (top * 2 <= nbins + 1) top *= 2;
    const hipStream_t st = (hipStream_t)stream;
    // the alignment conditions of varhip_token_score_f32's distance modes
    const bool vec = V % 4 == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)dist & 15) == 0 && ld_dist % 4 == 0;
    // bytes: as varhip_token_score_f32's mode 3 (the rows, the uncond rows, one distance-table row per scored row)
    const double bytes = 4.0 * V * (double)(2 * rows + (with_uncond ? (int64_t)images * l : 0)) + 8.0 * rows;
    VhScope sc(VH_FAM_SAMPLER, st, 0, bytes);
    const dim3 grid((unsigned)blocks);
    const bool cfg = with_uncond != 0;
    if (vec && V <= 1024) dp_launch<4>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, dist, ld_dist, edges, nbins, top, min_prob, mass_q, count, ld_img, ld_cls);
    else if (vec && V <= 4096) dp_launch<16>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, dist, ld_dist, edges, nbins, top, min_prob, mass_q, count, ld_img, ld_cls);
    else dp_launch<0>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, dist, ld_dist, edges, nbins, top, min_prob, mass_q, count, ld_img, ld_cls);
    return vh_launch_status();
}
