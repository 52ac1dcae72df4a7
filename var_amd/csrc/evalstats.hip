// evalstats.hip — the validation metrics of the trainer (reference trainer.py:54-84 eval_ep, :126-156 the logging block), reduced from the
// fp32 logits the head GEMM has just written: per token the negative log-likelihood, the label-smoothing term, the argmax and the rank of
// the ground-truth token; per call the per-scale sums, the count of correct tokens and the histogram of the predictions.
//   nll    = -((z_gt - max z) - log(sum_v exp(z_v - max z)))     the value of k_token_loglik (rowlse.h: one piece of code), negated
//   pred   = lowest index of max z (+0 == -0); a row holding a NaN: its lowest NaN index              (torch.argmax, k_cfg_argmax's rule)
//   rank   = |{v : z_v > z_gt or (z_v == z_gt and v < gt)}|                                          (k_token_score's total order)
//   smooth = (float)((double)z_gt - sum / V), sum = sum_v (double)z_v                                (CE(label_smoothing=e) = nll + e * smooth)
// k_token_eval is a streaming row reduction with the structure of k_token_loglik: one wave per row, four rows per 256-thread workgroup, no
// LDS and no barrier; where the row fits (V <= 4096, V % 4 == 0, 16-byte aligned rows) it is read once into registers and every
// reduction runs over that one copy.
// The float64 sum of a row has ONE order that depends on V alone: lane i adds its elements j * 256 + 4 * i + c in ascending (j, c) order
// (the register layout; the scalar path walks the same elements in the same order), the 64 lanes by the xor butterfly of detstats.h.
#include "common.h"
#include "rowlse.h"
#include "detstats.h"

#define EV_MAX_SCALES 32

// f(z_v, v) for every element of this lane, ascending in v; the same elements in the same order on both paths
template <int NV, typename F>
__device__ __forceinline__ void ev_each(const f32x4* z, const float* row, int V, int lane, F f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int e = j * 256 + 4 * lane;
            if (e < V) { f(z[j][0], e); f(z[j][1], e + 1); f(z[j][2], e + 2); f(z[j][3], e + 3); }
        }
    } else {
        for (int e = 4 * lane; e < V; e += 256)
            for (int c = 0; c < 4 && e + c < V; ++c) f(row[e + c], e + c);
    }
}

// smallest of the lanes' indices (exact: indices < 2^24 are exact in fp32); a lane without one passes `none` > every index
__device__ __forceinline__ int ev_wave_min_index(int i) {
    return (int)-vh_wave_max(-(float)i);
}

template <int NV>
__global__ void __launch_bounds__(256) k_token_eval(const float* __restrict__ logits, const int64_t* __restrict__ gt, int64_t ld_gt,
                                                    int64_t rows, int l, int V, float* __restrict__ nll, float* __restrict__ smooth,
                                                    int64_t* __restrict__ pred, int32_t* __restrict__ rank, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // row w = r * l + t of the pass
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t r = w / l;
    const int t = (int)(w - r * l);
    const float* row = logits + w * V;
    // z_gt first, one address for the whole wave (a broadcast load): every reduction below then runs in the one pass over the registers
    const int64_t g = gt[r * ld_gt + t];
    const bool valid = g >= 0 && g < V;                                 // a token outside [0, V) is never dereferenced
    const float zg = valid ? row[g] : NAN;
    const int gi = (int)g;
    f32x4 z[NV > 0 ? NV : 1];
    float m, s;
    if constexpr (NV > 0) {
        vh_row_load<NV, false>(z, row, row, 1.f, 0.f, V, lane);
        vh_row_max_expsum<NV>(z, m, s);
    } else {
        vh_row_max_expsum_mem<false>(row, row, 1.f, 0.f, V, lane, m, s);
    }
    s = vh_wave_sum(s);
    // (m through a scalar register: the compiler then cannot keep the 4 * NV values z - m of the sum above alive across the pass below)
    m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    const int none = 1 << 24;
    int n = 0, imax = none, inan = none;
    double acc = 0.0;
    ev_each<NV>(z, row, V, lane, [&](float x, int v) {
        n += (x > zg || (x == zg && v < gi)) ? 1 : 0;
        imax = (x == m && v < imax) ? v : imax;
        inan = (x != x && v < inan) ? v : inan;
        acc = acc + (double)x;
    });
    const int rk = (int)vh_wave_sum((float)n);                          // exact: counts < 2^24 are exact in fp32
    imax = ev_wave_min_index(imax);
    inan = ev_wave_min_index(inan);
    acc = vh_wave_sum_f64(acc);
    if (lane == 0) {
        const int64_t o = r * ld_out + t;
        const double mean = acc / (double)V;
        nll[o] = valid ? -vh_row_logp(zg, m, s) : NAN;
        smooth[o] = valid ? (float)((double)zg - mean) : NAN;
        pred[o] = inan < none ? inan : (imax < none ? imax : 0);
        rank[o] = valid ? rk : -1;
    }
}

extern "C" int varhip_token_eval_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V, float* nll, float* smooth,
                                     int64_t* pred, int32_t* rank, int64_t ld_out, varhip_stream_t stream) {
    if (!logits || !gt || !nll || !smooth || !pred || !rank || R <= 0 || l <= 0 || V <= 0 || V >= (1 << 24) || ld_gt < l || ld_out < l)
        return VARHIP_EINVAL;
    const int64_t rows = (int64_t)R * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && ((uintptr_t)logits & 15) == 0;
    VhScope sc(VH_FAM_SAMPLER, st, 0, 4.0 * V * (double)rows + 28.0 * rows);
    const dim3 grid((unsigned)blocks);
    if (vec && V <= 1024) hipLaunchKernelGGL((k_token_eval<4>), grid, dim3(256), 0, st, logits, gt, ld_gt, rows, l, V, nll, smooth, pred, rank, ld_out);
    else if (vec && V <= 4096) hipLaunchKernelGGL((k_token_eval<16>), grid, dim3(256), 0, st, logits, gt, ld_gt, rows, l, V, nll, smooth, pred, rank, ld_out);
    else hipLaunchKernelGGL((k_token_eval<0>), grid, dim3(256), 0, st, logits, gt, ld_gt, rows, l, V, nll, smooth, pred, rank, ld_out);
    return vh_launch_status();
}

// ---- per call: the per-scale sums and the histogram of the predictions ----------------------------------------------------------------------
struct EvScales { int S; int begin[EV_MAX_SCALES + 1]; };

// blocks [0, S): block s adds scale s (tokens [begin[s], begin[s + 1]) of every image): element i = image * l + token, thread t of 256 adds the
// elements t, t + 256, ... in ascending order in float64, then the butterfly and the four waves in order (detstats.h): an order that depends on
// (N, l) alone.  blocks [S, S + GH): 1024 predictions each into the histogram.
__global__ void __launch_bounds__(256) k_eval_reduce(const float* __restrict__ nll, const float* __restrict__ smooth, const int64_t* __restrict__ pred,
                                                     const int32_t* __restrict__ rank, int64_t ld, int N, EvScales sc, int V,
                                                     double* __restrict__ nll_S, double* __restrict__ smooth_S, long long* __restrict__ correct_S,
                                                     unsigned long long* __restrict__ hist) {
    __shared__ double red[4];
    __shared__ unsigned long long cnt;
    __shared__ unsigned int bins[VH_HIST_LDS_BINS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < sc.S) {                                        // (uniform per block: the barriers inside are safe)
        const int b = sc.begin[blockIdx.x], l = sc.begin[blockIdx.x + 1] - b;
        const int64_t n = (int64_t)N * l;
        if (tid == 0) cnt = 0ull;
        double a = 0.0, e = 0.0;
        unsigned long long c = 0ull;
        for (int64_t i = tid; i < n; i += 256) {
            const int64_t img = i / l;
            const int64_t o = img * ld + b + (i - img * l);
            a = a + (double)nll[o];
            e = e + (double)smooth[o];
            c += rank[o] == 0 ? 1ull : 0ull;                             // (an out-of-range gt has rank -1: never correct)
        }
        a = vh_block_sum256_f64(a, red);
        e = vh_block_sum256_f64(e, red);
        if (c) atomicAdd(&cnt, c);                                       // integer, LDS: exact in any order
        __syncthreads();
        if (tid == 0) { nll_S[blockIdx.x] = a; smooth_S[blockIdx.x] = e; correct_S[blockIdx.x] = (long long)cnt; }
    } else {
        const int L = sc.begin[sc.S];
        const int64_t i0 = (int64_t)(blockIdx.x - sc.S) * 1024;
        vh_hist_block1024([&](int64_t i) { const int64_t img = i / L; return pred[img * ld + (i - img * L)]; }, i0, (int64_t)N * L, V, hist, bins);
    }
}

extern "C" int varhip_eval_reduce_f32(const float* nll, const float* smooth, const int64_t* pred, const int32_t* rank, int64_t ld, int N,
                                      const int32_t* begin_S1, int S, int V, double* nll_S, double* smooth_S, int64_t* correct_S,
                                      int64_t* pred_hist_V, varhip_stream_t stream) {
    if (!nll || !smooth || !pred || !rank || !begin_S1 || !nll_S || !smooth_S || !correct_S || !pred_hist_V || N <= 0 || S < 1 ||
        S > EV_MAX_SCALES || V <= 0 || begin_S1[0] != 0)
        return VARHIP_EINVAL;
    EvScales sc;
    sc.S = S;
    for (int i = 0; i <= EV_MAX_SCALES; ++i) sc.begin[i] = 0;
    for (int i = 0; i <= S; ++i) {
        if (i > 0 && begin_S1[i] <= begin_S1[i - 1]) return VARHIP_EINVAL;
        sc.begin[i] = begin_S1[i];
    }
    const int64_t L = sc.begin[S], n = (int64_t)N * L;
    if (ld < L || n > (int64_t)1024 * 65536) return VARHIP_EINVAL;
    const int GH = (int)((n + 1023) / 1024);
    VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 2.0 * (double)n, 20.0 * (double)n);
    hipLaunchKernelGGL(k_eval_reduce, dim3(S + GH), dim3(256), 0, (hipStream_t)stream, nll, smooth, pred, rank, ld, N, sc, V, nll_S, smooth_S,
                       (long long*)correct_S, (unsigned long long*)pred_hist_V);
    return vh_launch_status();
}
