// generative.hip — the two kernels of generative zero-shot classification (VAR.classify_generative, reference eval_prob.py:466-516).
//
// varhip_cfg_argmax_f32: greedy CFG token selection, what var.inpainting(top_k=1, top_p=0) reduces to on rows without an exact tie.
//   One 256-thread workgroup per (image, token) row.  z = (1+t)*cond - t*uncond with the three roundings of cfg_sample_f32, then the first
//   maximum of z (lowest index among equal maxima; +0 and -0 are equal).  NaN rule: a row holding a NaN selects its lowest NaN index, as
//   torch.argmax does.  A row whose keep flag is set writes its given token and reads no logits (the torch.where of var.py:326-328, fork,
//   fused: no token_select_i64 launch behind it).  No Exp(1) noise, no top-k select.
// varhip_feature_l1_f32: score[r] = -mean_d |f_in[img[r]][d] - f_rec[r][d]| in one fixed order: thread t of the row's workgroup sums
//   d = t, t + 256, ... in float64, the 256 partials are added by a fixed tree, and the float64 sum / D is rounded once to fp32.
#include "common.h"

#define GA_THREADS 256

// is (cv, ci, cn) better than (av, ai, an)?  NaN beats a number, then larger value, then lower index
__device__ __forceinline__ bool ga_better(float av, int ai, int an, float cv, int ci, int cn) {
    if (ci < 0) return false;
    if (ai < 0) return true;
    if (an != cn) return cn != 0;
    if (!an && cv != av) return cv > av;
    return ci < ai;
}

__global__ void __launch_bounds__(GA_THREADS) k_cfg_argmax(const float* __restrict__ logits, const uint8_t* __restrict__ keep,
                                                           const int64_t* __restrict__ gt, int64_t ld_keep, int64_t* __restrict__ idx_out,
                                                           int64_t rows, int l, int V, float ca, float cb) {
    __shared__ float s_bv[GA_THREADS / 64];
    __shared__ int s_bi[GA_THREADS / 64], s_bn[GA_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (keep) {
        const int64_t b = row / l, j = row - b * l;
        if (keep[b * ld_keep + j]) {                       // uniform over the workgroup: no barrier is skipped by some threads only
            if (tid == 0) idx_out[row] = gt[b * ld_keep + j];
            return;
        }
    }
    const float* lc = logits + row * V;
    const float* lu = logits + (rows + row) * V;
    float bv = 0.f; int bi = -1, bn = 0;
    for (int i = tid; i < V; i += GA_THREADS) {            // ascending per thread: a later equal value never replaces an earlier one
        const float a = ca * lc[i];
        const float c = cb * lu[i];
        const float z = a - c;
        const int isn = (z != z);
        if (ga_better(bv, bi, bn, z, i, isn)) { bv = z; bi = i; bn = isn; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64); const int oi = __shfl_xor(bi, off, 64); const int on = __shfl_xor(bn, off, 64);
        if (ga_better(bv, bi, bn, ov, oi, on)) { bv = ov; bi = oi; bn = on; }
    }
    if ((tid & 63) == 0) { s_bv[tid >> 6] = bv; s_bi[tid >> 6] = bi; s_bn[tid >> 6] = bn; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < GA_THREADS / 64; ++w) if (ga_better(bv, bi, bn, s_bv[w], s_bi[w], s_bn[w])) { bv = s_bv[w]; bi = s_bi[w]; bn = s_bn[w]; }
        idx_out[row] = bi;
    }
}

extern "C" int varhip_cfg_argmax_f32(const float* logits, const uint8_t* keep, const int64_t* gt, int64_t ld_keep, int64_t* idx_out,
                                     int B, int l, int V, double t_cfg, varhip_stream_t stream) {
    if (!logits || !idx_out || B <= 0 || l <= 0 || V <= 0 || (keep && (!gt || ld_keep < l))) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    VhScope sc(VH_FAM_SAMPLER, (hipStream_t)stream, 3.0 * rows * V, 8.0 * rows * V);
    hipLaunchKernelGGL(k_cfg_argmax, dim3((unsigned)rows), dim3(GA_THREADS), 0, (hipStream_t)stream, logits, keep, gt, ld_keep, idx_out, rows, l,
                       V, (float)(1.0 + t_cfg), (float)t_cfg);
    return vh_launch_status();
}

__global__ void __launch_bounds__(GA_THREADS) k_feature_l1(const float* __restrict__ f_in, const float* __restrict__ f_rec,
                                                           const int64_t* __restrict__ img, int64_t D, float* __restrict__ score) {
    __shared__ double s_part[GA_THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* a = f_in + img[r] * D;
    const float* b = f_rec + r * D;
    double acc = 0.0;
    for (int64_t d = tid; d < D; d += GA_THREADS) acc += (double)fabsf(a[d] - b[d]);
    s_part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int h = GA_THREADS / 2; h >= 1; h >>= 1) {        // fixed pairwise tree: s[t] += s[t + h]
        if (tid < h) s_part[tid] = s_part[tid] + s_part[tid + h];
        __syncthreads();
    }
    if (tid == 0) score[r] = -(float)(s_part[0] / (double)D);
}

extern "C" int varhip_feature_l1_f32(const float* f_in, const float* f_rec, const int64_t* img, int64_t rows, int64_t D, float* score,
                                     varhip_stream_t stream) {
    if (!f_in || !f_rec || !img || !score || rows < 0 || D <= 0) return VARHIP_EINVAL;
    if (rows == 0) return 0;
    VhScope sc(VH_FAM_OTHER, (hipStream_t)stream, 3.0 * rows * D, 8.0 * rows * D);
    hipLaunchKernelGGL(k_feature_l1, dim3((unsigned)rows), dim3(GA_THREADS), 0, (hipStream_t)stream, f_in, f_rec, img, D, score);
    return vh_launch_status();
}
