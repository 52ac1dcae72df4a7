// vqstats.hip — the statistics of VectorQuantizer2.forward (reference quant.py:52-104) next to the quantizer loop of quant.hip:
// per scale the code histogram (quant.py:77 bincount) and mse(f_hat, f) (quant.py:95), then the loss combine (quant.py:95,97) and the
// straight-through output (quant.py:98).
//
// Determinism: the histogram uses integer atomics only (integer adds commute: exact and order-free); the squared error is summed in
// float64 in ONE fixed order that depends on n alone, without floating-point atomics:
//   thread g of T = G * 256 (G = varhip_vq_stats_blocks(n)) adds d^2 of elements g, g + T, g + 2T, ... in ascending order,
//   d = (double)f_hat - (double)f (exact: the difference of two floats is a double);
//   a wave adds its 64 lanes by the xor butterfly 32, 16, 8, 4, 2, 1 (both partners add the same pair: identical bits in every lane),
//   a workgroup its four waves as ((w0 + w1) + w2) + w3, and writes the partial to scratch[block];
//   a second one-workgroup launch adds the G partials the same way (thread t: partials t, t + 256, ... ascending; butterfly; four waves).
#include "common.h"

#include "detstats.h"         // the float64 butterfly / four-wave sum and the LDS-first integer histogram, shared with evalstats.hip

extern "C" int varhip_vq_stats_blocks(int64_t n) {
    if (n <= 0) return 0;
    const int64_t g = (n + 4095) / 4096;
    return (int)(g > VARHIP_VQ_STATS_MAX_BLOCKS ? VARHIP_VQ_STATS_MAX_BLOCKS : g);
}

// blocks [0, G): squared-error partials; blocks [0, GH) also count 1024 indices each (GH <= gridDim.x: the grid is max(G, GH) blocks)
__global__ __launch_bounds__(256) void k_vq_scale_stats(const float* __restrict__ f_hat, const float* __restrict__ f, int64_t n, int G,
                                                        const int64_t* __restrict__ idx, int64_t n_idx, int V, unsigned long long* __restrict__ hits,
                                                        double* __restrict__ part, int* __restrict__ bad) {
    __shared__ double red[4];
    __shared__ unsigned int bins[VH_HIST_LDS_BINS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 1024;
    if (i0 < n_idx) {
        const int nbad = vh_hist_block1024([&](int64_t i) { return idx[i]; }, i0, n_idx, V, hits, bins);
        if (nbad) atomicAdd(bad, nbad);
    }
    if ((int)blockIdx.x < G) {                                                   // (uniform per block: the barriers inside are safe)
        const int64_t T = (int64_t)G * 256;
        double s = 0.0;
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += T) {
            const double d = (double)f_hat[i] - (double)f[i];
            s = s + d * d;
        }
        s = vh_block_sum256_f64(s, red);
        if (tid == 0) part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void k_vq_stats_final(const double* __restrict__ part, int G, int64_t n, double* __restrict__ sum_out, float* __restrict__ mse_out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < G; i += 256) s = s + part[i];
    s = vh_block_sum256_f64(s, red);
    if (threadIdx.x == 0) {
        if (sum_out) *sum_out = s;
        *mse_out = (float)(s / (double)n);
    }
}

extern "C" int varhip_vq_scale_stats_f32(const float* f_hat, const float* f, int64_t n, const int64_t* idx, int64_t n_idx, int V, int64_t* hits,
                                         double* scratch, double* sum_out, float* mse_out, int32_t* bad, varhip_stream_t stream) {
    if (n <= 0 || n_idx < 0 || V <= 0 || !f_hat || !f || !hits || !scratch || !mse_out || !bad || (n_idx > 0 && !idx)) return VARHIP_EINVAL;
    if (n_idx > (int64_t)1024 * 65536) return VARHIP_EINVAL;
    const int G = varhip_vq_stats_blocks(n);
    const int GH = (int)((n_idx + 1023) / 1024);
    VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 3.0 * (double)n, 8.0 * (double)n + 8.0 * (double)n_idx);
    hipLaunchKernelGGL(k_vq_scale_stats, dim3(G > GH ? G : GH), dim3(256), 0, (hipStream_t)stream, f_hat, f, n, G, idx, n_idx, V,
                       (unsigned long long*)hits, scratch, bad);
    int rc = vh_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_vq_stats_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, G, n, sum_out, mse_out);
    return vh_launch_status();
}

// quant.py:95,97 on the S values of mse_S, in fp32, one rounding per operation (the library is built with contraction off)
__global__ void k_vq_loss_combine(const float* __restrict__ mse, int S, float beta, float inv_s, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float acc = 0.0f;
    for (int si = 0; si < S; ++si) {
        const float m = mse[si];
        const float t = m * beta + m;
        acc = acc + t;
    }
    *out = acc * inv_s;
}

extern "C" int varhip_vq_loss_combine_f32(const float* mse_S, int S, float beta, float* out, varhip_stream_t stream) {
    if (S <= 0 || !mse_S || !out) return VARHIP_EINVAL;
    hipLaunchKernelGGL(k_vq_loss_combine, dim3(1), dim3(64), 0, (hipStream_t)stream, mse_S, S, beta, (float)(1.0 / (double)S), out);
    return vh_launch_status();
}

// quant.py:98: (f_hat - f) + f per element, channels-last in and out, and [B][C][HW] as well when out_nchw is given
__global__ __launch_bounds__(256) void k_vq_straight_through(const float* __restrict__ f_hat, const float* __restrict__ f, float* __restrict__ out_nhwc,
                                                             float* __restrict__ out_nchw, int64_t n, int HW, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = f_hat[i], b = f[i];
    const float d = a - b;
    const float v = d + b;
    if (out_nhwc) out_nhwc[i] = v;
    if (out_nchw) {
        const int c = (int)(i % C);
        const int64_t pix = i / C, bi = pix / HW, hw = pix - bi * HW;
        out_nchw[(bi * C + c) * HW + hw] = v;
    }
}

extern "C" int varhip_vq_straight_through_f32(const float* f_hat, const float* f, float* out_nhwc, float* out_nchw, int B, int HW, int C,
                                              varhip_stream_t stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || !f_hat || !f || (!out_nhwc && !out_nchw)) return VARHIP_EINVAL;
    const int64_t n = (int64_t)B * HW * C;
    if ((n + 255) / 256 >= (1ll << 31)) return VARHIP_EINVAL;
    VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 2.0 * (double)n, 4.0 * (double)n * (2.0 + (out_nhwc ? 1.0 : 0.0) + (out_nchw ? 1.0 : 0.0)));
    hipLaunchKernelGGL(k_vq_straight_through, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f_hat, f, out_nhwc, out_nchw, n, HW, C);
    return vh_launch_status();
}
