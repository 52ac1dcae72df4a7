// lens.hip — the logit lens (VAR.logit_lens): the prediction the trained head makes from the residual stream behind a block, reduced against
// the final prediction while both scales' fp32 logits are in HBM.  Per token row w = r * l + t, with z the layer's row (m = max z, p its
// softmax) and zf the final row (mf = max zf, pf its softmax):
//   nll, pred, rank   the definitions of k_token_eval (evalstats.hip) on the layer row, from the same pieces of rowlse.h on the same path:
//                     the same bits as varhip_token_eval_f32 gives for that row
//   e_v = vm_exp(z_v - m), ef_v = vm_exp(zf_v - mf)            (fp32; the values of the row pass: m is exact, the exponential is one function)
//   S  = sum_v (double)e_v,    A = sum_{e_v > 0}  (double)e_v  * (double)(z_v - m)
//   Sf = sum_v (double)ef_v,   B = sum_{ef_v > 0} (double)ef_v * ((double)(zf_v - mf) - (double)(z_v - m))
//   ls = vm_log((float)S), lsf = vm_log((float)Sf)
//   entropy = (float)((double)ls - A / S)                      = log s - sum_v e_v (z_v - m) / s
//   kl      = (float)((B / Sf - (double)lsf) + (double)ls)     = sum_v pf_v (logpf_v - logp_v), with sum_v pf_v = 1 taken out of the sum
// The differences z_v - m are fp32 (one rounding each, the one the row pass makes); the four sums are float64 in ONE order that depends on V
// alone, the order of k_token_eval's `smooth` sum (lane i adds its elements j * 256 + 4 * i + c in ascending (j, c) order, the 64 lanes by the
// xor butterfly of detstats.h); S and Sf, not the row pass's fp32 s, normalise them, so entropy and kl are the same bits whether the register
// or the scalar path ran.  Each is rounded to fp32 once.
//   ef_v == 0 adds nothing, whatever the layer row holds there; ef_v > 0 against z_v = -inf adds +inf; a row whose z_v - m is a NaN somewhere
//   (a NaN, a +inf maximum, a row of -inf) gives NaN: entropy from the layer row, kl from either.
//   Equal rows (one pointer or equal contents): every term of B is ef_v * (d - d) = +0, lsf == ls, and kl = (0 - ls) + ls = +0.0 exactly.
// One wave per token row, four rows per 256-thread workgroup, no LDS and no barrier.  Both rows are held in registers (2 x NV float4 per lane:
// 128 row registers at NV = 16) where V % 4 == 0, V <= 4096 and both operands are 16-byte aligned: k_token_eval's own limit, which the nll's
// bits require (the register and the scalar path add the row pass's s in different orders); above it, the memory path reads each row twice.
#include "common.h"
#include "rowlse.h"
#include "detstats.h"

// f(z_v, zf_v, v) for every element of this lane, ascending in v; the same elements in the same order on both paths
template <int NV, typename F>
__device__ __forceinline__ void ln_each(const f32x4* z, const f32x4* zf, const float* row, const float* rowf, int V, int lane, F f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int e = j * 256 + 4 * lane;
            if (e < V) { f(z[j][0], zf[j][0], e); f(z[j][1], zf[j][1], e + 1); f(z[j][2], zf[j][2], e + 2); f(z[j][3], zf[j][3], e + 3); }
        }
    } else {
        for (int e = 4 * lane; e < V; e += 256)
            for (int c = 0; c < 4 && e + c < V; ++c) f(row[e + c], rowf[e + c], e + c);
    }
}

__device__ __forceinline__ int ln_wave_min_index(int i) {               // exact: indices < 2^24 are exact in fp32
    return (int)-vh_wave_max(-(float)i);
}

template <int NV>
__global__ void __launch_bounds__(256) k_token_lens(const float* __restrict__ logits, const float* __restrict__ final_logits,
                                                    const int64_t* __restrict__ gt, int64_t ld_gt, int64_t rows, int l, int V,
                                                    float* __restrict__ nll, float* __restrict__ entropy, float* __restrict__ kl,
                                                    int64_t* __restrict__ pred, int32_t* __restrict__ rank, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // row w = r * l + t of the pass
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t r = w / l;
    const int t = (int)(w - r * l);
    const float* row = logits + w * V;
    const float* rowf = final_logits + w * V;
    const int64_t g = gt[r * ld_gt + t];
    const bool valid = g >= 0 && g < V;                                 // a token outside [0, V) is never dereferenced
    const float zg = valid ? row[g] : NAN;
    const int gi = (int)g;
    f32x4 z[NV > 0 ? NV : 1], zf[NV > 0 ? NV : 1];
    float m, s, mf = -INFINITY;
    if constexpr (NV > 0) {                                             // k_token_eval's row pass on the layer row; the final row needs its maximum only
        vh_row_load<NV, false>(z, row, row, 1.f, 0.f, V, lane);
        vh_row_load<NV, false>(zf, rowf, rowf, 1.f, 0.f, V, lane);
        vh_row_max_expsum<NV>(z, m, s);
#pragma unroll
        for (int j = 0; j < NV; ++j) mf = fmaxf(mf, fmaxf(fmaxf(zf[j][0], zf[j][1]), fmaxf(zf[j][2], zf[j][3])));
    } else {
        vh_row_max_expsum_mem<false>(row, row, 1.f, 0.f, V, lane, m, s);
        for (int v = lane; v < V; v += 64) mf = fmaxf(mf, rowf[v]);
    }
    s = vh_wave_sum(s);
    mf = vh_wave_max(mf);
    // (through scalar registers, as k_token_eval does: the values z - m of the row pass then cannot stay alive across the pass below)
    m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    mf = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mf)));
    const int none = 1 << 24;
    int n = 0, imax = none, inan = none;
    double S = 0.0, A = 0.0, Sf = 0.0, B = 0.0;
    float bad = 0.f, badf = 0.f;
    ln_each<NV>(z, zf, row, rowf, V, lane, [&](float x, float xf, int v) {
        n += (x > zg || (x == zg && v < gi)) ? 1 : 0;
        imax = (x == m && v < imax) ? v : imax;
        inan = (x != x && v < inan) ? v : inan;
        const float d = x - m, df = xf - mf;
        const float e = vm_exp(d), ef = vm_exp(df);
        S = S + (double)e;
        Sf = Sf + (double)ef;
        if (e > 0.f) A = A + (double)e * (double)d;
        if (ef > 0.f) B = B + (double)ef * ((double)df - (double)d);
        bad = (d != d) ? 1.f : bad;
        badf = (df != df) ? 1.f : badf;
    });
    const int rk = (int)vh_wave_sum((float)n);                          // exact: counts < 2^24 are exact in fp32
    imax = ln_wave_min_index(imax);
    inan = ln_wave_min_index(inan);
    S = vh_wave_sum_f64(S);
    A = vh_wave_sum_f64(A);
    Sf = vh_wave_sum_f64(Sf);
    B = vh_wave_sum_f64(B);
    bad = vh_wave_max(bad);
    badf = vh_wave_max(badf);
    if (lane == 0) {
        const int64_t o = r * ld_out + t;
        const float ls = vm_log((float)S), lsf = vm_log((float)Sf);
        nll[o] = valid ? -vh_row_logp(zg, m, s) : NAN;
        entropy[o] = bad != 0.f ? NAN : (float)((double)ls - A / S);
        kl[o] = (bad != 0.f || badf != 0.f) ? NAN : (float)((B / Sf - (double)lsf) + (double)ls);
        pred[o] = inan < none ? inan : (imax < none ? imax : 0);
        rank[o] = valid ? rk : -1;
    }
}

static inline bool ln_args_ok(const void* logits, const void* final_logits, const void* gt, int64_t ld_gt, int R, int l, int V, const void* a,
                              const void* b, const void* c, const void* d, const void* e, int64_t ld_out) {
    if (!logits || !final_logits || !gt || !a || !b || !c || !d || !e) return false;
    return R > 0 && l > 0 && V > 0 && V < (1 << 24) && ld_gt >= l && ld_out >= l;
}

extern "C" int varhip_token_lens_f32(const float* logits, const float* final_logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V,
                                     float* nll, float* entropy, float* kl, int64_t* pred, int32_t* rank, int64_t ld_out, varhip_stream_t stream) {
    if (!ln_args_ok(logits, final_logits, gt, ld_gt, R, l, V, nll, entropy, kl, pred, rank, ld_out)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)R * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && ((((uintptr_t)logits) | ((uintptr_t)final_logits)) & 15) == 0;
    VhScope sc(VH_FAM_SAMPLER, st, 0, 8.0 * V * (double)rows + 32.0 * rows);
    const dim3 grid((unsigned)blocks);
    // the row path of varhip_token_eval_f32 for the same V and alignment: that is what makes nll its value bit for bit
    if (vec && V <= 1024) hipLaunchKernelGGL((k_token_lens<4>), grid, dim3(256), 0, st, logits, final_logits, gt, ld_gt, rows, l, V, nll, entropy, kl, pred, rank, ld_out);
    else if (vec && V <= 4096) hipLaunchKernelGGL((k_token_lens<16>), grid, dim3(256), 0, st, logits, final_logits, gt, ld_gt, rows, l, V, nll, entropy, kl, pred, rank, ld_out);
    else hipLaunchKernelGGL((k_token_lens<0>), grid, dim3(256), 0, st, logits, final_logits, gt, ld_gt, rows, l, V, nll, entropy, kl, pred, rank, ld_out);
    return vh_launch_status();
}

// ---- host twin (no GPU, no HIP call): the kernel's operations in the kernel's order, a wave as an array of 64 lanes ----------------------
// vm_exp / vm_log consist of correctly rounded operations only and this file is compiled with -ffp-contract=off on both sides, so the twin gives
// the kernel's bits.  (vh_exp_pair of the register path equals vm_exp on every non-NaN input and gives 0 on a NaN.)  Host addresses say nothing
// about the device's: the twin takes the register path's row pass wherever V allows it (V % 4 == 0, V <= 4096), the path the kernel takes
// on 16-byte aligned operands; only nll depends on that choice.
namespace {
double ln_host_sum64_f64(double* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        double q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

float ln_host_sum64(float* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

float ln_host_max(const float* z, int V) {                              // fmaxf drops a NaN operand; the maximum is exact in any order
    float m = -INFINITY;
    for (int v = 0; v < V; ++v) m = __builtin_fmaxf(m, z[v]);
    return m;
}

// s of rowlse.h for the maximum m: reg = the register layout (vh_row_max_expsum), else the lane-strided walk (vh_row_max_expsum_mem)
float ln_host_expsum(const float* z, int V, bool reg, float m) {
    float part[64];
    for (int lane = 0; lane < 64; ++lane) {
        float sl = 0.f;
        if (reg) {
            for (int e = 4 * lane; e < V; e += 256) {
                float x[4];
                for (int c = 0; c < 4; ++c) { const float d = z[e + c] - m; x[c] = (d != d) ? 0.f : vm_exp(d); }
                sl = ((sl + x[0]) + x[1]) + (x[2] + x[3]);
            }
        } else {
            for (int v = lane; v < V; v += 64) sl = sl + vm_exp(z[v] - m);
        }
        part[lane] = sl;
    }
    return ln_host_sum64(part);
}
}  // namespace

extern "C" int varhip_token_lens_host_f32(const float* logits, const float* final_logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V,
                                          float* nll, float* entropy, float* kl, int64_t* pred, int32_t* rank, int64_t ld_out) {
    if (!ln_args_ok(logits, final_logits, gt, ld_gt, R, l, V, nll, entropy, kl, pred, rank, ld_out)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)R * l;
    const bool reg = V % 4 == 0 && V <= 4096;
    for (int64_t w = 0; w < rows; ++w) {
        const int64_t r = w / l, t = w - r * l, o = r * ld_out + t;
        const float* z = logits + w * V;
        const float* zf = final_logits + w * V;
        const int64_t g = gt[r * ld_gt + t];
        const bool valid = g >= 0 && g < V;
        const float zg = valid ? z[g] : NAN;
        const float m = ln_host_max(z, V), mf = ln_host_max(zf, V);
        const float s = ln_host_expsum(z, V, reg, m);
        int64_t n = 0, imax = -1, inan = -1;
        for (int v = 0; v < V; ++v) {
            const float x = z[v];
            n += (x > zg || (x == zg && v < g)) ? 1 : 0;
            if (x == m && imax < 0) imax = v;
            if (x != x && inan < 0) inan = v;
        }
        double pS[64], pA[64], pSf[64], pB[64];
        bool bad = false, badf = false;
        for (int lane = 0; lane < 64; ++lane) {
            double S = 0.0, A = 0.0, Sf = 0.0, B = 0.0;
            for (int e = 4 * lane; e < V; e += 256)
                for (int c = 0; c < 4 && e + c < V; ++c) {
                    const float d = z[e + c] - m, df = zf[e + c] - mf;
                    const float ex = vm_exp(d), ef = vm_exp(df);
                    S = S + (double)ex;
                    Sf = Sf + (double)ef;
                    if (ex > 0.f) A = A + (double)ex * (double)d;
                    if (ef > 0.f) B = B + (double)ef * ((double)df - (double)d);
                    bad = bad || (d != d);
                    badf = badf || (df != df);
                }
            pS[lane] = S; pA[lane] = A; pSf[lane] = Sf; pB[lane] = B;
        }
        const double S = ln_host_sum64_f64(pS), A = ln_host_sum64_f64(pA), Sf = ln_host_sum64_f64(pSf), B = ln_host_sum64_f64(pB);
        const float ls = vm_log((float)S), lsf = vm_log((float)Sf);
        const float lp = -((zg - m) - vm_log(s));
        nll[o] = (valid && lp == lp) ? lp : NAN;                        // (a NaN result: the quiet NaN the device's arithmetic gives, sign and payload)
        entropy[o] = bad ? NAN : (float)((double)ls - A / S);
        kl[o] = (bad || badf) ? NAN : (float)((B / Sf - (double)lsf) + (double)ls);
        pred[o] = inan >= 0 ? inan : (imax >= 0 ? imax : 0);
        rank[o] = valid ? (int32_t)n : -1;
    }
    return 0;
}
