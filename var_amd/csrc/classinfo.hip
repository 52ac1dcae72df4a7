// classinfo.hip — VAR.class_information: how much the class changes the model's prediction at a token, the mutual information between the
// class and the next token under the teacher-forced prefix,  I(c ; x_t | x_<t) = H(sum_k pi_k p_k) - sum_k pi_k H(p_k),  reduced behind the
// head from the fp32 logits of a pass (the row layout, unconditional rows, gt addressing and CFG combine of loglik.hip).  The (K, L, V)
// softmax tensor the definition asks for never exists: a workgroup owns one (image, token), its four waves take the pass's class rows in
// turn (wave w: classes w, w + 4, ...), each row is reduced in registers as k_token_loglik reduces it, and the mixture is a V-vector of
// 64-bit fixed-point sums in the workgroup's LDS (32 KB at V = 4096).
//   row k:     m, s, e_v = vm_exp(z_v - m)            rowlse.h
//              H_k                                     the entropy rule of k_sample_stats (float64, canonical lane order, rounded once)
//              p_v = e_v / s                           one fp32 division
//              mix_q[v] += rint(p_v * pi_k * 2^48)     the product is exact in float64 (24 + 24 bits), so this is one rounding
//              hcond_q  += rint(pi_k * H_k * 2^40)     likewise
//   token:     q_v = (float)(mix_q[v] * 2^-48);  A = sum_{q_v > 0} q_v * vm_log(q_v) in float64, thread t of 256 adds its elements
//              j * 1024 + 4 * t + c in ascending (j, c) order, then detstats.h's block sum;  h_mix = (float)(0 - A),
//              h_cond = (float)(hcond_q * 2^-40),  mi = (float)((0 - A) - hcond_q * 2^-40),  logp_mix = vm_log(q_gt)
// Every sum across classes is an integer sum: the per-token results do not depend on the order of the classes, on how the classes are cut
// into passes or on the order of execution.  A pass that holds every class of its images finalises in the same kernel (the mixture never
// leaves the chip); otherwise the workgroup adds its LDS sums into a global accumulator it alone owns for that (image, token), and
// k_class_mix_finish runs after the last chunk.  V > 4096 has no LDS vector: the waves add straight into the global accumulator with 64-bit
// integer atomics.
// The next class row of a wave is loaded into a second register set before the current one is reduced: the kernel is a stream over
// classes x V x 4 bytes per token, and the loads of row k + 4 overlap the exponentials, divisions and LDS adds of row k.
#include "common.h"
#include "rowlse.h"
#include "detstats.h"

#define CM_LDS_V 4096                      // the mixture lives in LDS up to this V
#define CM_MIX_ONE 281474976710656.0       // 2^48
#define CM_H_ONE 1099511627776.0           // 2^40

__host__ __device__ static inline long long cm_rint_ll(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(x);
#else
    return (long long)__builtin_rint(x);
#endif
}

// the finalise step of one token from its mixture (LDS or global): every thread of the 256 must call it; thread 0 writes
template <typename P>
__device__ __forceinline__ void cm_finalise(P mix, long long hq, int bad, int64_t g, int V, double* red, float* h_mix, float* h_cond, float* mi,
                                            float* logp_mix, int64_t o) {
    double a = 0.0;
    for (int e = 4 * (int)threadIdx.x; e < V; e += 1024)
        for (int c = 0; c < 4; ++c)
            if (e + c < V) {
                const float q = (float)((double)(long long)mix[e + c] * (1.0 / CM_MIX_ONE));
                if (q > 0.f) a = a + (double)q * (double)vm_log(q);
            }
    a = vh_block_sum256_f64(a, red);
    if (threadIdx.x == 0) {
        const double hc = (double)hq * (1.0 / CM_H_ONE);
        const bool valid = g >= 0 && g < V;                                 // a token outside [0, V) is never dereferenced
        const float qg = valid ? (float)((double)(long long)mix[valid ? g : 0] * (1.0 / CM_MIX_ONE)) : 0.f;
        h_mix[o] = bad ? NAN : (float)(0.0 - a);
        h_cond[o] = bad ? NAN : (float)hc;
        mi[o] = bad ? NAN : (float)((0.0 - a) - hc);
        logp_mix[o] = (bad || !valid) ? NAN : vm_log(qg);
    }
}

// NV > 0: the row in NV float4 registers per lane (element j * 256 + 4 * lane + c), NV == 0: any V and alignment, re-read from memory;
// LDSMIX: the mixture of the token in LDS (V <= CM_LDS_V), else straight in the global accumulator
template <int NV, bool CFG, bool LDSMIX>
__global__ void __launch_bounds__(256) k_class_mix(const float* __restrict__ logits, const int64_t* __restrict__ gt, int64_t ld_gt, int images,
                                                   int classes, int l, int V, float ca, float cb, const float* __restrict__ prior, int64_t ld_prior,
                                                   float* __restrict__ entropy, int64_t ld_ei, int64_t ld_ec,
                                                   unsigned long long* __restrict__ mix_q, unsigned long long* __restrict__ hcond_q,
                                                   int* __restrict__ nanflag, int64_t ld_acc,
                                                   float* __restrict__ h_mix, float* __restrict__ h_cond, float* __restrict__ mi,
                                                   float* __restrict__ logp_mix, int64_t ld_out) {
    __shared__ unsigned long long s_mix[LDSMIX ? CM_LDS_V : 1];
    __shared__ unsigned long long s_hq;
    __shared__ int s_bad;
    __shared__ double s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = (int)(blockIdx.x / (unsigned)l), t = (int)(blockIdx.x - (unsigned)img * (unsigned)l);
    if constexpr (LDSMIX)
        for (int v = tid; v < V; v += 256) s_mix[v] = 0ull;
    if (tid == 0) { s_hq = 0ull; s_bad = 0; }
    __syncthreads();
    unsigned long long* gm = mix_q ? mix_q + ((int64_t)img * ld_acc + t) * V : nullptr;
    const float* lu = logits + (((int64_t)images * classes + img) * l + t) * V;      // unconditional rows follow the class rows
    const float* row0 = logits + ((int64_t)img * classes * l + t) * V;               // class k of this token: row0 + k * l * V
    const int64_t ld_row = (int64_t)l * V;
    f32x4 z[NV > 0 ? NV : 1], nx[NV > 0 ? NV : 1], un[(NV > 0 && CFG) ? NV : 1];
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int e = j * 256 + 4 * lane;
            if constexpr (CFG) un[j] = e < V ? *(const f32x4*)(lu + e) : (f32x4)(0.f);
            nx[j] = (e < V && wave < classes) ? *(const f32x4*)(row0 + wave * ld_row + e) : (f32x4)(0.f);
        }
    }
    for (int k = wave; k < classes; k += 4) {                                        // (wave-uniform)
        const float* lc = row0 + k * ld_row;
        float m, s;
        if constexpr (NV > 0) {
            // vh_row_load's combine on the prefetched registers, then the loads of this wave's next row
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int e = j * 256 + 4 * lane;
                if (e < V) {
                    if constexpr (CFG) { const f32x4 a = ca * nx[j]; const f32x4 b = cb * un[j]; z[j] = a - b; }
                    else z[j] = nx[j];
                } else {
                    z[j] = (f32x4)(-INFINITY);
                }
            }
            if (k + 4 < classes) {
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int e = j * 256 + 4 * lane;
                    if (e < V) nx[j] = *(const f32x4*)(lc + 4 * ld_row + e);
                }
            }
            vh_row_max_expsum<NV>(z, m, s);
        } else {
            vh_row_max_expsum_mem<CFG>(lc, lu, ca, cb, V, lane, m, s);
        }
        s = vh_wave_sum(s);
        // (m through a scalar register, as k_sample_stats: the values z - m of the sum above cannot stay alive across the pass below)
        m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
        const float logs = vm_log(s);
        const double pk = (double)prior[(int64_t)img * ld_prior + k];
        double acc = 0.0;
        float isbad = 0.f;
        auto elem = [&](float x, int v) {
            const float d = x - m;
            const float e = vm_exp(d);
            const float lp = d - logs;
            if (e > 0.f) acc = acc + (double)e * (double)lp;
            isbad = (x != x) ? 1.f : isbad;
            const float p = e / s;
            if (p > 0.f) {                                                           // (a NaN adds nothing; the token is flagged below)
                const unsigned long long q = (unsigned long long)cm_rint_ll(((double)p * pk) * CM_MIX_ONE);
                if (q) {
                    if constexpr (LDSMIX) atomicAdd(&s_mix[v], q);
                    else atomicAdd(&gm[v], q);
                }
            }
        };
        if constexpr (NV > 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int e = j * 256 + 4 * lane;
                if (e < V) { elem(z[j][0], e); elem(z[j][1], e + 1); elem(z[j][2], e + 2); elem(z[j][3], e + 3); }
            }
        } else {
            for (int e = 4 * lane; e < V; e += 256)
                for (int c = 0; c < 4; ++c)
                    if (e + c < V) elem(vh_row_z<CFG>(lc, lu, e + c, ca, cb), e + c);
        }
        acc = vh_wave_sum_f64(acc);
        isbad = vh_wave_max(isbad);
        if (lane == 0) {
            const float H = (float)((0.0 - acc) / (double)s);
            entropy[(int64_t)img * ld_ei + (int64_t)k * ld_ec + t] = isbad != 0.f ? NAN : H;
            if (isbad != 0.f) atomicOr(&s_bad, 1);
            else atomicAdd(&s_hq, (unsigned long long)cm_rint_ll((pk * (double)H) * CM_H_ONE));
        }
    }
    __syncthreads();
    const int64_t a_o = (int64_t)img * ld_acc + t;
    if (gm) {                                                                        // a chunk: this workgroup is the only owner of its token's sums
        if constexpr (LDSMIX)
            for (int v = tid; v < V; v += 256) { const unsigned long long q = s_mix[v]; if (q) gm[v] += q; }
        if (tid == 0) {
            hcond_q[a_o] += s_hq;
            if (s_bad) nanflag[a_o] = 1;
        }
        return;
    }
    if constexpr (LDSMIX)
        cm_finalise(s_mix, (long long)s_hq, s_bad, gt[(int64_t)img * ld_gt + t], V, s_red, h_mix, h_cond, mi, logp_mix, (int64_t)img * ld_out + t);
}

__global__ void __launch_bounds__(256) k_class_mix_finish(const unsigned long long* __restrict__ mix_q, const unsigned long long* __restrict__ hcond_q,
                                                          const int* __restrict__ nanflag, int64_t ld_acc, const int64_t* __restrict__ gt,
                                                          int64_t ld_gt, int l, int V, float* __restrict__ h_mix, float* __restrict__ h_cond,
                                                          float* __restrict__ mi, float* __restrict__ logp_mix, int64_t ld_out) {
    __shared__ double s_red[4];
    const int img = (int)(blockIdx.x / (unsigned)l), t = (int)(blockIdx.x - (unsigned)img * (unsigned)l);
    const int64_t a_o = (int64_t)img * ld_acc + t;
    cm_finalise(mix_q + a_o * V, (long long)hcond_q[a_o], nanflag[a_o], gt[(int64_t)img * ld_gt + t], V, s_red, h_mix, h_cond, mi, logp_mix,
                (int64_t)img * ld_out + t);
}

static inline bool cm_args_ok(const void* logits, const void* gt, int64_t ld_gt, int images, int classes, int l, int V, const void* prior,
                              int64_t ld_prior, const void* entropy, int64_t ld_ei, int64_t ld_ec, const void* mix_q, const void* hcond_q,
                              const void* nanflag, int64_t ld_acc, const void* h_mix, const void* h_cond, const void* mi, const void* logp_mix,
                              int64_t ld_out) {
    if (!logits || !gt || !prior || !entropy || images <= 0 || classes <= 0 || l <= 0 || V <= 0 || V > (1 << 24) || ld_gt < l ||
        ld_prior < classes || ld_ec < l || ld_ei < (int64_t)classes * ld_ec)
        return false;
    if (mix_q) return hcond_q && nanflag && ld_acc >= l;                             // a chunk: the accumulator, no per-token output
    return V <= CM_LDS_V && h_mix && h_cond && mi && logp_mix && ld_out >= l;        // the on-chip route finalises
}

static inline bool cm_finish_args_ok(const void* mix_q, const void* hcond_q, const void* nanflag, int64_t ld_acc, const void* gt, int64_t ld_gt,
                                     int images, int l, int V, const void* h_mix, const void* h_cond, const void* mi, const void* logp_mix,
                                     int64_t ld_out) {
    return mix_q && hcond_q && nanflag && gt && h_mix && h_cond && mi && logp_mix && images > 0 && l > 0 && V > 0 && V <= (1 << 24) &&
           ld_acc >= l && ld_gt >= l && ld_out >= l;
}

template <int NV, bool LDSMIX>
static void cm_launch(bool cfg, dim3 grid, hipStream_t st, const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l,
                      int V, float ca, float cb, const float* prior, int64_t ld_prior, float* entropy, int64_t ld_ei, int64_t ld_ec,
                      int64_t* mix_q, int64_t* hcond_q, int32_t* nanflag, int64_t ld_acc, float* h_mix, float* h_cond, float* mi, float* logp_mix,
                      int64_t ld_out) {
    if (cfg) hipLaunchKernelGGL((k_class_mix<NV, true, LDSMIX>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, prior,
                                ld_prior, entropy, ld_ei, ld_ec, (unsigned long long*)mix_q, (unsigned long long*)hcond_q, nanflag, ld_acc,
                                h_mix, h_cond, mi, logp_mix, ld_out);
    else hipLaunchKernelGGL((k_class_mix<NV, false, LDSMIX>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, prior,
                            ld_prior, entropy, ld_ei, ld_ec, (unsigned long long*)mix_q, (unsigned long long*)hcond_q, nanflag, ld_acc,
                            h_mix, h_cond, mi, logp_mix, ld_out);
}

extern "C" int varhip_class_mix_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V, int with_uncond,
                                    float ca, float cb, const float* prior, int64_t ld_prior, float* entropy, int64_t ld_ent_img,
                                    int64_t ld_ent_cls, int64_t* mix_q, int64_t* hcond_q, int32_t* nanflag, int64_t ld_acc, float* h_mix,
                                    float* h_cond, float* mi, float* logp_mix, int64_t ld_out, varhip_stream_t stream) {
    if (!cm_args_ok(logits, gt, ld_gt, images, classes, l, V, prior, ld_prior, entropy, ld_ent_img, ld_ent_cls, mix_q, hcond_q, nanflag, ld_acc,
                    h_mix, h_cond, mi, logp_mix, ld_out))
        return VARHIP_EINVAL;
    const int64_t blocks = (int64_t)images * l;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && ((uintptr_t)logits & 15) == 0;                    // the condition of varhip_token_loglik_f32
    const int64_t rows = blocks * classes;
    // bytes: as varhip_token_loglik_f32, plus a chunk's read-modify-write of its tokens' sums
    const double bytes = 4.0 * V * (double)(rows + (with_uncond ? blocks : 0)) + 4.0 * rows + (mix_q ? 16.0 * V * (double)blocks : 16.0 * blocks);
    VhScope sc(VH_FAM_SAMPLER, st, 0, bytes);
    const dim3 grid((unsigned)blocks);
    const bool cfg = with_uncond != 0;
#define CM_GO(NV, LDS) cm_launch<NV, LDS>(cfg, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, prior, ld_prior, entropy, ld_ent_img, \
                                          ld_ent_cls, mix_q, hcond_q, nanflag, ld_acc, h_mix, h_cond, mi, logp_mix, ld_out)
    if (vec && V <= 1024) CM_GO(4, true);
    else if (vec && V <= 4096) CM_GO(16, true);
    else if (V <= CM_LDS_V) CM_GO(0, true);
    else CM_GO(0, false);
#undef CM_GO
    return vh_launch_status();
}

extern "C" int varhip_class_mix_finish_f32(const int64_t* mix_q, const int64_t* hcond_q, const int32_t* nanflag, int64_t ld_acc, const int64_t* gt,
                                           int64_t ld_gt, int images, int l, int V, float* h_mix, float* h_cond, float* mi, float* logp_mix,
                                           int64_t ld_out, varhip_stream_t stream) {
    if (!cm_finish_args_ok(mix_q, hcond_q, nanflag, ld_acc, gt, ld_gt, images, l, V, h_mix, h_cond, mi, logp_mix, ld_out)) return VARHIP_EINVAL;
    const int64_t blocks = (int64_t)images * l;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    VhScope sc(VH_FAM_SAMPLER, st, 0, 8.0 * V * (double)blocks + 36.0 * blocks);
    hipLaunchKernelGGL(k_class_mix_finish, dim3((unsigned)blocks), dim3(256), 0, st, (const unsigned long long*)mix_q,
                       (const unsigned long long*)hcond_q, nanflag, ld_acc, gt, ld_gt, l, V, h_mix, h_cond, mi, logp_mix, ld_out);
    return vh_launch_status();
}

// ---- host twins (no GPU, no HIP call): the kernels' operations in the kernels' order, a wave as an array of 64 lanes -------------------------
// vm_exp / vm_log consist of correctly rounded operations only and this file is compiled with -ffp-contract=off on both sides, so the twins give
// the kernels' bits.  (vh_exp_pair of the register path equals vm_exp on every non-NaN input and gives 0 on a NaN.)  The register path is taken
// where the kernel takes it for 16-byte aligned logits: V % 4 == 0 and V <= 4096.
namespace {
struct CmRow {
    const float* lc; const float* lu; bool cfg; float ca, cb;
    float z(int64_t v) const {
        if (!cfg) return lc[v];
        const float a = ca * lc[v];
        const float b = cb * lu[v];
        return a - b;
    }
};

float cm_host_sum64(float* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

double cm_host_sum64_f64(double* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        double q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

// (m, s) of rowlse.h: reg = the register layout (vh_row_max_expsum), else the lane-strided walk (vh_row_max_expsum_mem)
void cm_host_max_expsum(const CmRow& r, int V, bool reg, float& m, float& s) {
    float part[64];
    m = -INFINITY;
    if (reg) {
        for (int lane = 0; lane < 64; ++lane) {
            float ml = -INFINITY;
            for (int e = 4 * lane; e < V; e += 256)
                ml = __builtin_fmaxf(ml, __builtin_fmaxf(__builtin_fmaxf(r.z(e), r.z(e + 1)), __builtin_fmaxf(r.z(e + 2), r.z(e + 3))));
            m = __builtin_fmaxf(m, ml);
        }
        for (int lane = 0; lane < 64; ++lane) {
            float sl = 0.f;
            for (int e = 4 * lane; e < V; e += 256) {
                float x[4];
                for (int c = 0; c < 4; ++c) { const float d = r.z(e + c) - m; x[c] = (d != d) ? 0.f : vm_exp(d); }
                sl = ((sl + x[0]) + x[1]) + (x[2] + x[3]);
            }
            part[lane] = sl;
        }
    } else {
        for (int lane = 0; lane < 64; ++lane) {
            float ml = -INFINITY;
            for (int v = lane; v < V; v += 64) ml = __builtin_fmaxf(ml, r.z(v));
            m = __builtin_fmaxf(m, ml);
        }
        for (int lane = 0; lane < 64; ++lane) {
            float sl = 0.f;
            for (int v = lane; v < V; v += 64) sl = sl + vm_exp(r.z(v) - m);
            part[lane] = sl;
        }
    }
    s = cm_host_sum64(part);
}

void cm_host_finalise(const int64_t* mix, int64_t hq, int bad, int64_t g, int V, float* h_mix, float* h_cond, float* mi, float* logp_mix, int64_t o) {
    double w[4];
    for (int wave = 0; wave < 4; ++wave) {
        double part[64];
        for (int lane = 0; lane < 64; ++lane) {
            double a = 0.0;
            for (int e = 4 * (wave * 64 + lane); e < V; e += 1024)
                for (int c = 0; c < 4; ++c)
                    if (e + c < V) {
                        const float q = (float)((double)mix[e + c] * (1.0 / CM_MIX_ONE));
                        if (q > 0.f) a = a + (double)q * (double)vm_log(q);
                    }
            part[lane] = a;
        }
        w[wave] = cm_host_sum64_f64(part);
    }
    const double a = ((w[0] + w[1]) + w[2]) + w[3];
    const double hc = (double)hq * (1.0 / CM_H_ONE);
    const bool valid = g >= 0 && g < V;
    const float qg = valid ? (float)((double)mix[g] * (1.0 / CM_MIX_ONE)) : 0.f;
    h_mix[o] = bad ? NAN : (float)(0.0 - a);
    h_cond[o] = bad ? NAN : (float)hc;
    mi[o] = bad ? NAN : (float)((0.0 - a) - hc);
    logp_mix[o] = (bad || !valid) ? NAN : vm_log(qg);
}
}  // namespace

extern "C" int varhip_class_mix_host_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                                         int with_uncond, float ca, float cb, const float* prior, int64_t ld_prior, float* entropy,
                                         int64_t ld_ent_img, int64_t ld_ent_cls, int64_t* mix_q, int64_t* hcond_q, int32_t* nanflag, int64_t ld_acc,
                                         float* h_mix, float* h_cond, float* mi, float* logp_mix, int64_t ld_out) {
    if (!cm_args_ok(logits, gt, ld_gt, images, classes, l, V, prior, ld_prior, entropy, ld_ent_img, ld_ent_cls, mix_q, hcond_q, nanflag, ld_acc,
                    h_mix, h_cond, mi, logp_mix, ld_out))
        return VARHIP_EINVAL;
    const bool reg = V % 4 == 0 && V <= 4096;
    int64_t* local = mix_q ? nullptr : (int64_t*)malloc(sizeof(int64_t) * (size_t)V);
    if (!mix_q && !local) return VARHIP_EINVAL;
    for (int img = 0; img < images; ++img)
        for (int t = 0; t < l; ++t) {
            const int64_t a_o = (int64_t)img * ld_acc + t;
            int64_t* mix = mix_q ? mix_q + a_o * V : local;
            int64_t hq = 0;
            int bad = 0;
            if (!mix_q) for (int v = 0; v < V; ++v) mix[v] = 0;
            const float* lu = logits + (((int64_t)images * classes + img) * l + t) * V;
            for (int k = 0; k < classes; ++k) {
                const float* lc = logits + (((int64_t)img * classes + k) * l + t) * V;
                const CmRow r{lc, lu, with_uncond != 0, ca, cb};
                float m, s;
                cm_host_max_expsum(r, V, reg, m, s);
                const float logs = vm_log(s);
                const double pk = (double)prior[(int64_t)img * ld_prior + k];
                double part[64];
                bool isbad = false;
                for (int lane = 0; lane < 64; ++lane) {
                    double acc = 0.0;
                    for (int e = 4 * lane; e < V; e += 256)
                        for (int c = 0; c < 4; ++c)
                            if (e + c < V) {
                                const float x = r.z(e + c);
                                const float d = x - m;
                                const float ex = vm_exp(d);
                                const float lp = d - logs;
                                if (ex > 0.f) acc = acc + (double)ex * (double)lp;
                                isbad = isbad || (x != x);
                                const float p = ex / s;
                                if (p > 0.f) mix[e + c] += (int64_t)cm_rint_ll(((double)p * pk) * CM_MIX_ONE);
                            }
                    part[lane] = acc;
                }
                const double acc = cm_host_sum64_f64(part);
                const float H = (float)((0.0 - acc) / (double)s);
                entropy[(int64_t)img * ld_ent_img + (int64_t)k * ld_ent_cls + t] = isbad ? NAN : H;
                if (isbad) bad = 1;
                else hq += (int64_t)cm_rint_ll((pk * (double)H) * CM_H_ONE);
            }
            if (mix_q) {
                hcond_q[a_o] += hq;
                if (bad) nanflag[a_o] = 1;
            } else {
                cm_host_finalise(mix, hq, bad, gt[(int64_t)img * ld_gt + t], V, h_mix, h_cond, mi, logp_mix, (int64_t)img * ld_out + t);
            }
        }
    free(local);
    return 0;
}

extern "C" int varhip_class_mix_finish_host_f32(const int64_t* mix_q, const int64_t* hcond_q, const int32_t* nanflag, int64_t ld_acc,
                                                const int64_t* gt, int64_t ld_gt, int images, int l, int V, float* h_mix, float* h_cond,
                                                float* mi, float* logp_mix, int64_t ld_out) {
    if (!cm_finish_args_ok(mix_q, hcond_q, nanflag, ld_acc, gt, ld_gt, images, l, V, h_mix, h_cond, mi, logp_mix, ld_out)) return VARHIP_EINVAL;
    for (int img = 0; img < images; ++img)
        for (int t = 0; t < l; ++t) {
            const int64_t a_o = (int64_t)img * ld_acc + t;
            cm_host_finalise(mix_q + a_o * V, hcond_q[a_o], nanflag[a_o], gt[(int64_t)img * ld_gt + t], V, h_mix, h_cond, mi, logp_mix,
                             (int64_t)img * ld_out + t);
        }
    return 0;
}
