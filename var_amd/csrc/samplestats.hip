// samplestats.hip — scored sampling (VAR.autoregressive_infer_cfg_scored, VAR.sample_best_of): what the sampler's own inputs and outputs say
// about the token it has just drawn, reduced right behind varhip_cfg_sample*_f32 while the scale's logits are still in HBM.  Per token row
// r = b * l + j, with cond = logits row r, uncond = logits row B * l + r, masked = the sampler's masked_out row r, g = idx[r]:
//   lp_cond   = log_softmax(cond)[g]                                  the value of k_token_loglik without guidance, bit for bit
//   lp_guided = log_softmax(z)[g],  z = ca * cond - cb * uncond        the value of k_token_loglik with (ca, cb), bit for bit
//   lp_drawn  = log_softmax(masked)[g]                                the distribution the token was drawn from (-inf entries add 0)
//   kept      = |{v : masked_v != -inf}|
//   entropy   = (float)((0 - sum_v (double)e_v * (double)lp_v) / (double)s)     of the guided row, in nats
// Every log-probability is rowlse.h's (m = max, s = sum exp(z - m), lp = (z_g - m) - vm_log(s)) on the path k_token_loglik takes for the same
// V: the row in 4 float4 registers per lane for V <= 1024, in 16 for V <= 4096, the two-pass lane-strided walk over memory beyond.
// The entropy sum: e_v = vm_exp(z_v - m), lp_v = (z_v - m) - vm_log(s) (the row's own log-probability of v), elements with e_v == 0 are
// skipped (0 * log 0 = 0; that includes z_v = -inf); float64, in ONE order that depends on V alone, the order of k_token_eval's `smooth` sum:
// lane i adds its elements j * 256 + 4 * i + c in ascending (j, c) order, the 64 lanes by the xor butterfly of detstats.h.  A guided row
// holding a NaN has entropy NaN.
// A streaming reduction bound by the three rows' bytes: one wave per row, four rows per 256-thread workgroup, no LDS and no barrier.
#include "common.h"
#include "rowlse.h"
#include "detstats.h"

// f(x, v) for every element of this lane in the entropy sum's order; NV > 0: from the registers, else z(v) is evaluated from memory
template <int NV, typename Z, typename F>
__device__ __forceinline__ void ss_each(const f32x4* z, Z zmem, int V, int lane, F f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int e = j * 256 + 4 * lane;
            if (e < V) { f(z[j][0]); f(z[j][1]); f(z[j][2]); f(z[j][3]); }
        }
    } else {
        for (int e = 4 * lane; e < V; e += 256)
            for (int c = 0; c < 4; ++c) f(zmem(e + c));
    }
}

template <int NV, bool CFG>
__device__ __forceinline__ void ss_row(f32x4 (&z)[NV > 0 ? NV : 1], const float* lc, const float* lu, float ca, float cb, int V, int lane,
                                       float& m, float& s) {
    if constexpr (NV > 0) {
        vh_row_load<NV, CFG>(z, lc, lu, ca, cb, V, lane);
        vh_row_max_expsum<NV>(z, m, s);
    } else {
        vh_row_max_expsum_mem<CFG>(lc, lu, ca, cb, V, lane, m, s);
    }
    s = vh_wave_sum(s);
}

template <int NV>
__global__ void __launch_bounds__(256) k_sample_stats(const float* __restrict__ logits, const float* __restrict__ masked, const int64_t* __restrict__ idx,
                                                      int64_t rows, int l, int V, float ca0, float cb0, const double* __restrict__ t_rows,
                                                      float* __restrict__ lp_cond, float* __restrict__ lp_guided, float* __restrict__ lp_drawn,
                                                      int32_t* __restrict__ kept, float* __restrict__ entropy, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // row w = b * l + j
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t b = w / l;
    const int j = (int)(w - b * l);
    float ca = ca0, cb = cb0;
    if (t_rows) { const double t = t_rows[b]; ca = (float)(1.0 + t); cb = (float)t; }      // rounded as k_cfg_sample_rows rounds them
    const float* lc = logits + w * V;
    const float* lu = logits + (rows + w) * V;                          // unconditional rows follow the conditional ones
    const float* mk = masked + w * V;
    const int64_t g = idx[w];
    const bool valid = g >= 0 && g < V;                                 // a token outside [0, V) (the sampler's -1) is never dereferenced
    f32x4 z[NV > 0 ? NV : 1];
    float m, s;

    ss_row<NV, false>(z, lc, lc, 1.f, 0.f, V, lane, m, s);
    const float o_cond = valid ? vh_row_logp(lc[g], m, s) : NAN;

    ss_row<NV, false>(z, mk, mk, 1.f, 0.f, V, lane, m, s);
    const float o_drawn = valid ? vh_row_logp(mk[g], m, s) : NAN;
    int n = 0;
    ss_each<NV>(z, [&](int v) { return mk[v]; }, V, lane, [&](float x) { n += (x != -INFINITY) ? 1 : 0; });
    const int o_kept = (int)vh_wave_sum((float)n);                      // exact: counts < 2^24 are exact in fp32

    ss_row<NV, true>(z, lc, lu, ca, cb, V, lane, m, s);
    const float o_guided = valid ? vh_row_logp(vh_row_z<true>(lc, lu, valid ? g : 0, ca, cb), m, s) : NAN;
    // (m through a scalar register, as k_token_eval does: the values z - m of the sum above then cannot stay alive across the pass below)
    m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    const float logs = vm_log(s);
    double acc = 0.0;
    float bad = 0.f;
    ss_each<NV>(z, [&](int v) { return vh_row_z<true>(lc, lu, v, ca, cb); }, V, lane, [&](float x) {
        const float d = x - m;
        const float e = vm_exp(d);
        const float lp = d - logs;
        if (e > 0.f) acc = acc + (double)e * (double)lp;
        bad = (x != x) ? 1.f : bad;
    });
    acc = vh_wave_sum_f64(acc);
    bad = vh_wave_max(bad);
    if (lane == 0) {
        const int64_t o = b * ld_out + j;
        lp_cond[o] = o_cond;
        lp_guided[o] = o_guided;
        lp_drawn[o] = o_drawn;
        kept[o] = o_kept;
        entropy[o] = bad != 0.f ? NAN : (float)((0.0 - acc) / (double)s);
    }
}

static inline bool ss_args_ok(const void* logits, const void* masked, const void* idx, int B, int l, int V, const void* a, const void* b_,
                              const void* c, const void* d, const void* e, int64_t ld_out, bool aligned) {
    if (!logits || !masked || !idx || !a || !b_ || !c || !d || !e) return false;
    if (B <= 0 || l <= 0 || V <= 0 || (V & 255) || V > 8192 || ld_out < l) return false;
    if (aligned && ((((uintptr_t)logits) | ((uintptr_t)masked)) & 15)) return false;      // (rows are read 16 bytes per lane)
    return true;
}

extern "C" int varhip_sample_stats_f32(const float* logits, const float* masked, const int64_t* idx, int B, int l, int V, double t_cfg,
                                       const double* t_rows, float* lp_cond, float* lp_guided, float* lp_drawn, int32_t* kept, float* entropy,
                                       int64_t ld_out, varhip_stream_t stream) {
    if (!ss_args_ok(logits, masked, idx, B, l, V, lp_cond, lp_guided, lp_drawn, kept, entropy, ld_out, true)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const float ca = (float)(1.0 + t_cfg), cb = (float)t_cfg;           // as varhip_cfg_sample_f32 rounds them
    VhScope sc(VH_FAM_SAMPLER, st, 0, 4.0 * V * 3.0 * (double)rows + 28.0 * rows);
    const dim3 grid((unsigned)blocks);
    // the row path of varhip_token_loglik_f32 for the same V: that is what makes lp_cond / lp_guided its values bit for bit
    if (V <= 1024)
        hipLaunchKernelGGL((k_sample_stats<4>), grid, dim3(256), 0, st, logits, masked, idx, rows, l, V, ca, cb, t_rows, lp_cond, lp_guided, lp_drawn, kept, entropy, ld_out);
    else if (V <= 4096)
        hipLaunchKernelGGL((k_sample_stats<16>), grid, dim3(256), 0, st, logits, masked, idx, rows, l, V, ca, cb, t_rows, lp_cond, lp_guided, lp_drawn, kept, entropy, ld_out);
    else
        hipLaunchKernelGGL((k_sample_stats<0>), grid, dim3(256), 0, st, logits, masked, idx, rows, l, V, ca, cb, t_rows, lp_cond, lp_guided, lp_drawn, kept, entropy, ld_out);
    return vh_launch_status();
}

// ---- host twin (no GPU, no HIP call): the kernel's operations in the kernel's order, a wave as an array of 64 lanes ----------------------
// vm_exp / vm_log consist of correctly rounded operations only and this file is compiled with -ffp-contract=off on both sides, so the twin gives
// the kernel's bits.  (vh_exp_pair of the register path equals vm_exp on every non-NaN input and gives 0 on a NaN.)
namespace {
struct SsRow {
    const float* lc; const float* lu; bool cfg; float ca, cb;
    float z(int64_t v) const {
        if (!cfg) return lc[v];
        const float a = ca * lc[v];
        const float b = cb * lu[v];
        return a - b;
    }
};

float ss_host_sum64(float* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

double ss_host_sum64_f64(double* p) {
    for (int off = 32; off >= 1; off >>= 1) {
        double q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}

// (m, s) of rowlse.h: reg = the register layout (vh_row_max_expsum), else the lane-strided walk (vh_row_max_expsum_mem)
void ss_host_max_expsum(const SsRow& r, int V, bool reg, float& m, float& s) {
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
    s = ss_host_sum64(part);
}
}  // namespace

extern "C" int varhip_sample_stats_host_f32(const float* logits, const float* masked, const int64_t* idx, int B, int l, int V, double t_cfg,
                                            const double* t_rows, float* lp_cond, float* lp_guided, float* lp_drawn, int32_t* kept,
                                            float* entropy, int64_t ld_out) {
    if (!ss_args_ok(logits, masked, idx, B, l, V, lp_cond, lp_guided, lp_drawn, kept, entropy, ld_out, false)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    const bool reg = V <= 4096;
    for (int64_t w = 0; w < rows; ++w) {
        const int64_t b = w / l, o = b * ld_out + (w - b * l);
        const double t = t_rows ? t_rows[b] : t_cfg;
        const float ca = (float)(1.0 + t), cb = (float)t;
        const float* lc = logits + w * V;
        const float* lu = logits + (rows + w) * V;
        const float* mk = masked + w * V;
        const int64_t g = idx[w];
        const bool valid = g >= 0 && g < V;
        float m, s;
        const SsRow rc{lc, lc, false, 1.f, 0.f}, rm{mk, mk, false, 1.f, 0.f}, rz{lc, lu, true, ca, cb};
        ss_host_max_expsum(rc, V, reg, m, s);
        lp_cond[o] = valid ? (lc[g] - m) - vm_log(s) : NAN;
        ss_host_max_expsum(rm, V, reg, m, s);
        lp_drawn[o] = valid ? (mk[g] - m) - vm_log(s) : NAN;
        int n = 0;
        for (int v = 0; v < V; ++v) n += (mk[v] != -INFINITY) ? 1 : 0;
        kept[o] = n;
        ss_host_max_expsum(rz, V, reg, m, s);
        lp_guided[o] = valid ? (rz.z(g) - m) - vm_log(s) : NAN;
        const float logs = vm_log(s);
        double part[64];
        bool bad = false;
        for (int lane = 0; lane < 64; ++lane) {
            double acc = 0.0;
            for (int e = 4 * lane; e < V; e += 256)
                for (int c = 0; c < 4; ++c) {
                    const float x = rz.z(e + c);
                    const float d = x - m;
                    const float ex = vm_exp(d);
                    const float lp = d - logs;
                    if (ex > 0.f) acc = acc + (double)ex * (double)lp;
                    bad = bad || (x != x);
                }
            part[lane] = acc;
        }
        const double acc = ss_host_sum64_f64(part);
        entropy[o] = bad ? NAN : (float)((0.0 - acc) / (double)s);
    }
    return 0;
}
