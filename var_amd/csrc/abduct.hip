// abduct.hip — the posterior of the sampler's Exp(1) noise given the token it drew (VAR.abduct_noise / VAR.counterfactual).
// The sampler picks argmax_v p_v / e_v with e_v ~ Exp(1) i.i.d.: the keys e_v / p_v are Exp(p_v), their minimum T is Exp(1) and independent
// of which key attains it, and given the winner g and T every other key is T + Exp(p_v) (memorylessness).  So with fresh E_v, T ~ Exp(1):
//   noise_g = T * p_g,      noise_v = p_v * (T + E_v / p_v) = T * p_v + E_v   (v != g)
// is a draw from the law of the noise given that the sampler returned g.  Replayed through varhip_cfg_sample_rows_f32 with the same logits
// it returns g again; replayed with other logits it gives the coupled (counterfactual) token.  fp32 does not keep the strict inequality
// p_v / noise_v < p_g / noise_g by itself where E_v vanishes next to T * p_v, so every entry is checked with the sampler's own score
// expression (samplerow.h) and, where needed, raised to the smallest float that loses: a closed-form start and five one-ulp steps, no
// data-dependent loop.  One 256-thread workgroup per token row, as the sampler: 2V floats read, V written, 16 bytes per lane.
#include "common.h"
#include "philox.h"
#include "samplerow.h"

#define VA_FLT_MIN 1.17549435e-38f
#define VA_DRAW_FILL 2          // E_v: the value at (seed, scale, t, v, draw 2)
#define VA_DRAW_MIN 3           // T:   the value at (seed, scale, t, 0, draw 3)
#define VA_STEPS 5

__host__ __device__ static inline float va_from_bits(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
__host__ __device__ static inline uint32_t va_bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }

// the race's winner: its noise, and the score r_g every other entry has to stay below
__host__ __device__ static inline float va_noise_g(float T, float pg) { const float n = T * pg; return n > VA_FLT_MIN ? n : VA_FLT_MIN; }

// A loser's noise: the smallest float n >= c = fl(fl(T * p) + E) whose score vs_score(ev, S, n) is strictly below rg.  The score does not
// increase with n, so the admissible n form an upper ray.  Its start lies above p / rg (a score below rg implies p / n < rg) and b = fl(p / rg)
// is within 2^-24 (relative) of that quotient, so pred(b) is at or below the start; and b + 3 ulp is admissible (three ulps of n move p / n
// by more than the 2 * 2^-24 that b's rounding and the score's own rounding can cost).  From max(c, pred(b)) at most four steps are
// needed: five are made.  c >= E >= 5.9e-8 is a normal number, rg is one too (>= 2^-23 even where noise_g was clamped), b is finite.
__host__ __device__ static inline float va_noise_v(float ev, float S, float rg, float T, float E) {
    const float p = ev / S;
    const float tp = T * p;
    const float c = tp + E;
    if (vs_score(ev, S, c) < rg) return c;
    const float b = p / rg;
    float n = c;
    if (b > c) n = va_from_bits(va_bits(b) - 1u);                     // (b > c > 0: positive and not the smallest float; pred(b) >= c)
#pragma unroll
    for (int k = 0; k < VA_STEPS; ++k)
        if (!(vs_score(ev, S, n) < rg)) n = va_from_bits(va_bits(n) + 1u);
    return n;
}

__host__ __device__ static inline float va_exp1_at(uint64_t seed, uint32_t scale, uint32_t t, uint32_t v, uint32_t draw) {
    const VrPhilox r = vr_philox4x32_10(v >> 2, t, scale, draw, (uint32_t)seed, (uint32_t)(seed >> 32));
    return vr_exp1(r.w[v & 3u]);
}

__global__ void __launch_bounds__(256) k_exp1_posterior(const float* __restrict__ logits, const double* __restrict__ t_cfg, const int64_t* __restrict__ gt,
                                                         int64_t ld_gt, const int64_t* __restrict__ seeds, int64_t rows, int l, int V, int scale,
                                                         float* __restrict__ noise_out, float* __restrict__ logp_out, int32_t* __restrict__ flag_out,
                                                         int64_t ld_out) {
    extern __shared__ __attribute__((aligned(16))) float xs[];        // [V] the guided logits, then their exponentials
    __shared__ float red[4];
    __shared__ int s_nan;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, b = row / l;
    const uint32_t t = (uint32_t)(row - b * l);
    const double tc = t_cfg[b];
    const uint64_t seed = (uint64_t)seeds[b];
    const int64_t g = gt[b * ld_gt + t];
    const bool valid = g >= 0 && g < V;

    VsCfgPair{logits + row * V, logits + (rows + row) * V, (float)(1.0 + tc), (float)tc}(xs, V, tid);
    if (tid == 0) s_nan = 0;
    __syncthreads();
    const float xg = xs[valid ? g : 0];
    float m = -INFINITY;
    int bad = 0;
    for (int i = tid; i < V; i += 256) { const float x = xs[i]; m = fmaxf(m, x); bad |= (x != x) ? 1 : 0; }
    if (bad) atomicOr(&s_nan, 1);
    m = vh_block_max256(m, red);                                      // (its barriers also order the reads of xs above before the writes below)
    float part = 0.f;
    for (int i = tid; i < V; i += 256) { const float e = vm_exp(xs[i] - m); xs[i] = e; part = part + e; }
    const float S = vh_block_sum256(part, red);                       // the sampler's stage (4) sum: same assignment, same order
    const float evg = vm_exp(xg - m);
    const float pg = evg / S;
    const float T = va_exp1_at(seed, (uint32_t)scale, t, 0u, VA_DRAW_MIN);
    const float ng = va_noise_g(T, pg);
    const float rg = pg / ng;
    const bool flagged = !valid || s_nan != 0 || pg == 0.0f || !(rg > 0.0f && rg < INFINITY);

    const int64_t orow = b * ld_out + t;
    float* out = noise_out + orow * V;
    for (int i4 = tid; i4 < (V >> 2); i4 += 256) {
        const VrPhilox r = vr_philox4x32_10((uint32_t)i4, t, (uint32_t)scale, VA_DRAW_FILL, (uint32_t)seed, (uint32_t)(seed >> 32));
        const f32x4 e4 = *(const f32x4*)(xs + 4 * i4);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float E = vr_exp1(r.w[k]);
            o[k] = flagged ? E : (4 * i4 + k == g ? ng : va_noise_v(e4[k], S, rg, T, E));
        }
        *(f32x4*)(out + 4 * i4) = o;
    }
    if (tid == 0) {
        logp_out[orow] = flagged ? -INFINITY : (xg - m) - vm_log(S);
        flag_out[orow] = flagged ? 1 : 0;
    }
}

static inline bool va_args_ok(const void* logits, const void* t_cfg, const void* gt, int64_t ld_gt, const void* seeds, int B, int l, int V, int scale,
                              const void* noise_out, const void* logp_out, const void* flag_out, int64_t ld_out, bool aligned) {
    if (!logits || !t_cfg || !gt || !seeds || !noise_out || !logp_out || !flag_out) return false;
    if (B <= 0 || l <= 0 || V <= 0 || (V & 3) || V > 8192 || scale < 0 || ld_gt < l || ld_out < l) return false;
    if (aligned && ((((uintptr_t)logits) | ((uintptr_t)noise_out)) & 15)) return false;      // (rows are read and written 16 bytes per lane)
    return true;
}

extern "C" int varhip_exp1_posterior_f32(const float* logits, const double* t_cfg, const int64_t* gt, int64_t ld_gt, const int64_t* seeds, int B, int l,
                                         int V, int scale, float* noise_out, float* logp_out, int32_t* flag_out, int64_t ld_out,
                                         varhip_stream_t stream) {
    if (!va_args_ok(logits, t_cfg, gt, ld_gt, seeds, B, l, V, scale, noise_out, logp_out, flag_out, ld_out, true)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    if (rows > 0x7fffffffLL) return VARHIP_EINVAL;
    VhScope sc(VH_FAM_SAMPLER, (hipStream_t)stream, 0, 4.0 * rows * V * 3.0);
    hipLaunchKernelGGL(k_exp1_posterior, dim3((unsigned)rows), dim3(256), sizeof(float) * (size_t)V, (hipStream_t)stream, logits, t_cfg, gt, ld_gt, seeds,
                       rows, l, V, scale, noise_out, logp_out, flag_out, ld_out);
    return vh_launch_status();
}

// ---- host twin (no GPU, no HIP call): the kernel's operations in the kernel's order -------------------------------------------------------
namespace {
float va_host_sum64(float* p) {                                       // vh_wave_sum: the xor butterfly 32, 16, 8, 4, 2, 1
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int i = 0; i < 64; ++i) q[i] = p[i] + p[i ^ off];
        for (int i = 0; i < 64; ++i) p[i] = q[i];
    }
    return p[0];
}
}  // namespace

extern "C" int varhip_exp1_posterior_host_f32(const float* logits, const double* t_cfg, const int64_t* gt, int64_t ld_gt, const int64_t* seeds, int B,
                                              int l, int V, int scale, float* noise_out, float* logp_out, int32_t* flag_out, int64_t ld_out) {
    if (!va_args_ok(logits, t_cfg, gt, ld_gt, seeds, B, l, V, scale, noise_out, logp_out, flag_out, ld_out, false)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    if (rows > 0x7fffffffLL) return VARHIP_EINVAL;                    // (the launcher's bound: one workgroup per row)
    float ev[8192];                                                   // V <= 8192 (va_args_ok)
    for (int64_t row = 0; row < rows; ++row) {
        const int64_t b = row / l;
        const uint32_t t = (uint32_t)(row - b * l);
        const double tc = t_cfg[b];
        const float ca = (float)(1.0 + tc), cb = (float)tc;
        const uint64_t seed = (uint64_t)seeds[b];
        const int64_t g = gt[b * ld_gt + t];
        const bool valid = g >= 0 && g < V;
        const float* lc = logits + row * V;
        const float* lu = logits + (rows + row) * V;
        float m = -INFINITY;
        bool bad = false;
        for (int v = 0; v < V; ++v) { const float x = vs_cfg_combine(ca, lc[v], cb, lu[v]); ev[v] = x; m = __builtin_fmaxf(m, x); bad = bad || (x != x); }
        const float xg = ev[valid ? g : 0];
        float part[256], w[4];
        for (int tid = 0; tid < 256; ++tid) {
            float p = 0.f;
            for (int i = tid; i < V; i += 256) { const float e = vm_exp(ev[i] - m); ev[i] = e; p = p + e; }
            part[tid] = p;
        }
        for (int k = 0; k < 4; ++k) w[k] = va_host_sum64(part + 64 * k);
        const float S = ((w[0] + w[1]) + w[2]) + w[3];
        const float evg = vm_exp(xg - m);
        const float pg = evg / S;
        const float T = va_exp1_at(seed, (uint32_t)scale, t, 0u, VA_DRAW_MIN);
        const float ng = va_noise_g(T, pg);
        const float rg = pg / ng;
        const bool flagged = !valid || bad || pg == 0.0f || !(rg > 0.0f && rg < INFINITY);
        const int64_t orow = b * ld_out + t;
        float* out = noise_out + orow * V;
        for (int v = 0; v < V; ++v) {
            const float E = va_exp1_at(seed, (uint32_t)scale, t, (uint32_t)v, VA_DRAW_FILL);
            out[v] = flagged ? E : (v == g ? ng : va_noise_v(ev[v], S, rg, T, E));
        }
        logp_out[orow] = flagged ? -INFINITY : (xg - m) - vm_log(S);
        flag_out[orow] = flagged ? 1 : 0;
    }
    return 0;
}
