// rowlse.h — the row pass of teacher-forced scoring, shared by k_token_loglik (loglik.hip) and k_token_eval (evalstats.hip): one wave reads one
// row of fp32 logits (optionally the CFG combine of two rows) and reduces it to m = max z and s = sum exp(z - m).  One piece of code, so
// that the log-probability both kernels derive from (m, s) is the same float for the same row: the rounding points and the summation order
// below are part of the contract of varhip_token_loglik_f32 and of varhip_token_eval_f32 (§21).
#pragma once
#include "common.h"

template <bool CFG>
__device__ __forceinline__ float vh_row_z(const float* lc, const float* lu, int64_t v, float ca, float cb) {
    if (!CFG) return lc[v];
    const float a = ca * lc[v];
    const float b = cb * lu[v];
    return a - b;
}

// the row in NV float4 registers per lane (element j * 256 + 4 * lane + c; V % 4 == 0, 16-byte aligned rows, V <= 256 * NV); the lanes
// past the row hold -inf
template <int NV, bool CFG>
__device__ __forceinline__ void vh_row_load(f32x4 (&z)[NV], const float* lc, const float* lu, float ca, float cb, int V, int lane) {
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
}

// m = max over the row (every lane), s = this lane's part of sum exp(z - m), registers in ascending order (the caller adds the lanes with vh_wave_sum)
template <int NV>
__device__ __forceinline__ void vh_row_max_expsum(const f32x4 (&z)[NV], float& m, float& s) {
    m = -INFINITY; s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(z[j][0], z[j][1]), fmaxf(z[j][2], z[j][3])));
    m = vh_wave_max(m);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const f32x2 e0 = vh_exp_pair(f32x2{z[j][0] - m, z[j][1] - m});
        const f32x2 e1 = vh_exp_pair(f32x2{z[j][2] - m, z[j][3] - m});
        s = ((s + e0[0]) + e0[1]) + (e1[0] + e1[1]);
    }
}

// the same for any V and alignment: scalar loads, lane-strided (element lane, lane + 64, ...), two passes over memory
template <bool CFG>
__device__ __forceinline__ void vh_row_max_expsum_mem(const float* lc, const float* lu, float ca, float cb, int V, int lane, float& m, float& s) {
    m = -INFINITY; s = 0.f;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, vh_row_z<CFG>(lc, lu, v, ca, cb));
    m = vh_wave_max(m);
    for (int v = lane; v < V; v += 64) s = s + vm_exp(vh_row_z<CFG>(lc, lu, v, ca, cb) - m);
}

// log p of the element with value zg: (zg - max z) - log(sum exp(z - max z)), s already added over the wave
__device__ __forceinline__ float vh_row_logp(float zg, float m, float s) {
    return (zg - m) - vm_log(s);
}
