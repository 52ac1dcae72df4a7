// samplerow.h — what the sampler (sampler.hip) and the posterior-noise kernel (abduct.hip) must form with the same operations: the guided
// logit of the CFG pair and the score whose arg-max is the drawn token.  One piece of code for both, so that the noise abduct.hip writes is
// judged by the comparison the sampler will make on it, bit for bit.  Compile with -ffp-contract=off: every operation is rounded on its own.
#pragma once
#include "common.h"

// (1+t)*cond - t*uncond (var.py:172-173), three roundings as in the reference's tensor expression; ca = (float)(1.0 + t), cb = (float)t
__host__ __device__ static inline float vs_cfg_combine(float ca, float c, float cb, float u) {
    const float a = ca * c;
    const float b = cb * u;
    return a - b;
}

// stage (4)'s score of an entry: its probability ev / S (ev = vm_exp(x - m), S the canonical W256 sum) divided by its Exp(1) noise; two
// correctly rounded fp32 divisions, never a reciprocal multiply
__host__ __device__ static inline float vs_score(float ev, float S, float noise) { return (ev / S) / noise; }

// Stage (1) of the sampler's shared body: what fills xs[V], the row's working logits.  Which thread computes an element is irrelevant — the sums
// of the later stages read xs in their own canonical assignment — so every form reads its rows 16 bytes per lane.
struct VsCfgPair {
    static constexpr bool kMinP = false;
    const float* lc; const float* lu; float ca, cb;
    __device__ __forceinline__ void operator()(float* __restrict__ xs, int V, int tid) const {
        for (int i4 = tid; i4 < (V >> 2); i4 += 256) {
            const f32x4 c4 = *(const f32x4*)(lc + 4 * i4), u4 = *(const f32x4*)(lu + 4 * i4);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = vs_cfg_combine(ca, c4[e], cb, u4[e]);
            *(f32x4*)(xs + 4 * i4) = o;
        }
    }
};
