// philox.h — Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), shared by the Exp(1) fill (rng.hip) and the resampling uniform
// (smcresample.hip).  Integer arithmetic only: the kernel and the host code produce the same words.  vr_exp1, the fill's transform of a
// word to Exp(1), follows it: built from include/var_math.h's vm_log, so the same bits on both sides too.
#pragma once
#include <stdint.h>
#include "../../include/var_math.h"

struct VrPhilox { uint32_t w[4]; };

__host__ __device__ static inline VrPhilox vr_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    VrPhilox o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// 32 random bits -> Exp(1): the top 23 bits n give u = (2n + 1) * 2^-24 in [2^-24, 1 - 2^-24] (2n + 1 < 2^24: the conversion and the scaling
// are exact), e = -ln u in (0, 16.7]
__host__ __device__ static inline float vr_exp1(uint32_t x) {
    const float u = (float)(int32_t)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f;
    return -vm_log(u);
}
