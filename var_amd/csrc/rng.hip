// rng.hip — the project's own Exp(1) stream for per-image sampling (VAR.autoregressive_infer_cfg_per_image): a counter-based fill whose
// value at (seed, scale, row t, column v, draw) is a pure function of those five numbers — not of the batch size, of the image's position
// in the batch or of which scales drew before.  Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), key = the image's 64-bit
// seed, counter = (v / 4, t, scale, draw), element v takes word v % 4.  A word x becomes u = (2 (x >> 9) + 1) * 2^-24 (exact in fp32, never 0
// or 1) and e = -vm_log(u): include/var_math.h's logarithm is built from correctly rounded operations only, so the kernel and the host twin
// below (plain host code of this library, same -ffp-contract=off) produce the same bits.  No libm / ocml transcendental is involved.
#include "common.h"
#include "philox.h"

// (vr_exp1, 32 random bits -> Exp(1), lives in philox.h: abduct.hip draws single values of this stream with it)

// one lane = one Philox block = four consecutive columns of one row = one 16-byte store
__global__ void __launch_bounds__(256) k_exp1_philox(const int64_t* __restrict__ seeds, int l, int V4, int scale, int draw, int64_t nblk,
                                                      float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nblk) return;
    const int64_t row = g / V4;
    const uint32_t v4 = (uint32_t)(g - row * V4);
    const int64_t b = row / l;
    const uint32_t t = (uint32_t)(row - b * l);
    const uint64_t seed = (uint64_t)seeds[b];
    const VrPhilox r = vr_philox4x32_10(v4, t, (uint32_t)scale, (uint32_t)draw, (uint32_t)seed, (uint32_t)(seed >> 32));
    f32x4 e;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = vr_exp1(r.w[k]);
    *(f32x4*)(out + 4 * g) = e;
}

static inline bool vr_args_ok(const void* seeds, int B, int l, int V, int scale, int draw, const void* out) {
    return seeds && out && B > 0 && l > 0 && V > 0 && (V & 3) == 0 && scale >= 0 && draw >= 0 && ((uintptr_t)out & 15) == 0;
}

extern "C" int varhip_exp1_philox_f32(const int64_t* seeds, int B, int l, int V, int scale, int draw, float* out, varhip_stream_t stream) {
    if (!vr_args_ok(seeds, B, l, V, scale, draw, out)) return VARHIP_EINVAL;
    const int V4 = V >> 2;
    const int64_t nblk = (int64_t)B * l * V4, grid = (nblk + 255) / 256;
    if (grid > 0x7fffffffLL) return VARHIP_EINVAL;
    VhScope sc(VH_FAM_SAMPLER, (hipStream_t)stream, 0, 16.0 * nblk);
    hipLaunchKernelGGL(k_exp1_philox, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, seeds, l, V4, scale, draw, nblk, out);
    return vh_launch_status();
}

// ---- host twins (no GPU, no HIP call: usable on a machine without a device) ----------------------------------------------------------
extern "C" int varhip_exp1_philox_host_f32(const int64_t* seeds, int B, int l, int V, int scale, int draw, float* out) {
    if (!seeds || !out || B <= 0 || l <= 0 || V <= 0 || (V & 3) || scale < 0 || draw < 0) return VARHIP_EINVAL;
    const int V4 = V >> 2;
    for (int b = 0; b < B; ++b) {
        const uint64_t seed = (uint64_t)seeds[b];
        for (int t = 0; t < l; ++t) {
            float* o = out + ((int64_t)b * l + t) * V;
            for (int v4 = 0; v4 < V4; ++v4) {
                const VrPhilox r = vr_philox4x32_10((uint32_t)v4, (uint32_t)t, (uint32_t)scale, (uint32_t)draw, (uint32_t)seed, (uint32_t)(seed >> 32));
                for (int k = 0; k < 4; ++k) o[4 * v4 + k] = vr_exp1(r.w[k]);
            }
        }
    }
    return 0;
}

extern "C" int varhip_philox4x32_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    if (!ctr || !key || !out) return VARHIP_EINVAL;
    const VrPhilox r = vr_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int k = 0; k < 4; ++k) out[k] = r.w[k];
    return 0;
}

extern "C" int varhip_exp1_from_bits_host_f32(const uint32_t* bits, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!bits || !out))) return VARHIP_EINVAL;
    for (int64_t i = 0; i < n; ++i) out[i] = vr_exp1(bits[i]);
    return 0;
}
