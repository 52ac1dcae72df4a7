// conv16s2.hip — the encoder's Downsample2x on 16-bit activations (reference basic_vae.py:31-37: F.pad(x, (0, 1, 0, 1)) then a 3x3 conv of
// stride 2): out[b][y][x][n] = round16(bias[n] + sum_{ky,kx,c} in[b][2y+ky][2x+kx][c] * w[n][ky][kx][c]), taps past the bottom / right edge
// read zero — the index rule of varhip_conv3x3_s2_nhwc_f32.  Implicit GEMM on the 16-bit MFMA (v_mfma_f32_16x16x32_*) with fp32 accumulation.
// Compiled twice (elem16.h): f16 and bf16.
//
// A workgroup is 4 waves; a wave owns 32 output pixels (two 16-pixel fragments, consecutive in the flattened b / y / x order) x 64 output
// channels (four 16-channel fragments): 8 accumulators.  Each step is one tap and 32 input channels: two 16-byte pixel pieces and four 16-byte
// weight pieces per lane, straight from global memory (a pixel piece is read by at most 4 taps of 4 neighbouring outputs; the weights are
// shared by every wave: both stay in L2), then 8 MFMAs.  The layer is small (4 of the encoder's convolutions, at most 128 x 128 outputs):
// no LDS staging.
#include "common.h"
#include "elem16.h"

namespace VH16_NS {

typedef vh_e16 s2h8 __attribute__((ext_vector_type(8)));
typedef vh_e16 s2h4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_conv16_s2(const vh_e16* __restrict__ in, const vh_e16* __restrict__ w, const float* __restrict__ bias,
                                                   vh_e16* __restrict__ out, int H, int W, int Cin, int Cout, int64_t M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int n0 = blockIdx.y * 64;
    const int Hi = 2 * H, Wi = 2 * W;
    int64_t pb[2]; int py[2], px[2]; bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t q = p0 + 16 * i + r16;
        pv[i] = q < M;
        const int64_t qq = pv[i] ? q : 0;
        pb[i] = qq / ((int64_t)H * W);
        const int64_t rem = qq - pb[i] * H * W;
        py[i] = 2 * (int)(rem / W); px[i] = 2 * (int)(rem % W);
    }
    const vh_e16* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = min(n0 + 16 * j + r16, Cout - 1);               // (channels past Cout repeat the last one: never stored)
        wrow[j] = w + (size_t)n * 9 * Cin + kq * 8;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const s2h8 zero = (s2h8)(vh_e16)0.0f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const vh_e16* arow[2]; bool ok[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = py[i] + ky, ix = px[i] + kx;
            ok[i] = pv[i] && iy < Hi && ix < Wi;                         // the (0, 1, 0, 1) zero pad: only the bottom row / right column
            arow[i] = ok[i] ? in + ((pb[i] * Hi + iy) * Wi + ix) * (int64_t)Cin + kq * 8 : in;
        }
#pragma unroll 1
        for (int c = 0; c < Cin; c += 32) {
            s2h8 a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = ok[i] ? *(const s2h8*)(arow[i] + c) : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const s2h8*)(wrow[j] + (size_t)tap * Cin + c);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = VH16_MFMA_16x16x32(b[j], a[i], acc[i][j]);
        }
    }
    // acc[i][j][e] = C[pixel p0 + 16 i + r16][channel n0 + 16 j + 4 kq + e]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!pv[i]) continue;
        const int64_t q = p0 + 16 * i + r16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nb = n0 + 16 * j + 4 * kq;
            if (nb >= Cout) continue;                                    // (Cout % 16 == 0: a fragment is wholly inside or outside)
            s2h4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (vh_e16)(acc[i][j][e] + bias[nb + e]);
            *(s2h4*)(out + q * Cout + nb) = o;
        }
    }
}

}  // namespace VH16_NS

// in [B][2H][2W][Cin], w [Cout][3][3][Cin] (16-bit), bias fp32 [Cout], out [B][H][W][Cout] (16-bit).  Needs Cin % 32 == 0, Cout % 16 == 0,
// 16-byte aligned in / w, 8-byte aligned out; else VARHIP_EINVAL.
extern "C" int VH16_FN(conv3x3_s2_nhwc)(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                         varhip_stream_t stream) {
    if (!in || !w || !bias || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 15)) return VARHIP_EINVAL;
    if ((((uintptr_t)in | (uintptr_t)w) & 15) || ((uintptr_t)out & 7)) return VARHIP_EINVAL;
    const int64_t M = (int64_t)B * H * W;
    if ((M + 127) / 128 >= (1ll << 31)) return VARHIP_EINVAL;
    const double npix = (double)M;
    VhScope sc(VH_FAM_CONV16_SMALL, (hipStream_t)stream, 2.0 * npix * Cout * 9.0 * Cin, 2.0 * (npix * 4 * Cin + npix * Cout + 9.0 * Cin * Cout));
    hipLaunchKernelGGL(VH16_NS::k_conv16_s2, dim3((unsigned)((M + 127) / 128), (unsigned)((Cout + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                       (const vh_e16*)in, (const vh_e16*)w, bias, (vh_e16*)out, H, W, Cin, Cout, M);
    return vh_launch_status();
}
