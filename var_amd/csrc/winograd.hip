// winograd.hip — fused fp32 Winograd F(2x2,3x3) convolution (stride 1, padding 1, NHWC) for the decoder's ResnetBlock convs (gfx950).
//
// out[y][x][co] = bias[co] (+ resid) + sum_ci sum_{ky,kx} in[y+ky-1][x+kx-1][ci] * w[co][ky][kx][ci], computed per 2x2 output tile as
//   Y = A^T [ sum_ci (G g G^T)[co][ci] .* (B^T d B)[ci] ] A        (d: the tile's 4x4 input window, g: a 3x3 kernel)
// 16 multiplies per tile and (ci, co) instead of 36.  U = G g G^T is made once per weight (DecoderEngine.refresh, float64 rounded once)
// and laid out [16 xi][Cin/16][Cout][16]: the 16 input channels of one K tile of one output channel are 64 contiguous bytes.
// Not bit-equal to the direct convolution (k_dma_gemm): the decoder is off the token path; error budget in DESIGN.md §13.
//
// Workgroup = 16 x 16 output pixels (8 x 8 = 64 Winograd tiles) of one image x 32 output channels; 4 waves, wave w owns the four
// transform positions xi = 4w + j (row w of B^T d B).  Per K tile of 16 input channels:
//   * the 18 x 18 input patch goes global -> LDS by LDS-DMA (vh_dma16_buf, 21 requests of 16 pixels x 64 B); pixels outside the
//     image are requests past the buffer descriptor's range, which deliver zeros (the padding);
//   * each wave reads the two patch rows its B^T row needs (ds_read_b128: the 4 channels of one step set at once) and builds its
//     four V values per (tile, channel) in registers — 8 VALU per (tile, channel) — as the B operand of v_mfma_f32_16x16x4_f32;
//   * its U fragments come from global memory (L2) straight into registers (no wave shares another's xi).
// K order: K tile kt outermost, then step s, and within a step lane group kq holds channel 16 kt + 4 kq + s — fixed, independent of
// the batch size and of the image's position in it (no split-K).  Epilogue: each wave reduces its xi row over A (2 values per
// tile and channel), the waves exchange those through LDS once per 16 channels, and every thread finishes A^T . (.) for one tile and
// four channels: bias, optional residual add, NHWC float4 stores and the GroupNorm partial sums.
#include "common.h"

namespace {

constexpr int WG_PT = 18;                         // input patch side (16 outputs + 2 halo)
constexpr int WG_NDMA = 21;                       // 16-pixel LDS-DMA requests per K tile: ceil(18*18 / 16)
constexpr int WG_STAGE = WG_NDMA * 16 * 64;       // bytes of one patch stage (16 channels = 64 B per pixel; slots past 324 are zeros)
constexpr int WG_ZSTR = 20;                       // floats per tile in the epilogue exchange (16 used; 20 makes the b128 reads conflict-free)
constexpr int WG_LDS = 2 * WG_STAGE;
static_assert(8 * 64 * WG_ZSTR * 4 <= WG_LDS, "epilogue exchange must fit in the K-loop stages");

struct WinoP {
    const float* in; const float* u; const float* bias; const float* resid; float* out; double* gn_part;
    int H, W, Cin, Cout, ncg, pw, ppi;
};

__device__ __forceinline__ void wg_wait_dma_barrier() { asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS slot of 16-byte chunk c of patch pixel pix (the DMA swizzles on the source side: slot c holds chunk c ^ g(pix)); with
// g = (pix >> 1) & 3 a b128 lane group of 16 tiles touches each 16-B bank slot at most twice
__device__ __forceinline__ int wg_swz(int pix) { return (pix >> 1) & 3; }

__global__ void __launch_bounds__(256, 2) k_conv3x3_wino(WinoP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    // workgroup -> (patch, 32-channel group), XCD-aware: consecutive `lin` (the channel groups of one patch, then the next patches)
    // run on one XCD, so a patch's input is fetched into one L2
    int lin;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        lin = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + loc;
    }
    const int cg = lin % p.ncg, pidx = lin / p.ncg, b = pidx / p.ppi, pi = pidx - b * p.ppi, py = pi / p.pw, px = pi - py * p.pw;
    const int y0 = py * 16, x0 = px * 16, c0 = cg * 32;
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout, nk = Cin >> 4;

    // ---- DMA roles: request i of wave w is piece qd = w + 4 i (pixels 16 qd .. 16 qd + 15 of the row-major 18 x 18 patch)
    const int64_t img = (int64_t)H * W * Cin;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in + (int64_t)b * img), 0, (int)(img * 4), 0x00020000);
    uint32_t doff[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int pix = (wave + 4 * i) * 16 + (lane >> 2), c = lane & 3;
        const int yy = y0 - 1 + pix / WG_PT, xx = x0 - 1 + pix % WG_PT;
        const bool ok = pix < WG_PT * WG_PT && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        doff[i] = ok ? (uint32_t)((((int64_t)yy * W + xx) * Cin + ((c ^ wg_swz(pix)) << 2)) * 4) : 0x80000000u;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    auto dma = [&](int kt, int st) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (wave + 4 * i < WG_NDMA) vh_dma16_buf(rsrc, doff[i], (uint32_t)kt * 64u, lds0 + st * WG_STAGE + (wave + 4 * i) * 1024);
    };

    // ---- U fragments: xi = 4 wave + j, channels c0 + 16 cb + r16, K tile kt, the 4 input channels 4 kq .. 4 kq + 3 (one per step)
    // read through a buffer descriptor: one 32-bit lane offset, the (xi, K tile, channel block) offset is scalar (U < 2 GB, host-checked)
    const uint32_t ustr_xi = (uint32_t)nk * Cout * 64, ustr_kt = (uint32_t)Cout * 64;          // bytes
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, (int)(16 * ustr_xi), 0x00020000);
    const uint32_t uoff = (uint32_t)((c0 + r16) * 16 + 4 * kq) * 4u;
    auto load_u = [&](int kt, f32x4 (&u)[4][2]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
                u[j][cb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    ursrc, uoff, __builtin_amdgcn_readfirstlane((uint32_t)(4 * wave + j) * ustr_xi + (uint32_t)kt * ustr_kt + cb * 1024u), 0));
    };

    // ---- patch reads: B^T row `wave` combines rows (ra, rb) of the 4x4 window: e = d[ra] + sg * d[rb] (sg * d exact: one rounding)
    const int ra = wave == 3 ? 1 : (wave == 2 ? 2 : wave), rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
    const float sg = wave == 1 ? 1.0f : -1.0f;
    // tile t = r16 of tile block tb: tile row 2 tb + (t >> 3), column t & 7; window pixel (r, c) = (4 tb + 2 (t >> 3) + r) * 18 + 2 (t & 7) + c.
    // 4 tb * 18 = 72 pixels (a multiple of 4), so the swizzle does not depend on tb and tb is an immediate offset (72 * 64 B)
    uint32_t roff[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int pa = (2 * (r16 >> 3) + ra) * WG_PT + 2 * (r16 & 7) + c, pb = (2 * (r16 >> 3) + rb) * WG_PT + 2 * (r16 & 7) + c;
        roff[0][c] = (uint32_t)(pa * 64 + ((kq ^ wg_swz(pa)) << 4));
        roff[1][c] = (uint32_t)(pb * 64 + ((kq ^ wg_swz(pb)) << 4));
    }

    f32x4 acc[4][4][2];                                            // [j][tb][cb]: D[co = 16 cb + 4 kq + e][tile = 16 tb + r16]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[j][tb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int st, const f32x4 (&u)[4][2]) {
        const char* sb = (const char*)smem + st * WG_STAGE;
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
            f32x4 da[4], db[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                da[c] = *(const f32x4*)(sb + roff[0][c] + tb * 72 * 64);
                db[c] = *(const f32x4*)(sb + roff[1][c] + tb * 72 * 64);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float e[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) e[c] = __builtin_fmaf(sg, db[c][s], da[c][s]);
                const float v[4] = {e[0] - e[2], e[1] + e[2], e[2] - e[1], e[1] - e[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[j][tb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[j][cb][s], v[j], acc[j][tb][cb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);                     // one tile block's patch values live at a time (register budget)
        }
    };

    // One U register set (128 accumulators + 32 U + 32 patch floats per lane leave no room for a second one at 2 workgroups per CU): a
    // K tile's U loads go out first, then the DMA of the next patch.  vmcnt retires in order and the compiler does not count the DMA
    // statements, so its wait for the U registers (vmcnt(0) near the top of compute) also waits for that DMA: within one wave the
    // next patch's fetch does not overlap this tile's MFMAs.  The other workgroup's wave on the SIMD covers both latencies.
    f32x4 u[4][2];
    dma(0, 0);
    wg_wait_dma_barrier();
    // two K tiles per trip: the LDS stage is compile-time in each copy of the body
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        load_u(kt, u); dma(kt + 1, 1);
        compute(0, u);
        wg_wait_dma_barrier();
        load_u(kt + 1, u); if (kt + 2 < nk) dma(kt + 2, 0);
        compute(1, u);
        wg_wait_dma_barrier();
    }
    if (kt < nk) { load_u(kt, u); compute(0, u); wg_wait_dma_barrier(); }

    // ---- epilogue, one 16-channel half (cb) at a time
    float* zb = smem;                                              // [wave][b][tile][WG_ZSTR]
    const int et = tid & 63, eq = tid >> 6;                        // this thread's tile and channel quad (4 eq .. 4 eq + 3 of the half)
    const int ety = et >> 3, etx = et & 7;
    const int64_t obase = (((int64_t)b * H + y0 + 2 * ety) * W + x0 + 2 * etx) * Cout;
    const int nblk = p.gn_part ? (H * W) >> 7 : 0;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
            const f32x4 m0 = acc[0][tb][cb], m1 = acc[1][tb][cb], m2 = acc[2][tb][cb], m3 = acc[3][tb][cb];
            const f32x4 z0 = (m0 + m1) + m2, z1 = (m1 - m2) - m3;  // (M A)[wave][0..1]
            const int t = tb * 16 + r16;
            *(f32x4*)(zb + ((wave * 2 + 0) * 64 + t) * WG_ZSTR + 4 * kq) = z0;
            *(f32x4*)(zb + ((wave * 2 + 1) * 64 + t) * WG_ZSTR + 4 * kq) = z1;
        }
        __syncthreads();
        f32x4 z[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) z[i][bb] = *(const f32x4*)(zb + ((i * 2 + bb) * 64 + et) * WG_ZSTR + 4 * eq);
        const int co = c0 + cb * 16 + 4 * eq;
        const f32x4 b4 = *(const f32x4*)(p.bias + co);
        double gs[4] = {0.0, 0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const f32x4 yv = a == 0 ? (z[0][bb] + z[1][bb]) + z[2][bb] : (z[1][bb] - z[2][bb]) - z[3][bb];
                f32x4 v = yv + b4;
                const int64_t o = obase + ((int64_t)a * W + bb) * Cout + co;
                if (p.resid) v = *(const f32x4*)(p.resid + o) + v;
                *(f32x4*)(p.out + o) = v;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double d = (double)v[e]; gs[e] += d; gq[e] += d * d; }
            }
        if (p.gn_part) {
            // lanes 0-31 hold tiles 0-31 (output rows y0 .. y0+7: block 2 pi), lanes 32-63 the lower half (block 2 pi + 1): fixed butterfly
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) { gs[e] += __shfl_xor(gs[e], off, 64); gq[e] += __shfl_xor(gq[e], off, 64); }
            if ((lane & 31) == 0) {
                double* g = p.gn_part + (((int64_t)b * nblk + 2 * pi + (lane >> 5)) * Cout + co) * 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) { g[2 * e] = gs[e]; g[2 * e + 1] = gq[e]; }
            }
        }
        if (cb == 0) __syncthreads();
    }
}

}  // namespace

extern "C" int varhip_conv3x3_wino_nhwc_f32(const float* in, const float* u, const float* bias, const float* resid, float* out, double* gn_part,
                                            int B, int H, int W, int Cin, int Cout, varhip_stream_t stream) {
    if (!in || !u || !bias || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VARHIP_EINVAL;
    if ((H & 15) || (W & 15) || (Cin & 31) || (Cout & 31)) return VARHIP_EINVAL;
    if ((((uintptr_t)in | (uintptr_t)u | (uintptr_t)bias | (uintptr_t)out | (uintptr_t)resid) & 15)) return VARHIP_EINVAL;
    if ((int64_t)H * W * Cin * 4 >= (1ll << 31) || 64ll * Cin * Cout >= (1ll << 31) || (int64_t)B * H * W >= (1ll << 31))
        return VARHIP_EINVAL;                                      // descriptor windows (one image, U), pixel count
    const int ppi = (H / 16) * (W / 16), ncg = Cout / 32;
    const int64_t nwg = (int64_t)B * ppi * ncg;
    if (nwg >= (1ll << 31)) return VARHIP_EINVAL;
    WinoP p{};
    p.in = in; p.u = u; p.bias = bias; p.resid = resid; p.out = out; p.gn_part = gn_part;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ncg = ncg; p.pw = W / 16; p.ppi = ppi;
    const double npix = (double)B * H * W;
    // executed multiplies: 16 per 2x2 tile and (ci, co)
    VhScope scope(VH_FAM_CONV_WINO, (hipStream_t)stream, 2.0 * (npix / 4.0) * 16.0 * Cin * Cout,
                  4.0 * (npix * Cin + npix * Cout * (resid ? 2.0 : 1.0) + 16.0 * Cin * Cout));
    hipLaunchKernelGGL(k_conv3x3_wino, dim3((unsigned)nwg), dim3(256), WG_LDS, (hipStream_t)stream, p);
    return vh_launch_status();
}
