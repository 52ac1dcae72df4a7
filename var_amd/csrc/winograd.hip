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
// Schedule: inside a tile block the MFMAs run j-outermost, so the U fragments of position j are dead after the 8 MFMAs of
// j in the last tile block and the next K tile's are loaded into the same registers there (24 MFMAs ahead of their first use); the
// next patch's DMA goes out after the first tile block and the wait before the end-of-tile barrier is counted (it leaves the U loads
// in flight); the epilogue requests bias and residual before the LDS exchange.  Per accumulator the order of the sum is unchanged.
#include <cstdlib>
#include <type_traits>

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

// End of a K tile: the youngest 8 vector-memory operations of a wave are always the next tile's 8 U loads, everything older is
// patch DMA.  vmcnt retires in order, so vmcnt(8) is "my DMA has landed" without waiting for U; the barrier publishes it.
__device__ __forceinline__ void wg_wait_dma_barrier() { asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory"); }

// Timing-only knock-outs (VARHIP_WINO_DBG, tools/bench_kernels.py wino): separate instantiations, the default one carries none of it
constexpr int WG_KO_NOEPI = 1, WG_KO_NOGN = 2, WG_KO_NORES = 4, WG_KO_NOBTDB = 8;

// LDS slot of 16-byte chunk c of patch pixel pix (the DMA swizzles on the source side: slot c holds chunk c ^ g(pix)); with
// g = (pix >> 1) & 3 a b128 lane group of 16 tiles touches each 16-B bank slot at most twice
__device__ __forceinline__ int wg_swz(int pix) { return (pix >> 1) & 3; }

template <bool RES, bool GN, int KO>
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
    f32x4 u[4][2];
    auto load_u = [&](int kt, int j) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
            u[j][cb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                ursrc, uoff, __builtin_amdgcn_readfirstlane((uint32_t)(4 * wave + j) * ustr_xi + (uint32_t)kt * ustr_kt + cb * 1024u), 0));
    };
    // the first patch and the first K tile's U go out together: one round trip before the first MFMA
    dma(0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) { load_u(0, j); __builtin_amdgcn_sched_barrier(0); }     // in the K loop's order: its counted waits then hold on entry too

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

    // ---- epilogue roles: this thread's tile and channel quad (4 eq .. 4 eq + 3 of each 16-channel half)
    const int et = tid & 63, eq = tid >> 6;
    const int ety = et >> 3, etx = et & 7;
    const int64_t obase = (((int64_t)b * H + y0 + 2 * ety) * W + x0 + 2 * etx) * Cout + c0 + 4 * eq;
    // bias and residual are requested in the last tile block of the last K tile, into the U registers as they fall free: one memory
    // round trip, under the last MFMAs, instead of one at every point of use
    f32x4 b4[2], rs[2][2][2];
    auto epi_load = [&](int j) {
        if constexpr (KO & WG_KO_NOEPI) return;
        if (j == 0) { b4[0] = *(const f32x4*)(p.bias + c0 + 4 * eq); b4[1] = *(const f32x4*)(p.bias + c0 + 16 + 4 * eq); }
        if constexpr (RES) {
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) rs[j >> 1][j & 1][bb] = *(const f32x4*)(p.resid + obase + ((int64_t)(j & 1) * W + bb) * Cout + (j >> 1) * 16);
        }
    };

    // One K tile.  kt_dma: the K tile whose patch goes to the other stage; kt_u: the K tile whose U replaces this one's.  The last tile
    // (compile-time flag) does neither: its freed U registers take the epilogue's bias and residual instead.
    auto compute = [&](int st, int kt_dma, int kt_u, auto last) {
        const char* sb = (const char*)smem + st * WG_STAGE;
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
            f32x4 da[4], db[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                da[c] = *(const f32x4*)(sb + roff[0][c] + tb * 72 * 64);
                db[c] = *(const f32x4*)(sb + roff[1][c] + tb * 72 * 64);
            }
            float e[4][4];                                         // [c][s]
            if constexpr (!(KO & WG_KO_NOBTDB)) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int s = 0; s < 4; ++s) e[c][s] = __builtin_fmaf(sg, db[c][s], da[c][s]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float v;
                    if constexpr (KO & WG_KO_NOBTDB) v = (j & 1) ? db[j][s] : da[j][s];
                    else v = j == 0 ? e[0][s] - e[2][s] : (j == 1 ? e[1][s] + e[2][s] : (j == 2 ? e[2][s] - e[1][s] : e[1][s] - e[3][s]));
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[j][tb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[j][cb][s], v, acc[j][tb][cb], 0, 0, 0);
                }
                if (tb == 3) {
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (decltype(last)::value) epi_load(j); else load_u(kt_u, j);
                }
            }
            __builtin_amdgcn_sched_barrier(0);                     // one tile block's patch values live at a time (register budget)
            if (tb == 0 && !decltype(last)::value) dma(kt_dma, st ^ 1);
        }
    };

    // One U register set (128 accumulators + 32 U + 32 patch floats per lane leave no room for a second one at 2 workgroups per CU), refilled
    // position by position in the last tile block of each K tile.  Per wave and K tile the vector-memory order is: DMA of the next patch
    // (after tile block 0), then the 8 U loads (tile block 3), then the counted wait.  The compiler counts only the U loads, and none of
    // them is issued before a DMA it would have to wait through, so its waits for U registers never drain a DMA.
    wg_wait_dma_barrier();
    // two K tiles per trip: the LDS stage is compile-time in each copy of the body.  nk is even (Cin is a multiple of 32, host-checked);
    // the last pair is peeled so that the last tile is a copy of its own.
    int kt = 0;
    for (; kt + 2 < nk; kt += 2) {
        compute(0, kt + 1, kt + 1, std::false_type{});
        wg_wait_dma_barrier();
        compute(1, kt + 2, kt + 2, std::false_type{});
        wg_wait_dma_barrier();
    }
    compute(0, kt + 1, kt + 1, std::false_type{});
    wg_wait_dma_barrier();
    compute(1, 0, 0, std::true_type{});
    __builtin_amdgcn_s_barrier();                                  // no DMA is in flight; the exchange below overwrites the stages
    if constexpr (KO & WG_KO_NOEPI) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) asm volatile("" :: "v"(acc[j][tb][cb]));
        return;
    }

    // ---- epilogue, one 16-channel half (cb) at a time
    float* zb = smem;                                              // [wave][b][tile][WG_ZSTR]
    const int nblk = (H * W) >> 7;
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
        double gs[4] = {0.0, 0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const f32x4 yv = a == 0 ? (z[0][bb] + z[1][bb]) + z[2][bb] : (z[1][bb] - z[2][bb]) - z[3][bb];
                f32x4 v = yv + b4[cb];
                const int64_t o = obase + ((int64_t)a * W + bb) * Cout + cb * 16;
                if constexpr (RES) v = rs[cb][a][bb] + v;
                *(f32x4*)(p.out + o) = v;
                if constexpr (GN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double d = (double)v[e]; gs[e] += d; gq[e] += d * d; }
                }
            }
        if constexpr (GN) {
            // lanes 0-31 hold tiles 0-31 (output rows y0 .. y0+7: block 2 pi), lanes 32-63 the lower half (block 2 pi + 1).  The sum over
            // a half's 32 lanes is the fixed xor butterfly 16, 8, 4, 2, 1 per quantity; the first three levels also halve the number of
            // quantities a lane carries (8 -> 4 -> 2 -> 1: a lane keeps the half its lane bit selects and sends the other), which pairs
            // the same operands in the same tree as a butterfly on all 8 and needs 9 exchanges of a double instead of 40.
            const double t8[8] = {gs[0], gq[0], gs[1], gq[1], gs[2], gq[2], gs[3], gq[3]};    // the order of the partial's 8 doubles
            const bool h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
            double r4[4], r2[2], r1;
#pragma unroll
            for (int i = 0; i < 4; ++i) r4[i] = (h4 ? t8[4 + i] : t8[i]) + __shfl_xor(h4 ? t8[i] : t8[4 + i], 16, 64);
#pragma unroll
            for (int i = 0; i < 2; ++i) r2[i] = (h3 ? r4[2 + i] : r4[i]) + __shfl_xor(h3 ? r4[i] : r4[2 + i], 8, 64);
            r1 = (h2 ? r2[1] : r2[0]) + __shfl_xor(h2 ? r2[0] : r2[1], 4, 64);
            r1 += __shfl_xor(r1, 2, 64);
            r1 += __shfl_xor(r1, 1, 64);
            if ((lane & 3) == 0)                                   // lane bits 4, 3, 2 name the quantity this lane ended up with
                p.gn_part[(((int64_t)b * nblk + 2 * pi + (lane >> 5)) * Cout + co) * 2 + ((lane >> 2) & 7)] = r1;
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
    // VARHIP_WINO_DBG: timing experiments only (bit 1 no epilogue, 2 no GroupNorm partials, 4 no residual, 8 V straight from the patch
    // registers); every value but 0 gives wrong results
    static const int dbg = [] { const char* e = getenv("VARHIP_WINO_DBG"); return e ? atoi(e) : 0; }();
    const bool res = resid && !(dbg & WG_KO_NORES), gn = gn_part && !(dbg & WG_KO_NOGN);
    if ((dbg & WG_KO_NOBTDB) && !(res && gn)) return VARHIP_EINVAL;
    auto kfn = (dbg & WG_KO_NOEPI) ? k_conv3x3_wino<false, false, WG_KO_NOEPI> : (dbg & WG_KO_NOBTDB) ? k_conv3x3_wino<true, true, WG_KO_NOBTDB>
             : res ? (gn ? k_conv3x3_wino<true, true, 0> : k_conv3x3_wino<true, false, 0>)
                   : (gn ? k_conv3x3_wino<false, true, 0> : k_conv3x3_wino<false, false, 0>);
    hipLaunchKernelGGL(kfn, dim3((unsigned)nwg), dim3(256), WG_LDS, (hipStream_t)stream, p);
    return vh_launch_status();
}
