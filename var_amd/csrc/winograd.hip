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

// ---- the "wide" shape: 32 tiles x 80 output channels per workgroup ------------------------------------------------------
// Workgroup = one 16 x 8-pixel half patch (8 x 4 = 32 tiles, 18 x 10 input patch, 12 DMA requests: the last one is ragged, its pixels past
// 180 are out-of-range requests) x 80 output channels; wave w still owns row w of B^T d B.  160 accumulators per lane, and every V value
// feeds 5 MFMAs instead of 2: 64 VALU per K tile for 160 MFMAs.  The four positions' U (80 registers) do not fit beside 160 accumulators, so
// the MFMAs of a K tile run position j, channel block cb, step s, tile block tb (a dependent pair is two MFMAs apart), the five U quads are
// one ring indexed by cb, and the quad of (j, cb) is replaced by that of (j + 1, cb) — (0, cb) of the next K tile after j = 3 — right behind
// its 8 MFMAs: every load is 32 MFMAs ahead of its first use.  V of position j needs two window columns of the wave's two patch rows; it is
// read from LDS and built per position (the same expressions, hence the same values, as k_conv3x3_wino's e[c][s] and v).
// Per accumulator the sum runs K tile, step, channel 16 kt + 4 kq + s as above, the epilogue keeps the A^T (.) A association, and a half patch
// is exactly GroupNorm partial block 2 pi + h with the same lane -> tile map and butterfly: outputs and partials equal k_conv3x3_wino's bit for bit.
constexpr int WW_PH = 10;                         // input patch rows (8 outputs + 2 halo); WG_PT columns
constexpr int WW_NDMA = 12;                       // ceil(18 * 10 / 16)
constexpr int WW_STAGE = WW_NDMA * 16 * 64;
constexpr int WW_NCB = 5;                         // 16-channel blocks per workgroup
constexpr int WW_ZBLK = 8 * 32 * WG_ZSTR;         // floats of one channel block in the epilogue exchange: [wave][b][tile][WG_ZSTR]
constexpr int WW_LDS = 2 * WW_ZBLK * 4;           // the exchange takes two channel blocks at a time
static_assert(2 * WW_STAGE <= WW_LDS, "the K-loop stages must fit in the epilogue exchange");

// End of a K tile: the youngest 5 vector-memory operations of a wave are the U quads of position 0 of the next tile; the patch DMA is older
// than the 10 loads before them, whose registers the wave has used since: it has landed, and the barrier publishes it.
__device__ __forceinline__ void ww_wait_dma_barrier() { asm volatile("s_waitcnt vmcnt(5)\n\ts_barrier" ::: "memory"); }

template <bool RES, bool GN, int KO>
__global__ void __launch_bounds__(256, 2) k_conv3x3_wino_wide(WinoP p) {          // p.ncg = Cout / 80
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    int lin;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        lin = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + loc;
    }
    // consecutive `lin`: the channel groups of one half patch, then the other half of the same patch (their halo rows overlap)
    const int cg = lin % p.ncg, hidx = lin / p.ncg, b = hidx / (2 * p.ppi), hp = hidx - b * 2 * p.ppi, pi = hp >> 1, hh = hp & 1;
    const int py = pi / p.pw, px = pi - py * p.pw;
    const int y0 = py * 16 + 8 * hh, x0 = px * 16, c0 = cg * 80;
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout, nk = Cin >> 4;

    // ---- DMA roles: request i of wave w is piece qd = w + 4 i (pixels 16 qd .. 16 qd + 15 of the row-major 10 x 18 patch)
    const int64_t img = (int64_t)H * W * Cin;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in + (int64_t)b * img), 0, (int)(img * 4), 0x00020000);
    uint32_t doff[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int pix = (wave + 4 * i) * 16 + (lane >> 2), c = lane & 3;
        const int yy = y0 - 1 + pix / WG_PT, xx = x0 - 1 + pix % WG_PT;
        const bool ok = pix < WW_PH * WG_PT && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        doff[i] = ok ? (uint32_t)((((int64_t)yy * W + xx) * Cin + ((c ^ wg_swz(pix)) << 2)) * 4) : 0x80000000u;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    auto dma = [&](int kt, int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 3; ++i) vh_dma16_buf(rsrc, doff[i], (uint32_t)kt * 64u, lds0 + st * WW_STAGE + (wave + 4 * i) * 1024);
    };

    // ---- U quads: the ring u[cb] holds (xi = 4 wave + j, channels c0 + 16 cb + r16, K tile kt, input channels 4 kq .. 4 kq + 3) of the
    // position in flight; the table, the descriptor and the lane offset are k_conv3x3_wino's
    const uint32_t ustr_xi = (uint32_t)nk * Cout * 64, ustr_kt = (uint32_t)Cout * 64;          // bytes
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, (int)(16 * ustr_xi), 0x00020000);
    const uint32_t uoff = (uint32_t)((c0 + r16) * 16 + 4 * kq) * 4u;
    f32x4 u[WW_NCB];
    auto load_u = [&](int kt, int j, int cb) __attribute__((always_inline)) {
        u[cb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            ursrc, uoff, __builtin_amdgcn_readfirstlane((uint32_t)(4 * wave + j) * ustr_xi + (uint32_t)kt * ustr_kt + cb * 1024u), 0));
    };
    dma(0, 0);
#pragma unroll
    for (int cb = 0; cb < WW_NCB; ++cb) { load_u(0, 0, cb); __builtin_amdgcn_sched_barrier(0); }

    // ---- patch reads, as in k_conv3x3_wino with two tile blocks: tb is an immediate offset of 72 pixels
    const int ra = wave == 3 ? 1 : (wave == 2 ? 2 : wave), rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
    const float sg = wave == 1 ? 1.0f : -1.0f;
    uint32_t roff[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int pa = (2 * (r16 >> 3) + ra) * WG_PT + 2 * (r16 & 7) + c, pb = (2 * (r16 >> 3) + rb) * WG_PT + 2 * (r16 & 7) + c;
        roff[0][c] = (uint32_t)(pa * 64 + ((kq ^ wg_swz(pa)) << 4));
        roff[1][c] = (uint32_t)(pb * 64 + ((kq ^ wg_swz(pb)) << 4));
    }

    f32x4 acc[4][2][WW_NCB];                                       // [j][tb][cb]: D[co = 16 cb + 4 kq + e][tile = 16 tb + r16]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int cb = 0; cb < WW_NCB; ++cb) acc[j][tb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // V of position j for both tile blocks: e[c] = d[ra][c] + sg * d[rb][c] for the two window columns j combines, then k_conv3x3_wino's v
    auto build_v = [&](const char* sb, int j, f32x4 (&v)[2]) __attribute__((always_inline)) {
        const int ca = j == 0 ? 0 : (j == 2 ? 2 : 1), cc = j == 0 ? 2 : (j == 1 ? 2 : (j == 2 ? 1 : 3));
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const f32x4 daa = *(const f32x4*)(sb + roff[0][ca] + tb * 72 * 64), dba = *(const f32x4*)(sb + roff[1][ca] + tb * 72 * 64);
            const f32x4 dac = *(const f32x4*)(sb + roff[0][cc] + tb * 72 * 64), dbc = *(const f32x4*)(sb + roff[1][cc] + tb * 72 * 64);
            if constexpr (KO & WG_KO_NOBTDB) {
                asm volatile("" :: "v"(dba), "v"(dbc));
#pragma unroll
                for (int s = 0; s < 4; ++s) v[tb][s] = (s & 1) ? dac[s] : daa[s];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float ea = __builtin_fmaf(sg, dba[s], daa[s]), ec = __builtin_fmaf(sg, dbc[s], dac[s]);
                    v[tb][s] = j == 1 ? ea + ec : ea - ec;         // e0 - e2 | e1 + e2 | e2 - e1 | e1 - e3
                }
            }
        }
    };

    // One K tile.  kt_n: the next K tile (its patch goes to the other stage, its position-0 U into the ring behind position 3); the last
    // tile (compile-time flag) does neither.  The DMA goes out behind position 0; the U loads are the compiler's to count.
    auto compute = [&](int st, int kt, int kt_n, auto last) __attribute__((always_inline)) {
        const char* sb = (const char*)smem + st * WW_STAGE;
        f32x4 v[2], vn[2];
        build_v(sb, 0, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int cb = 0; cb < WW_NCB; ++cb) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb) acc[j][tb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[cb][s], v[tb][s], acc[j][tb][cb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (j < 3) load_u(kt, j + 1, cb);
                else if constexpr (!decltype(last)::value) load_u(kt_n, 0, cb);
                if (cb == 1 && j < 3) build_v(sb, j + 1, vn);      // the next position's V under this one's MFMAs
                __builtin_amdgcn_sched_barrier(0);
            }
            if (j == 0 && !decltype(last)::value) dma(kt_n, st ^ 1);
            if (j < 3) { v[0] = vn[0]; v[1] = vn[1]; }
        }
    };

    ww_wait_dma_barrier();
    int kt = 0;
    for (; kt + 2 < nk; kt += 2) {
        compute(0, kt, kt + 1, std::false_type{});
        ww_wait_dma_barrier();
        compute(1, kt + 1, kt + 2, std::false_type{});
        ww_wait_dma_barrier();
    }
    compute(0, kt, kt + 1, std::false_type{});
    ww_wait_dma_barrier();
    compute(1, kt + 1, 0, std::true_type{});
    __builtin_amdgcn_s_barrier();                                  // no DMA is in flight; the exchange below overwrites the stages

    // ---- epilogue, two 16-channel blocks at a time: lanes 0-31 of a wave finish block 2 ps, lanes 32-63 block 2 ps + 1 (the fifth block has
    // no partner: those lanes run on block 4 again and store nothing).  Lane & 31 is the tile, the wave the channel quad.
    float* zb = smem;
    const int nblk = (H * W) >> 7;
    const int et = lane & 31, sel = lane >> 5, eq = wave, ety = et >> 3, etx = et & 7;
    const int64_t obase = (((int64_t)b * H + y0 + 2 * ety) * W + x0 + 2 * etx) * Cout + c0 + 4 * eq;
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {
        const bool active = 2 * ps + sel < WW_NCB;
        const int cbe = active ? 2 * ps + sel : WW_NCB - 1, zsel = active ? sel : 0;
        const f32x4 b4 = *(const f32x4*)(p.bias + c0 + 16 * cbe + 4 * eq);
        f32x4 rs[2][2];
        if constexpr (RES) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) rs[a][bb] = *(const f32x4*)(p.resid + obase + ((int64_t)a * W + bb) * Cout + cbe * 16);
        }
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            const int cb = 2 * ps + c2;
            if (cb >= WW_NCB) continue;
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const f32x4 m0 = acc[0][tb][cb], m1 = acc[1][tb][cb], m2 = acc[2][tb][cb], m3 = acc[3][tb][cb];
                const f32x4 z0 = (m0 + m1) + m2, z1 = (m1 - m2) - m3;  // (M A)[wave][0..1]
                const int t = tb * 16 + r16;
                *(f32x4*)(zb + c2 * WW_ZBLK + ((wave * 2 + 0) * 32 + t) * WG_ZSTR + 4 * kq) = z0;
                *(f32x4*)(zb + c2 * WW_ZBLK + ((wave * 2 + 1) * 32 + t) * WG_ZSTR + 4 * kq) = z1;
            }
        }
        __syncthreads();
        f32x4 z[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) z[i][bb] = *(const f32x4*)(zb + zsel * WW_ZBLK + ((i * 2 + bb) * 32 + et) * WG_ZSTR + 4 * eq);
        const int co = c0 + cbe * 16 + 4 * eq;
        double gs[4] = {0.0, 0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const f32x4 yv = a == 0 ? (z[0][bb] + z[1][bb]) + z[2][bb] : (z[1][bb] - z[2][bb]) - z[3][bb];
                f32x4 v = yv + b4;
                if constexpr (RES) v = rs[a][bb] + v;
                if (active) *(f32x4*)(p.out + obase + ((int64_t)a * W + bb) * Cout + cbe * 16) = v;
                if constexpr (GN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double d = (double)v[e]; gs[e] += d; gq[e] += d * d; }
                }
            }
        if constexpr (GN) {
            // k_conv3x3_wino's sum over the 32 lanes of a half: the same lane -> tile map, the same pairs, the same tree
            const double t8[8] = {gs[0], gq[0], gs[1], gq[1], gs[2], gq[2], gs[3], gq[3]};
            const bool h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
            double r4[4], r2[2], r1;
#pragma unroll
            for (int i = 0; i < 4; ++i) r4[i] = (h4 ? t8[4 + i] : t8[i]) + __shfl_xor(h4 ? t8[i] : t8[4 + i], 16, 64);
#pragma unroll
            for (int i = 0; i < 2; ++i) r2[i] = (h3 ? r4[2 + i] : r4[i]) + __shfl_xor(h3 ? r4[i] : r4[2 + i], 8, 64);
            r1 = (h2 ? r2[1] : r2[0]) + __shfl_xor(h2 ? r2[0] : r2[1], 4, 64);
            r1 += __shfl_xor(r1, 2, 64);
            r1 += __shfl_xor(r1, 1, 64);
            if (active && (lane & 3) == 0)
                p.gn_part[(((int64_t)b * nblk + 2 * pi + hh) * Cout + co) * 2 + ((lane >> 2) & 7)] = r1;
        }
        if (ps < 2) __syncthreads();
    }
}

// ---- Upsample2x (nearest 2x, then conv3x3) on the LOW-resolution map: position-sparse F(2x2,3x3) ----------------------
// The 4x4 window of the 2x2 output tile at (2i, 2j) takes its rows from low-res rows (i-1, i, i, i+1) = (a, b, b, c), so B^T d has rows
// (a - b, 2b, 0, b - c): transform row 2 and, likewise, column 2 vanish.  9 of the 16 positions are left: 9 multiplies per tile and (ci, co).
// The filter side needs no table of its own: with G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]] the rows 0, 1, 3 of G g are g's row 0, half the
// sum of its rows, and its row 2 — and the pre-summed 2x2 phase kernels the direct form already uses (varhip_upconv_pack_f32: w_phase) hold
// exactly those row and column sums.  The halves of G cancel the doublings of B^T d exactly, so neither is applied: the K loop multiplies
// (sums of) phase weights by (a - b | b | b - c) in rows and columns.  Per lane and K tile the nine positions are 9 loads and 6 additions.
//
// Workgroup = 16 x 16 output pixels (64 tiles, one per low-res pixel of an 8 x 8 block) x 32 output channels; 4 waves, wave w owns ALL nine
// positions of tile half th = w & 1 (32 tiles: one 8-row half of the output patch) and channel half ch = w >> 1 (16 channels): 72
// accumulators, the nine filter quads of its channel half (36 registers; each weight byte is loaded by two waves, 36 KB per workgroup and
// K tile against the 32 KB of k_conv3x3_wino), and the whole A^T (.) A of a tile in one lane: no LDS exchange.  Every wave runs the same 72 MFMAs
// per K tile.  Per K tile the 10 x 10 low-res patch (rows of 12 pixel slots, 8 LDS-DMA requests) lands in LDS; padding = requests past the
// descriptor's range, as above.  Chunk c of a pixel in patch row r sits in slot c ^ 2 (r & 1): every 16-lane group of a ds_read_b128 (two tile
// rows x 8 tiles x the lanes' channel quads) then touches each 16-B bank slot once.
// K order as in k_conv3x3_wino: K tile, step, channel 16 kt + 4 kq + s.  Schedule: per tile block the MFMAs run transform row by transform
// row (3 positions in rotation, 4 steps), so the 3 filter quads of a row are dead after its 12 MFMAs of the last tile block and the next K tile's
// go into the same registers there (9 loads per K tile: the counted wait is vmcnt(9)); the next patch's DMA goes out after tile block 0.
constexpr int WU_PS = 12;                         // pixel slots per patch row (10 used: two tile rows = 24 slots keep the swizzle, so tb is an immediate)
constexpr int WU_NDMA = 8;                        // ceil(10 * 12 / 16)
constexpr int WU_STAGE = WU_NDMA * 16 * 64;
constexpr int WU_LDS = 2 * WU_STAGE;

__device__ __forceinline__ void wu_wait_dma_barrier() { asm volatile("s_waitcnt vmcnt(9)\n\ts_barrier" ::: "memory"); }

template <bool GN>
__global__ void __launch_bounds__(256, 2) k_conv3x3_wino_up(WinoP p) {         // p.H, p.W: the OUTPUT map; the input is [H/2][W/2][Cin]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4, th = wave & 1, ch = wave >> 1;
    int lin;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        lin = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + loc;
    }
    const int cg = lin % p.ncg, pidx = lin / p.ncg, b = pidx / p.ppi, pi = pidx - b * p.ppi, py = pi / p.pw, px = pi - py * p.pw;
    const int y0 = py * 16, x0 = px * 16, c0 = cg * 32 + ch * 16;  // c0: this wave's 16 channels
    const int H = p.H, W = p.W, Hi = H >> 1, Wi = W >> 1, Cin = p.Cin, Cout = p.Cout, nk = Cin >> 4;

    // ---- DMA roles: request i of wave w is piece qd = w + 4 i (slots 16 qd .. 16 qd + 15 of the 10 x 12 patch, origin (y0 / 2 - 1, x0 / 2 - 1))
    const int64_t img = (int64_t)Hi * Wi * Cin;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in + (int64_t)b * img), 0, (int)(img * 4), 0x00020000);
    uint32_t doff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pix = (wave + 4 * i) * 16 + (lane >> 2), c = lane & 3;
        const int pr = pix / WU_PS, pc = pix - pr * WU_PS;
        const int yy = (y0 >> 1) - 1 + pr, xx = (x0 >> 1) - 1 + pc;
        const bool ok = pr < 10 && pc < 10 && (unsigned)yy < (unsigned)Hi && (unsigned)xx < (unsigned)Wi;
        doff[i] = ok ? (uint32_t)((((int64_t)yy * Wi + xx) * Cin + ((c ^ ((pr & 1) << 1)) << 2)) * 4) : 0x80000000u;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    auto dma = [&](int kt, int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) vh_dma16_buf(rsrc, doff[i], (uint32_t)kt * 64u, lds0 + st * WU_STAGE + (wave + 4 * i) * 1024);
    };

    // ---- filter fragments of position j = 3 r + c (transform row (0, 1, 3)[r], column (0, 1, 3)[c]) from w_phase [phase 2 py + px][Cout][a][b][Cin];
    // channel c0 + r16, the 4 input channels 4 kq .. 4 kq + 3.  With P = phase 0, Q = phase 1, S = phase 2, T = phase 3 and tap index 2 a + b the
    // registers are loaded with  P0 P1 Q1 | P2 P3 Q3 | S2 S3 T3  and become, row by row before their first MFMA of a K tile,
    //   P0, P0 + P1, Q1 | P0 + P2, (P0 + P1) + (P2 + P3), Q1 + Q3 | S2, S2 + S3, T3     (sums over the kernel rows / columns a phase tap stands for)
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, (int)(64u * Cin * Cout), 0x00020000);
    const uint32_t uoff = (uint32_t)((c0 + r16) * 4 * Cin + 4 * kq) * 4u;
    f32x4 u[9];
    auto load_u = [&](int kt, int r) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            u[3 * r + c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                ursrc, uoff, __builtin_amdgcn_readfirstlane((uint32_t)((((r == 2 ? 2 : 0) + (c == 2 ? 1 : 0)) * Cout * 4 + (r == 0 ? 0 : 2) + (c == 0 ? 0 : 1)) * Cin + 16 * kt) * 4u), 0));
    };
    dma(0, 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) { load_u(0, r); __builtin_amdgcn_sched_barrier(0); }

    // ---- patch reads: tile t = 32 th + 16 tb + r16 is low-res pixel (4 th + 2 tb + (r16 >> 3), r16 & 7) of the 8 x 8 block = patch pixel
    // (+1, +1); its window is patch rows +0 .. +2 (a, b, c) and columns +0 .. +2.  The slot swizzle depends on the patch row's parity alone:
    // one base for window rows 0 and 2, one for row 1; window column, window row, tile block are immediates
    const int prow = 4 * th + (r16 >> 3), pbase = (prow * WU_PS + (r16 & 7)) * 64;
    const uint32_t roff_e = (uint32_t)(pbase + ((kq ^ ((prow & 1) << 1)) << 4)), roff_o = (uint32_t)(pbase + ((kq ^ (((prow + 1) & 1) << 1)) << 4));

    f32x4 acc[9][2];                                               // [j][tb]: D[co = c0 + 4 kq + e][tile = 32 th + 16 tb + r16]
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) acc[j][tb] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 b4;
    auto compute = [&](int st, int kt_dma, int kt_u, auto last) __attribute__((always_inline)) {
        const char* sb = (const char*)smem + st * WU_STAGE;
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            f32x4 d[3][3];                                         // [window row][window column], steps s = 0..3
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[r][c] = *(const f32x4*)(sb + (r == 1 ? roff_o : roff_e) + (r * WU_PS + c + tb * 2 * WU_PS) * 64);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if (tb == 0) {                                     // this row's filter fragments from the phase taps (the order above)
                    if (r == 0) u[1] = u[0] + u[1];
                    if (r == 1) { u[4] = u[1] + (u[3] + u[4]); u[3] = u[0] + u[3]; u[5] = u[2] + u[5]; }
                    if (r == 2) u[7] = u[6] + u[7];
                }
                f32x4 e[3];                                        // row r of B^T d without its doubling: a - b | b | b - c
#pragma unroll
                for (int c = 0; c < 3; ++c) e[c] = r == 0 ? d[0][c] - d[1][c] : (r == 1 ? d[1][c] : d[1][c] - d[2][c]);
                const f32x4 v[3] = {e[0] - e[1], e[1], e[1] - e[2]};
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[3 * r + c][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[3 * r + c][s], v[c][s], acc[3 * r + c][tb], 0, 0, 0);
                if (tb == 1) {
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (decltype(last)::value) { if (r == 0) b4 = *(const f32x4*)(p.bias + c0 + 4 * kq); } else load_u(kt_u, r);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (tb == 0 && !decltype(last)::value) dma(kt_dma, st ^ 1);
        }
    };
    // per wave and K tile the vector-memory order is: DMA of the next patch (after tile block 0), the 9 weight loads (tile block 1), the counted wait
    wu_wait_dma_barrier();
    int kt = 0;
    for (; kt + 2 < nk; kt += 2) {
        compute(0, kt + 1, kt + 1, std::false_type{});
        wu_wait_dma_barrier();
        compute(1, kt + 2, kt + 2, std::false_type{});
        wu_wait_dma_barrier();
    }
    compute(0, kt + 1, kt + 1, std::false_type{});
    wu_wait_dma_barrier();
    compute(1, 0, 0, std::true_type{});

    // ---- epilogue, all in this lane: with m2 = 0, (M A)[r] = (m[r][0] + m[r][1], m[r][1] - m[r][3]), and A^T over the rows the same way:
    // y[0] = z[0] + z[1], y[1] = z[1] - z[3] — the association of k_conv3x3_wino with the zero terms dropped
    const int nblk = (H * W) >> 7;
    double gs[4] = {0.0, 0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int ty = 4 * th + 2 * tb + (r16 >> 3), tx = r16 & 7;
        const int64_t obase = (((int64_t)b * H + y0 + 2 * ty) * W + x0 + 2 * tx) * Cout + c0 + 4 * kq;
        f32x4 z[3][2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            z[r][0] = acc[3 * r][tb] + acc[3 * r + 1][tb]; z[r][1] = acc[3 * r + 1][tb] - acc[3 * r + 2][tb];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const f32x4 v = (a == 0 ? z[0][bb] + z[1][bb] : z[1][bb] - z[2][bb]) + b4;
                *(f32x4*)(p.out + obase + ((int64_t)a * W + bb) * Cout) = v;
                if constexpr (GN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double dd = (double)v[e]; gs[e] += dd; gq[e] += dd * dd; }
                }
            }
    }
    if constexpr (GN) {
        // this wave's 32 tiles are the 8-row half th of the output patch: block 2 pi + th of k_conv3x3_wino's partial layout.  The 16 lanes of a
        // channel quad sum by the fixed xor butterfly 8, 4, 2, 1; the first three levels also halve the quantities a lane carries (8 -> 4 -> 2 -> 1)
        const double t8[8] = {gs[0], gq[0], gs[1], gq[1], gs[2], gq[2], gs[3], gq[3]};        // the order of the partial's 8 doubles
        const bool h3 = lane & 8, h2 = lane & 4, h1 = lane & 2;
        double r4[4], r2[2], r1;
#pragma unroll
        for (int k = 0; k < 4; ++k) r4[k] = (h3 ? t8[4 + k] : t8[k]) + __shfl_xor(h3 ? t8[k] : t8[4 + k], 8, 64);
#pragma unroll
        for (int k = 0; k < 2; ++k) r2[k] = (h2 ? r4[2 + k] : r4[k]) + __shfl_xor(h2 ? r4[k] : r4[2 + k], 4, 64);
        r1 = (h1 ? r2[1] : r2[0]) + __shfl_xor(h1 ? r2[0] : r2[1], 2, 64);
        r1 += __shfl_xor(r1, 1, 64);
        if ((lane & 1) == 0)                                       // lane bits 3, 2, 1 name the quantity this lane ended up with
            p.gn_part[(((int64_t)b * nblk + 2 * pi + th) * Cout + c0 + 4 * kq) * 2 + ((lane >> 1) & 7)] = r1;
    }
}

}  // namespace

// 0 when the shape is one k_conv3x3_wino_up takes
static bool wino_up_ok(const float* in, const float* w_phase, const float* bias, float* out, int B, int H, int W, int Cin, int Cout) {
    if (!in || !w_phase || !bias || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return false;
    if ((H & 15) || (W & 15) || (Cin & 31) || (Cout & 31)) return false;
    if ((((uintptr_t)in | (uintptr_t)w_phase | (uintptr_t)bias | (uintptr_t)out) & 15)) return false;
    if ((int64_t)(H / 2) * (W / 2) * Cin * 4 >= (1ll << 31) || 64ll * Cin * Cout >= (1ll << 31) || (int64_t)B * H * W >= (1ll << 31))
        return false;                                              // descriptor windows (one low-res image, w_phase), pixel count
    return (int64_t)B * (H / 16) * (W / 16) * (Cout / 32) < (1ll << 31);
}

extern "C" int varhip_conv3x3_wino_up_nhwc_f32(const float* in, const float* w_phase, const float* bias, float* out, double* gn_part,
                                               int B, int H, int W, int Cin, int Cout, varhip_stream_t stream) {
    if (!wino_up_ok(in, w_phase, bias, out, B, H, W, Cin, Cout)) return VARHIP_EINVAL;
    const int ppi = (H / 16) * (W / 16), ncg = Cout / 32;
    const int64_t nwg = (int64_t)B * ppi * ncg;
    WinoP p{};
    p.in = in; p.u = w_phase; p.bias = bias; p.resid = nullptr; p.out = out; p.gn_part = gn_part;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ncg = ncg; p.pw = W / 16; p.ppi = ppi;
    const double npix = (double)B * H * W;
    // executed multiplies: 9 per 2x2 tile and (ci, co)
    VhScope scope(VH_FAM_CONV_WINO_UP, (hipStream_t)stream, 2.0 * (npix / 4.0) * 9.0 * Cin * Cout,
                  4.0 * (npix / 4.0 * Cin + npix * Cout + 16.0 * Cin * Cout));
    hipLaunchKernelGGL(gn_part ? k_conv3x3_wino_up<true> : k_conv3x3_wino_up<false>, dim3((unsigned)nwg), dim3(256), WU_LDS, (hipStream_t)stream, p);
    return vh_launch_status();
}

// The switch of varhip_upconv_phase[_gn]_f32 (gemm.hip): non-zero, a launch whose shape k_conv3x3_wino_up takes runs there.  A plain exported
// int, 0 by default: every direct caller gets the four-phase kernel; DecoderEngine.upsample sets it around its own launch (var_amd/hip.py).
extern "C" { int vh_g_upconv_wino = 0; }
int vh_upconv_wino_try(const float* in, const float* w_phase, const float* bias, float* out, double* gn_part,
                       int B, int H, int W, int Cin, int Cout, hipStream_t stream) {
    if (!vh_g_upconv_wino || !wino_up_ok(in, w_phase, bias, out, B, H, W, Cin, Cout)) return 1;        // 1: not taken
    return varhip_conv3x3_wino_up_nhwc_f32(in, w_phase, bias, out, gn_part, B, H, W, Cin, Cout, (varhip_stream_t)stream);
}

// Which shape a launch of varhip_conv3x3_wino_nhwc_f32 takes: 0 = k_conv3x3_wino (64 tiles x 32 channels), 1 = k_conv3x3_wino_wide (32 tiles x
// 80 channels; Cout must be a multiple of 80).  Both give the same bits.  The automatic rule is the measured one of DESIGN.md §13.3.
// varhip_wino_force_shape(-1 | 0 | 1): tests and experiments (VARHIP_WINO_SHAPE sets the start value); a forced 1 still falls back to 0
// where Cout is no multiple of 80.  varhip_wino_last_shape(): the shape of the latest accepted launch.
static int vh_g_wino_force_shape = [] { const char* e = getenv("VARHIP_WINO_SHAPE"); const int t = e ? atoi(e) : -1; return (t == 0 || t == 1) ? t : -1; }();
static int vh_g_wino_last_shape = -1;
extern "C" int varhip_wino_force_shape(int shape) { vh_g_wino_force_shape = (shape == 0 || shape == 1) ? shape : -1; return 0; }
extern "C" int varhip_wino_last_shape(void) { return vh_g_wino_last_shape; }
extern "C" int varhip_wino_auto_shape(int H, int W, int Cin, int Cout) {
    (void)H; (void)W; (void)Cin;                                   // every decoder level measured 4-8 % faster on the wide shape
    return Cout > 0 && Cout % 80 == 0;
}
extern "C" int varhip_wino_pick_shape(int H, int W, int Cin, int Cout) {
    if (Cout <= 0 || Cout % 80) return 0;
    if (Cout & 31) return 1;                                       // 80, 240, ...: no whole groups of 32, the wide shape is the only one
    return vh_g_wino_force_shape >= 0 ? vh_g_wino_force_shape : varhip_wino_auto_shape(H, W, Cin, Cout);
}

extern "C" int varhip_conv3x3_wino_nhwc_f32(const float* in, const float* u, const float* bias, const float* resid, float* out, double* gn_part,
                                            int B, int H, int W, int Cin, int Cout, varhip_stream_t stream) {
    if (!in || !u || !bias || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VARHIP_EINVAL;
    if ((H & 15) || (W & 15) || (Cin & 31) || ((Cout & 31) && (Cout % 80))) return VARHIP_EINVAL;      // Cout: whole groups of 32, or of 80 (wide shape only)
    if ((((uintptr_t)in | (uintptr_t)u | (uintptr_t)bias | (uintptr_t)out | (uintptr_t)resid) & 15)) return VARHIP_EINVAL;
    if ((int64_t)H * W * Cin * 4 >= (1ll << 31) || 64ll * Cin * Cout >= (1ll << 31) || (int64_t)B * H * W >= (1ll << 31))
        return VARHIP_EINVAL;                                      // descriptor windows (one image, U), pixel count
    const int shape = varhip_wino_pick_shape(H, W, Cin, Cout);
    const int ppi = (H / 16) * (W / 16), ncg = shape ? Cout / 80 : Cout / 32;
    const int64_t nwg = (int64_t)B * ppi * ncg * (shape ? 2 : 1);
    if (nwg >= (1ll << 31)) return VARHIP_EINVAL;
    vh_g_wino_last_shape = shape;                                  // varhip_wino_last_shape (a refused call never gets here)
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
    if (shape) {                                                   // the wide shape has knock-out 8 alone
        if (dbg & ~WG_KO_NOBTDB) return VARHIP_EINVAL;
        auto wfn = (dbg & WG_KO_NOBTDB) ? k_conv3x3_wino_wide<true, true, WG_KO_NOBTDB>
                 : res ? (gn ? k_conv3x3_wino_wide<true, true, 0> : k_conv3x3_wino_wide<true, false, 0>)
                       : (gn ? k_conv3x3_wino_wide<false, true, 0> : k_conv3x3_wino_wide<false, false, 0>);
        hipLaunchKernelGGL(wfn, dim3((unsigned)nwg), dim3(256), WW_LDS, (hipStream_t)stream, p);
        return vh_launch_status();
    }
    auto kfn = (dbg & WG_KO_NOEPI) ? k_conv3x3_wino<false, false, WG_KO_NOEPI> : (dbg & WG_KO_NOBTDB) ? k_conv3x3_wino<true, true, WG_KO_NOBTDB>
             : res ? (gn ? k_conv3x3_wino<true, true, 0> : k_conv3x3_wino<true, false, 0>)
                   : (gn ? k_conv3x3_wino<false, true, 0> : k_conv3x3_wino<false, false, 0>);
    hipLaunchKernelGGL(kfn, dim3((unsigned)nwg), dim3(256), WG_LDS, (hipStream_t)stream, p);
    return vh_launch_status();
}
