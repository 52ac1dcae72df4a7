// attnprofile.hip — where the attention of l new queries over curL cached keys goes: per query the softmax mass on every key scale and on the
// query's own neighbourhood, as integers (VAR.attention_profile; the (L, L) matrix softmax(QK^T) of reference basic_var.py:107-117 is never made).
//
// The scores are the bits k_attn_cached (attn.hip) sees: the same "swapped" product S^T = K_tile . Q^T with MFMA 32x32x2 (A = keys by LDS-DMA,
// B = the query fragments in registers), so a LANE owns one query and its 16 accumulator registers are 16 keys of the 32-key tile (register
// 4g + j of lane half h = key 8g + 4h + j), every q.k one fp32 fma chain in the 4-interleaved channel order.  Unlike attn.hip nothing here is a
// running recurrence: the contract of include/var_hip.h wants the exact maximum first, so the key tiles are walked twice:
//   pass 1: m = max_j s_j and "any score is NaN", per lane, both lane halves of a query combined once at the end (v_permlane32_swap);
//   pass 2: the same scores again (same instructions, same bits), w_j = rint(vm_exp_le0(s_j - m) * 2^30) as an integer, added to the running
//           sum of the key scale the key belongs to.  Scale boundaries are wave-uniform: a lane keeps ONE running 64-bit sum and stores it to
//           its LDS slot [bin][lane] when the walk crosses a boundary; inside the query's own scale a second sum takes the keys whose grid
//           position is within `radius` of the query's (the near bin).
// Then per query Z = sum of the bins, share_b = (W_b << 21) / Z (64-bit integer division, the bins of a query split between its two lanes),
// the shares are added per workgroup in LDS (integer atomics) and leave with one 64-bit global atomic per (row, head, bin, workgroup): integer
// sums, the same bits for any launch geometry and any order of arrival.
// The two exchanges with attn.hip's structure that matter for time: no V tile and no P.V product, but twice the QK^T and a 64-bit integer add per
// key in pass 2.
#include "common.h"

#define AP_KPIECE 272           // floats per 4-row piece of the K tile in LDS (attn.hip's KPIECE: 4 x 64 + 16 pad)
#define AP_MAXS 16              // key scales of one call (bins 0 .. S1-1, the near bin at S1)
#define AP_SHIFT 21             // SHARE_ONE = 2^21
#define AP_W_ONE 1073741824.0f  // 2^30: the fixed point of a softmax numerator

struct ApEnds { int v[AP_MAXS]; };

__device__ __forceinline__ void vh_ap_dma16(const void* base, uint32_t voff, uint32_t lds) {      // attn.hip's LDS-DMA request
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(base), "s"(lds) : "memory", "m0");
}

template <int NW>
__global__ void __launch_bounds__(NW * 64) k_attn_profile(const float* __restrict__ q, const float* __restrict__ kcache, ApEnds ends, int S1,
                                                          int l, int H, int curL, int Lmax, int pn, int radius, uint32_t pn_magic,
                                                          unsigned long long* __restrict__ share_sum, int64_t ld_row, int64_t ld_head,
                                                          int* __restrict__ nan_count, int* __restrict__ tokens, int64_t ld_tok_row, int64_t ld_tok_head) {
    constexpr int KST = 8 * AP_KPIECE;                             // floats per K stage
    __shared__ __attribute__((aligned(16))) float sK[2 * KST];
    __shared__ unsigned long long sW[NW][AP_MAXS + 1][64];         // [wave][bin][lane]: each lane's sum over ITS keys of the bin
    __shared__ unsigned long long sAcc[AP_MAXS + 1];               // the workgroup's share sums
    __shared__ int sEnds[AP_MAXS];
    __shared__ int sNan;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int C = H * 64;
    const int t0 = (blockIdx.x * NW + wave) * 32;                  // this wave's first query
    const int t = t0 + r;
    const float* Kc = kcache + ((int64_t)b * H + hd) * Lmax * 64;
    const int ntile = (curL + 31) / 32;
    const int own0 = curL - l;                                     // first key of the queries' own scale

    if (tid <= AP_MAXS) sAcc[tid] = 0ull;
    if (tid == 0) sNan = 0;
#pragma unroll
    for (int i = 0; i < AP_MAXS; ++i) if (tid == i) sEnds[i] = ends.v[i];

    // ---- Q fragments: lane (query r, half h) keeps q[8c + 4h + u], c = 0..7, u = 0..3 (a lane without a query reads query 0 and writes nothing)
    float qf[32];
    {
        const float* src = q + ((int64_t)b * l + (t < l ? t : 0)) * C + hd * 64 + h2 * 4;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 a = *(const f32x4*)(src + c * 8);
            qf[c * 4 + 0] = a[0]; qf[c * 4 + 1] = a[1]; qf[c * 4 + 2] = a[2]; qf[c * 4 + 3] = a[3];
        }
    }
    const int qy = (t < l ? t : 0) / pn, qx = (t < l ? t : 0) - qy * pn;

    // K tile: 8 pieces of 4 key rows (1 KiB each) by LDS-DMA; wave w issues pieces w, w + NW, ...  Rows past curL repeat the last key: the
    // cache is never read at or beyond curL, and those scores are masked below.
    auto dma_k = [&](int kt, int st) {
#pragma unroll
        for (int n = wave; n < 8; n += NW) {
            int key = kt * 32 + n * 4 + (lane >> 4);
            key = key < curL ? key : curL - 1;
            vh_ap_dma16(Kc, (uint32_t)key * 256u + (uint32_t)(lane & 15) * 16u,
                        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(sK + st * KST + n * AP_KPIECE));
        }
    };

    float mx = -INFINITY;
    unsigned bad = 0u;
    int bin = 0;                                                   // wave-uniform: the key scale the walk of pass 2 is in
    unsigned long long W = 0ull, Wn = 0ull;                        // this lane's running sums: current bin, near bin
    dma_k(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // one loop over both passes: iteration `it` works on tile it mod ntile in stage it & 1 while the next tile of the sequence lands in the other
    for (int it = 0; it < 2 * ntile; ++it) {
        const int kt = it < ntile ? it : it - ntile, buf = it & 1;
        if (it + 1 < 2 * ntile) dma_k(it + 1 < ntile ? it + 1 : it + 1 - ntile, buf ^ 1);
        if (t0 < l) {                                              // (a wave without queries only stages and syncs)
            f32x16 p;
            {
                const float* kb = sK + buf * KST + (r >> 2) * AP_KPIECE + (r & 3) * 64 + h2 * 4;
                f32x4 kf = *(const f32x4*)kb;
                p = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[0], qf[0], (f32x16)(0.f), 0, 0, 0);
                p = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[1], qf[1], p, 0, 0, 0);
                p = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[2], qf[2], p, 0, 0, 0);
                p = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[3], qf[3], p, 0, 0, 0);
#pragma unroll
                for (int c = 1; c < 8; ++c) {
                    kf = *(const f32x4*)(kb + c * 8);
#pragma unroll
                    for (int u = 0; u < 4; ++u) p = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u], qf[c * 4 + u], p, 0, 0, 0);
                }
            }
            const int tlo = kt * 32;
            const bool ragged = tlo + 32 > curL;                   // only the last tile can hold keys past curL (wave-uniform)
            if (it < ntile) {
                // ---- pass 1: exact maximum (fmaxf drops a NaN operand) and the NaN flag
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = tlo + (e & 3) + 8 * (e >> 2) + 4 * h2;
                    if (!ragged || key < curL) {
                        mx = fmaxf(mx, p[e]);
                        bad |= (p[e] != p[e]) ? 1u : 0u;
                    }
                }
                if (it == ntile - 1) {                             // both lane halves of a query agree on m and on the flag
                    const auto xm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                    mx = fmaxf(__uint_as_float(xm[0]), __uint_as_float(xm[1]));
                    const auto xb = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);
                    bad = xb[0] | xb[1];
                }
            } else {
                // ---- pass 2: integer numerators, added to the running sum of the scale each key belongs to
                uint32_t w[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = tlo + (e & 3) + 8 * (e >> 2) + 4 * h2;
                    const float x = vm_exp_le0(p[e] - mx) * AP_W_ONE;        // a power-of-two multiple: exact; <= 2^30
                    w[e] = (uint32_t)(int)__builtin_rintf(x);
                    if (ragged && key >= curL) w[e] = 0u;                    // keys past curL do not exist
                }
                const int thi = ragged ? curL : tlo + 32;
                int lo = tlo;
                for (;;) {
                    const int be = __builtin_amdgcn_readfirstlane(sEnds[bin]);
                    const int hi = be < thi ? be : thi;
                    const bool own = bin == S1 - 1;
                    if (lo == tlo && hi == tlo + 32) {                       // the whole tile lies in this scale
#pragma unroll
                        for (int e = 0; e < 16; ++e) W += w[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int key = tlo + (e & 3) + 8 * (e >> 2) + 4 * h2;
                            W += (key >= lo && key < hi) ? w[e] : 0u;
                        }
                    }
                    if (own) {                                               // near bin: Chebyshev distance of the grid positions <= radius
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int key = tlo + (e & 3) + 8 * (e >> 2) + 4 * h2;
                            const uint32_t tk = (uint32_t)(key - own0);      // (meaningless for key < own0: excluded by `in`; only S1 == 1 can have such keys here)
                            const int ky = (int)((tk * pn_magic) >> 20), kx = (int)tk - ky * pn;       // tk / pn, tk % pn for tk < 4096, pn <= 64
                            const int dy = ky - qy, dx = kx - qx;
                            const bool in = key >= own0 && key >= lo && key < hi && dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
                            Wn += in ? w[e] : 0u;
                        }
                    }
                    if (hi == be) { sW[wave][bin][lane] = W; W = 0ull; ++bin; }
                    lo = hi;
                    if (hi >= thi) break;
                }
                if (it == 2 * ntile - 1) sW[wave][S1][lane] = Wn;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's K pieces of the next tile have landed
        __syncthreads();
    }

    // ---- per query: Z, the shares; the bins of a query are split between its two lanes (bin parity = lane half)
    if (t0 < l) {
        unsigned long long Z = 0ull;
        for (int bb = 0; bb < S1; ++bb) Z += sW[wave][bb][r] + sW[wave][bb][r + 32];
        // a maximum that is not finite makes s - m NaN at the maximal key: such a query counts as a NaN query (and Z >= 2^30 holds for the others)
        const bool isbad = bad != 0u || !(__builtin_fabsf(mx) < INFINITY);
        if (isbad) Z = 1ull;
        if (t < l) {
            int* tok = tokens ? tokens + (int64_t)b * ld_tok_row + (int64_t)hd * ld_tok_head + (int64_t)t * (S1 + 1) : nullptr;
            for (int bb = h2; bb <= S1; bb += 2) {
                const unsigned long long Wb = sW[wave][bb][r] + sW[wave][bb][r + 32];
                const int share = isbad ? -1 : (int)((Wb << AP_SHIFT) / Z);
                if (tok) tok[bb] = share;
                if (!isbad) atomicAdd(&sAcc[bb], (unsigned long long)share);
            }
            if (isbad && h2 == 0) atomicAdd(&sNan, 1);
        }
    }
    __syncthreads();
    if (tid <= S1) atomicAdd(share_sum + (int64_t)b * ld_row + (int64_t)hd * ld_head + tid, sAcc[tid]);
    if (tid == 0) atomicAdd(nan_count + (int64_t)b * H + hd, sNan);
}

// attn.hip's attn_waves: whole 32-query waves, as few idle ones as possible, larger workgroups on ties (the K tiles are staged once per workgroup)
static int ap_waves(int l) {
    const int nq = (l + 31) / 32;
    int best = 4, waste = ((nq + 3) / 4) * 4 - nq;
    for (int nw = 3; nw >= 1; --nw) { const int w = ((nq + nw - 1) / nw) * nw - nq; if (w < waste) { waste = w; best = nw; } }
    return best;
}

static int ap_check(const float* q, const float* kcache, int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1, int pn, int radius,
                    const int64_t* share_sum, const int32_t* nan_count) {
    if (!q || !kcache || !ends || !share_sum || !nan_count) return VARHIP_EINVAL;
    if (B2 <= 0 || l <= 0 || H <= 0 || curL <= 0 || Lmax <= 0 || pn <= 0) return VARHIP_EINVAL;
    if (curL > Lmax || curL > 4096) return VARHIP_EINVAL;
    if (pn > 64 || l != pn * pn || l > curL) return VARHIP_EINVAL;
    if (S1 < 1 || S1 > AP_MAXS) return VARHIP_EINVAL;
    if (ends[0] < 1 || ends[S1 - 1] != curL) return VARHIP_EINVAL;
    for (int i = 1; i < S1; ++i) if (ends[i] <= ends[i - 1]) return VARHIP_EINVAL;
    if (S1 > 1 && ends[S1 - 2] != curL - l) return VARHIP_EINVAL;
    if (radius < 0) return VARHIP_EINVAL;
    if (((uintptr_t)q & 15) || ((uintptr_t)kcache & 15)) return VARHIP_EINVAL;
    if (B2 > 65535 || H > 65535) return VARHIP_EINVAL;
    return 0;
}

extern "C" int varhip_attn_profile_f32(const float* q, const float* kcache, int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1,
                                       int pn, int radius, int64_t* share_sum, int64_t ld_row, int64_t ld_head, int32_t* nan_count,
                                       int32_t* tokens, int64_t ld_tok_row, int64_t ld_tok_head, varhip_stream_t stream) {
    if (int rc = ap_check(q, kcache, B2, l, H, curL, Lmax, ends, S1, pn, radius, share_sum, nan_count)) return rc;
    ApEnds e;
    for (int i = 0; i < AP_MAXS; ++i) e.v[i] = i < S1 ? ends[i] : curL;
    const uint32_t magic = ((1u << 20) + (uint32_t)pn - 1u) / (uint32_t)pn;
    hipStream_t s = (hipStream_t)stream;
    VhScope sc(VH_FAM_ATTN_PROFILE, s, 2.0 * 2.0 * B2 * H * (double)l * curL * 64, 4.0 * B2 * H * (2.0 * curL * 64 + 1.0 * l * 64));
    const int nw = ap_waves(l);
    dim3 grid((l + nw * 32 - 1) / (nw * 32), H, B2);
    unsigned long long* ss = reinterpret_cast<unsigned long long*>(share_sum);
    if (radius > 4096) radius = 4096;
    switch (nw) {
#define VH_AP_LAUNCH(NW_) hipLaunchKernelGGL((k_attn_profile<NW_>), grid, dim3(NW_ * 64), 0, s, q, kcache, e, S1, l, H, curL, Lmax, pn, radius, magic, \
                                             ss, ld_row, ld_head, nan_count, tokens, ld_tok_row, ld_tok_head)
        case 1: VH_AP_LAUNCH(1); break;
        case 2: VH_AP_LAUNCH(2); break;
        case 3: VH_AP_LAUNCH(3); break;
        default: VH_AP_LAUNCH(4); break;
#undef VH_AP_LAUNCH
    }
    return vh_launch_status();
}

// the host twin: the contract of include/var_hip.h in plain host code, query by query (the kernel's bits without a GPU)
extern "C" int varhip_attn_profile_host_f32(const float* q, const float* kcache, int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1,
                                            int pn, int radius, int64_t* share_sum, int64_t ld_row, int64_t ld_head, int32_t* nan_count,
                                            int32_t* tokens, int64_t ld_tok_row, int64_t ld_tok_head) {
    if (int rc = ap_check(q, kcache, B2, l, H, curL, Lmax, ends, S1, pn, radius, share_sum, nan_count)) return rc;
    const int C = H * 64, own0 = curL - l;
    float* s = (float*)malloc(sizeof(float) * (size_t)curL);
    if (!s) return VARHIP_EINVAL;
    for (int b = 0; b < B2; ++b) {
        for (int h = 0; h < H; ++h) {
            const float* K = kcache + ((int64_t)b * H + h) * Lmax * 64;
            for (int t = 0; t < l; ++t) {
                const float* qr = q + ((int64_t)b * l + t) * C + h * 64;
                float m = -INFINITY;
                bool bad = false;
                for (int j = 0; j < curL; ++j) {
                    float a = 0.0f;
                    for (int i = 0; i < 64; ++i) { const int d = (i & ~7) + ((i & 1) << 2) + ((i & 7) >> 1); a = vm_fma(K[(int64_t)j * 64 + d], qr[d], a); }
                    s[j] = a;
                    if (a != a) bad = true; else if (a > m) m = a;
                }
                if (!(__builtin_fabsf(m) < INFINITY)) bad = true;
                int32_t* tok = tokens ? tokens + (int64_t)b * ld_tok_row + (int64_t)h * ld_tok_head + (int64_t)t * (S1 + 1) : nullptr;
                if (bad) {
                    nan_count[(int64_t)b * H + h] += 1;
                    if (tok) for (int bb = 0; bb <= S1; ++bb) tok[bb] = -1;
                    continue;
                }
                uint64_t Wb[AP_MAXS + 1] = {0}, Z = 0;
                const int qy = t / pn, qx = t % pn;
                int bin = 0;
                for (int j = 0; j < curL; ++j) {
                    while (j >= ends[bin]) ++bin;
                    const uint64_t w = (uint64_t)llrintf(vm_exp_le0(s[j] - m) * AP_W_ONE);
                    Wb[bin] += w; Z += w;
                    if (j >= own0) {
                        const int dy = (j - own0) / pn - qy, dx = (j - own0) % pn - qx;
                        if (dy <= radius && -dy <= radius && dx <= radius && -dx <= radius) Wb[S1] += w;
                    }
                }
                for (int bb = 0; bb <= S1; ++bb) {
                    const int32_t share = (int32_t)((Wb[bb] << AP_SHIFT) / Z);
                    if (tok) tok[bb] = share;
                    share_sum[(int64_t)b * ld_row + (int64_t)h * ld_head + bb] += share;
                }
            }
        }
    }
    free(s);
    return 0;
}
