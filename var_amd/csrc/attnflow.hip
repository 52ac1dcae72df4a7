// attnflow.hip — rows of softmax(QK^T) for a handful of target tokens, and row vectors pushed through it (VAR.attention_maps,
// VAR.attention_rollout): out = r P with P formed tile by tile from q . k and never stored.  This is the dV = P^T dO half of a flash-attention
// backward pass with the target rows in the place of dO: a KEY tile owns the accumulator and the walk is over the queries, under the
// block-causal limit of every query's scale.
//
// Two kernels (the contract is in include/var_hip.h):
//   k_attn_rowstats  attnprofile.hip's roles (S^T = K_tile . Q^T, a lane owns a query): two walks over the visible key tiles, the exact maximum,
//                    then the sum of vm_exp_le0(s - m) in two partial sums (one per lane half), m and 1 / sum per (row, head, query).
//   k_attn_flow      the roles transposed (S = Q_tile . K^T with MFMA 32x32x2: A = the queries, B = the key fragments in registers), so a LANE owns
//                    one key and its 16 accumulator registers are 16 queries of the 32-query tile: register 4g + j of lane half h = query
//                    8g + 4h + j.  That is exactly the operand layout a second MFMA chain wants for its B side with k = the query: out^T is never
//                    needed, p goes from the score registers straight into acc[s][key] += r[s][t] p[t][key], the 32 queries of a tile in the
//                    4-interleaved order 0,4,1,5,.. that every other dot product of the library has.  A workgroup owns (row, 32 keys); its four
//                    waves take four heads at a time, each with a chain of its own, and wave 0 adds the heads in ascending order: no
//                    floating-point atomics, nothing depends on the launch geometry or on arrival order.
// No LDS staging of Q or K: a lane's fragment is eight 16-byte global loads (the key fragment once per head, the query fragment once per tile).
#include "common.h"

#define AF_MAXS 16              // key scales of one call
#define AF_MAXT 32              // target rows of one call: the rows of one MFMA
#define AF_MAXL 4096
#define AF_NW 4                 // waves per workgroup, both kernels

struct AfEnds { int v[AF_MAXS]; };                                 // ends, padded with Lq

// one past the last key query t sees: ends[i] of its scale (t < Lq; the padding makes the unrolled loop end at Lq)
__device__ __forceinline__ int af_limit(const AfEnds& e, int t) {
    int lim = 0;
#pragma unroll
    for (int i = 0; i < AF_MAXS; ++i) lim = (lim == 0 && t < e.v[i]) ? e.v[i] : lim;
    return lim;
}

// a lane's operand fragment of a 64-channel row: channels 8c + 4h + u, c = 0..7, u = 0..3 (src already points at channel 4h)
__device__ __forceinline__ void af_frag(const float* src, float (&f)[32]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const f32x4 a = *(const f32x4*)(src + c * 8);
        f[c * 4 + 0] = a[0]; f[c * 4 + 1] = a[1]; f[c * 4 + 2] = a[2]; f[c * 4 + 3] = a[3];
    }
}

__device__ __forceinline__ f32x16 af_scores(const float (&a)[32], const float (&b)[32]) {
    f32x16 p = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], (f32x16)(0.f), 0, 0, 0);
#pragma unroll
    for (int i = 1; i < 32; ++i) p = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], p, 0, 0, 0);
    return p;
}

__global__ void __launch_bounds__(AF_NW * 64) k_attn_rowstats(const float* __restrict__ q, const float* __restrict__ kcache, AfEnds ends, int Lq, int H,
                                                              int Lmax, float* __restrict__ m_out, float* __restrict__ rinv_out,
                                                              int* __restrict__ nan_count) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int b = blockIdx.z, hd = blockIdx.y;
    const int t0 = (blockIdx.x * AF_NW + wave) * 32;               // this wave's first query
    if (t0 >= Lq) return;                                          // (no barrier in this kernel)
    const int t = t0 + r, tq = t < Lq ? t : Lq - 1;                // a lane without a query repeats the last one and writes nothing
    const int lim = af_limit(ends, tq);
    const int tl = t0 + 31 < Lq ? t0 + 31 : Lq - 1;
    const int wlim = __builtin_amdgcn_readfirstlane(af_limit(ends, tl));     // the wave's last query sees the most keys
    const int ntile = (wlim + 31) / 32;
    const float* Kc = kcache + ((int64_t)b * H + hd) * Lmax * 64;

    float qf[32];
    af_frag(q + ((int64_t)b * Lq + tq) * (H * 64) + hd * 64 + h2 * 4, qf);

    float mx = -INFINITY, sum = 0.0f;
    unsigned bad = 0u;
    for (int it = 0; it < 2 * ntile; ++it) {
        const int kt = it < ntile ? it : it - ntile;
        int key = kt * 32 + r;
        key = key < wlim ? key : wlim - 1;                         // no key at or beyond the limit is read (wlim <= Lq)
        float kf[32];
        af_frag(Kc + (int64_t)key * 64 + h2 * 4, kf);
        const f32x16 p = af_scores(kf, qf);                        // lane = query r; register e = key 8 (e >> 2) + 4 h2 + (e & 3) of the tile
        if (it < ntile) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kk = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2;
                if (kk < lim) {
                    mx = fmaxf(mx, p[e]);                          // (drops a NaN operand)
                    bad |= (p[e] != p[e]) ? 1u : 0u;
                }
            }
            if (it == ntile - 1) {                                 // both lane halves of a query agree on m and on the flag
                const auto xm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(xm[0]), __uint_as_float(xm[1]));
                const auto xb = __builtin_amdgcn_permlane32_swap(bad, bad, false, false);
                bad = xb[0] | xb[1];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kk = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2;
                const float w = vm_exp_le0(p[e] - mx);
                sum = sum + (kk < lim ? w : 0.0f);                 // + 0 leaves the bits: the same as skipping the key
            }
        }
    }
    const auto xs = __builtin_amdgcn_permlane32_swap(__float_as_uint(sum), __float_as_uint(sum), false, false);
    const float total = __uint_as_float(xs[0]) + __uint_as_float(xs[1]);     // (keys with bit 2 clear) + (keys with bit 2 set)
    const bool isbad = bad != 0u || !(__builtin_fabsf(mx) < INFINITY);
    const bool mine = h2 == 0 && t < Lq;
    if (mine) {
        const int64_t o = ((int64_t)b * H + hd) * Lq + t;
        m_out[o] = mx;
        rinv_out[o] = isbad ? __builtin_nanf("") : 1.0f / total;
    }
    const unsigned long long nb = __ballot(mine && isbad);
    if (lane == 0 && nb) atomicAdd(nan_count + (int64_t)b * H + hd, (int)__popcll(nb));
}

__global__ void __launch_bounds__(AF_NW * 64) k_attn_flow(const float* __restrict__ q, const float* __restrict__ kcache, const float* __restrict__ m,
                                                          const float* __restrict__ rinv, const float* __restrict__ rv, float* __restrict__ out,
                                                          AfEnds ends, int Lq, int H, int Lmax, int T, int per_head, float alpha) {
    __shared__ unsigned short sLim[AF_MAXL + 32];                  // per query: one past its last visible key; 0 for the padding of the last tile
    __shared__ float sAcc[AF_NW][16][64];                          // a round's per-head chains on their way to wave 0

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane & 31, h2 = lane >> 5;
    const int b = blockIdx.y, j0 = blockIdx.x * 32;
    const int key = j0 + rr, keyc = key < Lq ? key : Lq - 1;       // a lane without a key repeats the last one and writes nothing
    const int nqt = (Lq + 31) / 32;
    const int C = H * 64;

    for (int t = tid; t < nqt * 32; t += AF_NW * 64) sLim[t] = (unsigned short)(t < Lq ? af_limit(ends, t) : 0);
    // the first query that sees key j0 (and with it any key of the tile) opens j0's scale: query tiles wholly before it are skipped
    int s0 = 0;
#pragma unroll
    for (int i = 0; i < AF_MAXS; ++i) s0 = ends.v[i] <= j0 ? ends.v[i] : s0;
    const int qt0 = s0 >> 5;
    __syncthreads();

    f32x16 hs = (f32x16)(0.f);                                     // wave 0: the sum over the heads
    for (int h0 = 0; h0 < H; h0 += AF_NW) {
        const int hd = h0 + wave;
        const bool active = hd < H;                                // wave-uniform
        f32x16 acc = (f32x16)(0.f);
        if (active) {
            float kf[32];
            af_frag(kcache + (((int64_t)b * H + hd) * Lmax + keyc) * 64 + h2 * 4, kf);
            const float* mrow = m + ((int64_t)b * H + hd) * Lq;
            const float* irow = rinv + ((int64_t)b * H + hd) * Lq;
            for (int qt = qt0; qt < nqt; ++qt) {
                const int tl = qt * 32 + rr;
                float qf[32];
                af_frag(q + ((int64_t)b * Lq + (tl < Lq ? tl : Lq - 1)) * C + hd * 64 + h2 * 4, qf);
                const f32x16 s = af_scores(qf, kf);                // lane = key rr; register e = query 8 (e >> 2) + 4 h2 + (e & 3) of the tile
                float pv[16], a[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int t = qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2, tc = t < Lq ? t : Lq - 1;
                    const float pe = vm_exp_le0(s[e] - mrow[tc]) * irow[tc];
                    pv[e] = key < (int)sLim[t] ? pe : 0.0f;        // exactly 0 where query t does not see the key
                    a[e] = (rr < T && t < Lq) ? rv[((int64_t)b * T + rr) * Lq + t] : 0.0f;      // as the A side the lane is target row rr
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], pv[e], acc, 0, 0, 0);
            }
            if (per_head) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int s = (e & 3) + 8 * (e >> 2) + 4 * h2;
                    if (s < T && key < Lq) out[(((int64_t)b * H + hd) * T + s) * Lq + key] = acc[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) sAcc[wave][e][lane] = acc[e];
            }
        }
        if (!per_head) {                                           // (kernel-uniform: every wave meets both barriers)
            __syncthreads();
            if (wave == 0) {
                for (int w = 0; w < AF_NW && h0 + w < H; ++w) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) hs[e] = hs[e] + sAcc[w][e][lane];
                }
            }
            __syncthreads();
        }
    }
    if (!per_head && wave == 0) {
        const float invH = 1.0f / (float)H, om = 1.0f - alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int s = (e & 3) + 8 * (e >> 2) + 4 * h2;
            if (s < T && key < Lq) {
                const int64_t o = ((int64_t)b * T + s) * Lq + key;
                out[o] = vm_fma(alpha, hs[e] * invH, om * rv[o]);
            }
        }
    }
}

static int af_check(const float* q, const float* kcache, int B, int Lq, int H, int Lmax, const int32_t* ends, int S1) {
    if (!q || !kcache || !ends) return VARHIP_EINVAL;
    if (B <= 0 || Lq <= 0 || H <= 0 || Lmax <= 0) return VARHIP_EINVAL;
    if (Lq > Lmax || Lq > AF_MAXL) return VARHIP_EINVAL;
    if (S1 < 1 || S1 > AF_MAXS) return VARHIP_EINVAL;
    if (ends[0] < 1 || ends[S1 - 1] != Lq) return VARHIP_EINVAL;
    for (int i = 1; i < S1; ++i) if (ends[i] <= ends[i - 1]) return VARHIP_EINVAL;
    if (((uintptr_t)q & 15) || ((uintptr_t)kcache & 15)) return VARHIP_EINVAL;
    if (B > 65535 || H > 65535) return VARHIP_EINVAL;
    return 0;
}

static int af_check_flow(const float* q, const float* kcache, const float* m, const float* rinv, const float* r, const float* out, int B, int Lq,
                         int H, int Lmax, const int32_t* ends, int S1, int T) {
    if (!m || !rinv || !r || !out || T <= 0 || T > AF_MAXT) return VARHIP_EINVAL;
    return af_check(q, kcache, B, Lq, H, Lmax, ends, S1);
}

static AfEnds af_ends(const int32_t* ends, int S1, int Lq) {
    AfEnds e;
    for (int i = 0; i < AF_MAXS; ++i) e.v[i] = i < S1 ? ends[i] : Lq;
    return e;
}

extern "C" int varhip_attn_rowstats_f32(const float* q, const float* kcache, int B, int Lq, int H, int Lmax, const int32_t* ends, int S1,
                                        float* m, float* rinv, int32_t* nan_count, varhip_stream_t stream) {
    if (!m || !rinv || !nan_count) return VARHIP_EINVAL;
    if (int rc = af_check(q, kcache, B, Lq, H, Lmax, ends, S1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    VhScope sc(VH_FAM_OTHER, s, 2.0 * 2.0 * B * H * (double)Lq * Lq * 64 * 0.5, 4.0 * B * H * (double)Lq * (64 + 64 + 2));
    const int nq = (Lq + 31) / 32;
    hipLaunchKernelGGL(k_attn_rowstats, dim3((nq + AF_NW - 1) / AF_NW, H, B), dim3(AF_NW * 64), 0, s, q, kcache, af_ends(ends, S1, Lq), Lq, H, Lmax,
                       m, rinv, nan_count);
    return vh_launch_status();
}

extern "C" int varhip_attn_flow_f32(const float* q, const float* kcache, const float* m, const float* rinv, const float* r, float* out, int B,
                                    int Lq, int H, int Lmax, const int32_t* ends, int S1, int T, int per_head, float alpha, varhip_stream_t stream) {
    if (int rc = af_check_flow(q, kcache, m, rinv, r, out, B, Lq, H, Lmax, ends, S1, T)) return rc;
    hipStream_t s = (hipStream_t)stream;
    VhScope sc(VH_FAM_OTHER, s, 2.0 * B * H * (double)Lq * Lq * (64 + 32) * 0.5, 4.0 * B * H * (double)Lq * (64 + 64 + 2 + T));
    hipLaunchKernelGGL(k_attn_flow, dim3((Lq + 31) / 32, B), dim3(AF_NW * 64), 0, s, q, kcache, m, rinv, r, out, af_ends(ends, S1, Lq), Lq, H, Lmax,
                       T, per_head ? 1 : 0, alpha);
    return vh_launch_status();
}

// ---- the host twins: the contract of include/var_hip.h in plain host code (the kernels' bits without a GPU) ------------------------------------
static inline float af_score(const float* K, const float* qr) {
    float a = 0.0f;
    for (int i = 0; i < 64; ++i) { const int d = (i & ~7) + ((i & 1) << 2) + ((i & 7) >> 1); a = vm_fma(K[d], qr[d], a); }
    return a;
}

static inline int af_limit_host(const int32_t* ends, int t) {
    int i = 0;
    while (t >= ends[i]) ++i;
    return ends[i];
}

extern "C" int varhip_attn_rowstats_host_f32(const float* q, const float* kcache, int B, int Lq, int H, int Lmax, const int32_t* ends, int S1,
                                             float* m, float* rinv, int32_t* nan_count) {
    if (!m || !rinv || !nan_count) return VARHIP_EINVAL;
    if (int rc = af_check(q, kcache, B, Lq, H, Lmax, ends, S1)) return rc;
    float* s = (float*)malloc(sizeof(float) * (size_t)Lq);
    if (!s) return VARHIP_EINVAL;
    for (int b = 0; b < B; ++b) {
        for (int h = 0; h < H; ++h) {
            const float* K = kcache + ((int64_t)b * H + h) * Lmax * 64;
            for (int t = 0; t < Lq; ++t) {
                const float* qr = q + ((int64_t)b * Lq + t) * (H * 64) + h * 64;
                const int lim = af_limit_host(ends, t);
                float mx = -INFINITY;
                bool bad = false;
                for (int j = 0; j < lim; ++j) {
                    s[j] = af_score(K + (int64_t)j * 64, qr);
                    if (s[j] != s[j]) bad = true; else if (s[j] > mx) mx = s[j];
                }
                if (!(__builtin_fabsf(mx) < INFINITY)) bad = true;
                float part[2] = {0.0f, 0.0f};
                for (int j = 0; j < lim; ++j) part[(j >> 2) & 1] = part[(j >> 2) & 1] + vm_exp_le0(s[j] - mx);
                const int64_t o = ((int64_t)b * H + h) * Lq + t;
                m[o] = mx;
                rinv[o] = bad ? __builtin_nanf("") : 1.0f / (part[0] + part[1]);
                if (bad) nan_count[(int64_t)b * H + h] += 1;
            }
        }
    }
    free(s);
    return 0;
}

extern "C" int varhip_attn_flow_host_f32(const float* q, const float* kcache, const float* m, const float* rinv, const float* r, float* out, int B,
                                         int Lq, int H, int Lmax, const int32_t* ends, int S1, int T, int per_head, float alpha) {
    if (int rc = af_check_flow(q, kcache, m, rinv, r, out, B, Lq, H, Lmax, ends, S1, T)) return rc;
    const int nqt = (Lq + 31) / 32;
    float* p = (float*)malloc(sizeof(float) * (size_t)nqt * 32);               // one key's column of P, the padding queries at 0
    float* hs = per_head ? nullptr : (float*)malloc(sizeof(float) * (size_t)T * Lq);
    if (!p || (!per_head && !hs)) { free(p); free(hs); return VARHIP_EINVAL; }
    const float invH = 1.0f / (float)H, om = 1.0f - alpha;
    for (int b = 0; b < B; ++b) {
        if (hs) for (int64_t i = 0; i < (int64_t)T * Lq; ++i) hs[i] = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float* K = kcache + ((int64_t)b * H + h) * Lmax * 64;
            const float* mrow = m + ((int64_t)b * H + h) * Lq;
            const float* irow = rinv + ((int64_t)b * H + h) * Lq;
            for (int j = 0; j < Lq; ++j) {
                const int j0 = j & ~31;
                int s0 = 0;
                for (int i = 0; i < S1; ++i) if (ends[i] <= j0) s0 = ends[i];
                const int tb = (s0 >> 5) * 32;                                  // the chain starts at the first query tile that is not skipped
                for (int t = tb; t < nqt * 32; ++t) {
                    p[t] = 0.0f;
                    if (t < Lq && j < af_limit_host(ends, t))
                        p[t] = vm_exp_le0(af_score(K + (int64_t)j * 64, q + ((int64_t)b * Lq + t) * (H * 64) + h * 64) - mrow[t]) * irow[t];
                }
                for (int s = 0; s < T; ++s) {
                    const float* rs = r + ((int64_t)b * T + s) * Lq;
                    float acc = 0.0f;
                    for (int t = tb; t < nqt * 32; t += 32)
                        for (int i = 0; i < 32; ++i) {
                            const int tt = t + (i & ~7) + ((i & 1) << 2) + ((i & 7) >> 1);
                            acc = vm_fma(tt < Lq ? rs[tt] : 0.0f, p[tt], acc);
                        }
                    if (per_head) out[(((int64_t)b * H + h) * T + s) * Lq + j] = acc;
                    else hs[(int64_t)s * Lq + j] = hs[(int64_t)s * Lq + j] + acc;
                }
            }
        }
        if (!per_head)
            for (int64_t i = 0; i < (int64_t)T * Lq; ++i) out[(int64_t)b * T * Lq + i] = vm_fma(alpha, hs[i] * invH, om * r[(int64_t)b * T * Lq + i]);
    }
    free(p);
    free(hs);
    return 0;
}
