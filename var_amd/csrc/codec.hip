// codec.hip — lossless token coding (VAR.compress / VAR.decompress): the model's guided distribution of a token row as an integer frequency
// table, and the rANS decoder that reads a token out of a word stream with it.  include/var_hip.h states the table and the coder; what this
// file adds is how they are computed.
// k_code_table: one wave per token row, four rows per 256-thread workgroup, no LDS and no barrier.  V % 256 == 0, so lane i owns the float4 at
// element 256 * j + 4 * i of every 256-element chunk j and a pass over the row is V / 256 coalesced 16-byte loads per operand.  Four passes
// (the rows stay in L2 between them): max and NaN; I = sum i_v and v*; the quotients q_v (into cum_out as F_v, where that is asked for) with
// their sum and the token's (C, F); the inclusive prefix in place.  The table is integers from the exponentials on, so neither the lanes'
// order nor the shape of the reductions can change a bit of it.
// The quotient (i_v * K) / I: a float64 estimate corrected by the exact 64-bit remainder.  n = i_v * K < 2^57 and I < 2^46 convert to double
// within 2^-53 relative, the quotient is below 2^24, so the estimate's floor is off by at most one and one correction step makes it exact.
// k_rans_decode: one wave per image, serial over the image's tokens; see the header.
#include "common.h"
#include <string.h>

#define CD_PB VARCODEC_PB
#define CD_TOTAL (1u << CD_PB)
#define CD_MASK (CD_TOTAL - 1u)
#define CD_LOW (1ull << 31)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// i_v of the header: e in [0, 1], the product is exact and non-negative, so the conversion truncates nothing but the fraction
__host__ __device__ static inline uint64_t cd_iv(float e) { return (uint64_t)((double)e * 4294967296.0); }

__device__ __forceinline__ uint64_t cd_div(uint64_t n, uint64_t I, double Id) {
    uint64_t q = (uint64_t)((double)n / Id);
    const int64_t r = (int64_t)(n - q * I);
    if (r < 0) q -= 1;
    else if ((uint64_t)r >= I) q += 1;
    return q;
}

__device__ __forceinline__ uint64_t cd_wave_sum_u64(uint64_t v) {
    for (int off = 32; off >= 1; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off);
    return v;
}
__device__ __forceinline__ uint32_t cd_wave_min_u32(uint32_t v) {
    for (int off = 32; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, off); v = o < v ? o : v; }
    return v;
}

__device__ __forceinline__ f32x4 cd_z4(const float* lc, const float* lu, int e, float ca, float cb) {
    const f32x4 c = *(const f32x4*)(lc + e);
    const f32x4 u = *(const f32x4*)(lu + e);
    const f32x4 a = ca * c;
    const f32x4 b = cb * u;
    return a - b;
}

__global__ void __launch_bounds__(256) k_code_table(const float* __restrict__ logits, int64_t rows, int l, int V, float ca0, float cb0,
                                                    const double* __restrict__ t_rows, const int64_t* __restrict__ gt, int64_t ld,
                                                    uint32_t* cum_out, uint32_t* __restrict__ pair_out, int32_t* __restrict__ flag_out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // row w = b * l + j
    if (w >= rows) return;                                              // (wave-uniform)
    const int64_t b = w / l;
    const int64_t o = b * ld + (w - b * l);
    float ca = ca0, cb = cb0;
    if (t_rows) { const double t = t_rows[b]; ca = (float)(1.0 + t); cb = (float)t; }
    const float* lc = logits + w * V;
    const float* lu = logits + (rows + w) * V;                          // unconditional rows follow the conditional ones
    uint32_t* cum = cum_out ? cum_out + w * V : nullptr;
    const int64_t g = gt ? gt[o] : -1;
    const bool gvalid = g >= 0 && g < V;

    float m = -INFINITY, bad = 0.f;
    for (int e = 4 * lane; e < V; e += 256) {
        const f32x4 z = cd_z4(lc, lu, e, ca, cb);
        m = fmaxf(m, fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
        bad = (z[0] != z[0] || z[1] != z[1] || z[2] != z[2] || z[3] != z[3]) ? 1.f : bad;
    }
    m = vh_wave_max(m);
    bad = vh_wave_max(bad);
    if (bad != 0.f || m == INFINITY || m == -INFINITY) {                // refused (wave-uniform): an ownerless table, a (0, 0) pair
        if (cum)
            for (int e = 4 * lane; e < V; e += 256) *(u32x4*)(cum + e) = (u32x4)(0u);
        if (lane == 0) {
            if (pair_out) { pair_out[2 * o] = 0u; pair_out[2 * o + 1] = 0u; }
            flag_out[o] = 1;
        }
        return;
    }

    uint64_t I = 0;
    uint32_t vs = 0xffffffffu;
    for (int e = 4 * lane; e < V; e += 256) {
        const f32x4 z = cd_z4(lc, lu, e, ca, cb);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            I +=cd_iv(vm_exp(z[c] - m));
            if (z[c] == m && (uint32_t)(e + c) < vs) vs = (uint32_t)(e + c);
        }
    }
    I = cd_wave_sum_u64(I);
    vs = cd_wave_min_u32(vs);

    const uint64_t K = (uint64_t)(CD_TOTAL - (uint32_t)V);
    const double Id = (double)I;
    uint64_t sq = 0, below = 0, qg = 0;
    for (int e = 4 * lane; e < V; e += 256) {
        const f32x4 z = cd_z4(lc, lu, e, ca, cb);
        u32x4 f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t q = cd_div(cd_iv(vm_exp(z[c] - m)) * K, I, Id);
            sq += q;
            if ((int64_t)(e + c) < g) below += 1 + q;
            if ((int64_t)(e + c) == g) qg = q;
            f[c] = (uint32_t)(1 + q);
        }
        if (cum) *(u32x4*)(cum + e) = f;
    }
    sq = cd_wave_sum_u64(sq);
    const uint32_t D = (uint32_t)(K - sq);
    if (pair_out) {
        below = cd_wave_sum_u64(below);
        qg = cd_wave_sum_u64(qg);
        if (lane == 0) {
            pair_out[2 * o] = gvalid ? (uint32_t)below + ((int64_t)vs < g ? D : 0u) : 0u;
            pair_out[2 * o + 1] = gvalid ? (uint32_t)(1 + qg) + ((int64_t)vs == g ? D : 0u) : 0u;
        }
    }
    if (lane == 0) flag_out[o] = (gt && !gvalid) ? 2 : 0;

    if (cum) {                                                          // the inclusive prefix, in place: every lane rereads what it stored
        uint32_t carry = 0;
        for (int e = 4 * lane; e < V; e += 256) {
            u32x4 f = *(u32x4*)(cum + e);
            if (vs - (uint32_t)e < 4u) f[vs - (uint32_t)e] += D;
            f[1] += f[0]; f[2] += f[1]; f[3] += f[2];
            uint32_t incl = f[3];
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
                if (lane >= off) incl += up;
            }
            f += (u32x4)(incl - f[3] + carry);
            *(u32x4*)(cum + e) = f;
            carry += (uint32_t)__shfl((int)incl, 63);
        }
    }
}

static inline bool cd_table_args_ok(const void* logits, int B, int l, int V, const void* gt, int64_t ld, const void* cum_out, const void* pair_out,
                                    const void* flag_out, bool aligned) {
    if (!logits || !flag_out || (!cum_out && !pair_out) || ((gt != nullptr) != (pair_out != nullptr))) return false;
    if (B <= 0 || l <= 0 || V <= 0 || (V & 255) || V > 8192 || ld < l) return false;
    if (aligned && ((((uintptr_t)logits) | ((uintptr_t)cum_out)) & 15)) return false;      // (rows are read and written 16 bytes per lane)
    return true;
}

extern "C" int varhip_code_table_f32(const float* logits, int B, int l, int V, double t_cfg, const double* t_rows, const int64_t* gt, int64_t ld,
                                     uint32_t* cum_out, uint32_t* pair_out, int32_t* flag_out, varhip_stream_t stream) {
    if (!cd_table_args_ok(logits, B, l, V, gt, ld, cum_out, pair_out, flag_out, true)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const float ca = (float)(1.0 + t_cfg), cb = (float)t_cfg;           // as varhip_cfg_sample_f32 rounds them
    VhScope sc(VH_FAM_SAMPLER, st, 0, 4.0 * V * (2.0 + (cum_out ? 1.0 : 0.0)) * (double)rows);
    hipLaunchKernelGGL(k_code_table, dim3((unsigned)blocks), dim3(256), 0, st, logits, rows, l, V, ca, cb, t_rows, gt, ld, cum_out, pair_out, flag_out);
    return vh_launch_status();
}

extern "C" int varhip_code_table_host_f32(const float* logits, int B, int l, int V, double t_cfg, const double* t_rows, const int64_t* gt, int64_t ld,
                                          uint32_t* cum_out, uint32_t* pair_out, int32_t* flag_out) {
    if (!cd_table_args_ok(logits, B, l, V, gt, ld, cum_out, pair_out, flag_out, false)) return VARHIP_EINVAL;
    const int64_t rows = (int64_t)B * l;
    uint64_t* q = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)V);
    if (!q) return VARHIP_EINVAL;
    for (int64_t w = 0; w < rows; ++w) {
        const int64_t b = w / l, o = b * ld + (w - b * l);
        const double t = t_rows ? t_rows[b] : t_cfg;
        const float ca = (float)(1.0 + t), cb = (float)t;
        const float* lc = logits + w * V;
        const float* lu = logits + (rows + w) * V;
        uint32_t* cum = cum_out ? cum_out + w * V : nullptr;
        const int64_t g = gt ? gt[o] : -1;
        const bool gvalid = g >= 0 && g < V;
        auto z = [&](int v) { const float a = ca * lc[v]; const float c = cb * lu[v]; return a - c; };
        float m = -INFINITY;
        bool bad = false;
        for (int v = 0; v < V; ++v) { const float x = z(v); bad = bad || (x != x); if (x > m) m = x; }
        if (bad || m == INFINITY || m == -INFINITY) {
            if (cum) memset(cum, 0, sizeof(uint32_t) * (size_t)V);
            if (pair_out) { pair_out[2 * o] = 0u; pair_out[2 * o + 1] = 0u; }
            flag_out[o] = 1;
            continue;
        }
        uint64_t I = 0;
        int vs = -1;
        for (int v = 0; v < V; ++v) {
            const float x = z(v);
            q[v] = cd_iv(vm_exp(x - m));
            I += q[v];
            if (vs < 0 && x == m) vs = v;
        }
        const uint64_t K = (uint64_t)(CD_TOTAL - (uint32_t)V);
        uint64_t sq = 0;
        for (int v = 0; v < V; ++v) { q[v] = (q[v] * K) / I; sq += q[v]; }
        const uint64_t D = K - sq;
        uint64_t c = 0;
        for (int v = 0; v < V; ++v) {
            const uint64_t f = 1 + q[v] + (v == vs ? D : 0);
            if (pair_out && v == g) { pair_out[2 * o] = (uint32_t)c; pair_out[2 * o + 1] = (uint32_t)f; }
            c += f;
            if (cum) cum[v] = (uint32_t)c;
        }
        if (pair_out && !gvalid) { pair_out[2 * o] = 0u; pair_out[2 * o + 1] = 0u; }
        flag_out[o] = (gt && !gvalid) ? 2 : 0;
    }
    free(q);
    return 0;
}

// ---- the coder ------------------------------------------------------------------------------------------------------------------------------
extern "C" int varhip_rans_encode_host(const uint32_t* pairs, int64_t n, uint32_t* words_out, int64_t cap, int64_t* nwords_out) {
    if (!pairs || !words_out || !nwords_out || n < 0 || cap < 2) return VARHIP_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t C = pairs[2 * i], F = pairs[2 * i + 1];
        if (F == 0 || C + F > CD_TOTAL) return VARHIP_EINVAL;
    }
    uint64_t x = CD_LOW;
    int64_t p = cap;                                                    // the words are laid down from the back: the stream reads forward
    for (int64_t i = n - 1; i >= 0; --i) {
        const uint64_t C = pairs[2 * i], F = pairs[2 * i + 1];
        if (x >= ((CD_LOW >> CD_PB) << 32) * F) {
            if (p <= 2) return VARHIP_EINVAL;                           // (two words are kept for the final state)
            words_out[--p] = (uint32_t)x;
            x >>= 32;
        }
        x = ((x / F) << CD_PB) + x % F + C;
    }
    words_out[--p] = (uint32_t)x;
    words_out[--p] = (uint32_t)(x >> 32);
    memmove(words_out, words_out + p, sizeof(uint32_t) * (size_t)(cap - p));
    *nwords_out = cap - p;
    return 0;
}

// one token of image state (x, pos, err) from the row's inclusive table; SEG = V / 64.  rd(k) reads entry k of the row; ballot(pred_of_lane)
// -> the lowest lane whose predicate holds, or -1: the kernel and the host twin differ in these two alone
template <typename Rd, typename First>
__host__ __device__ static inline int64_t cd_decode_one(uint64_t& x, int64_t& pos, int& err, int V, const uint32_t* wd, int64_t nw, Rd rd, First first) {
    const uint32_t slot = (uint32_t)x & CD_MASK;
    const int SEG = V >> 6;
    const int gseg = first([&](int i) { return rd(SEG * i + SEG - 1) > slot; });
    if (gseg < 0) { err = 2; return -1; }
    int p = -1;
    for (int k = 0; k < SEG && p < 0; k += 64) {
        const int f = first([&](int i) { return k + i < SEG && rd(SEG * gseg + k + i) > slot; });
        if (f >= 0) p = k + f;
    }
    if (p < 0) { err = 2; return -1; }                                  // (cannot happen: the segment's last entry is above the slot)
    const int s = SEG * gseg + p;
    const uint32_t C = s ? rd(s - 1) : 0u;
    if (C > slot) { err = 2; return -1; }                               // (a table that does not ascend: no symbol owns the slot)
    const uint32_t F = rd(s) - C;
    x = (uint64_t)F * (x >> CD_PB) + (slot - C);
    if (x < CD_LOW) {
        if (pos >= nw) { err = 1; return s; }
        x = (x << 32) | wd[pos];
        pos += 1;
    }
    return s;
}

template <typename Rd, typename First>
__host__ __device__ static inline void cd_decode_image(const uint32_t* cum, int l, int V, const uint32_t* words, int64_t words_total, int64_t off,
                                                       int64_t nw, uint32_t* st, int64_t* idx, int32_t* errp, bool writer, Rd rd_of, First first) {
    uint64_t x = (uint64_t)st[0] | ((uint64_t)st[1] << 32);
    int64_t pos = (int64_t)st[2];
    int err = *errp;
    if (!err && (off < 0 || nw < 0 || nw > 0x7fffffff || off > words_total || nw > words_total - off)) err = 3;
    const uint32_t* wd = words + (err == 3 ? 0 : off);
    if (!err && st[3] == 0u) {
        if (nw < 2) err = 1;
        else { x = ((uint64_t)wd[0] << 32) | wd[1]; pos = 2; }
    }
    for (int j = 0; j < l; ++j) {
        int64_t tok = -1;
        if (!err) {
            const uint32_t* row = cum + (int64_t)j * V;
            tok = cd_decode_one(x, pos, err, V, wd, nw, rd_of(row), first);
        }
        if (writer) idx[j] = tok;
    }
    if (writer) {
        st[0] = (uint32_t)x; st[1] = (uint32_t)(x >> 32); st[2] = (uint32_t)pos; st[3] = 1u;
        *errp = err;
    }
}

__global__ void __launch_bounds__(64) k_rans_decode(const uint32_t* __restrict__ cum, int l, int V, const uint32_t* __restrict__ words, int64_t words_total,
                                                    const int64_t* __restrict__ word_off, const int64_t* __restrict__ nwords, uint32_t* state,
                                                    int64_t* __restrict__ idx_out, int32_t* err_out, int B) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= B) return;
    auto first = [&](auto pred) {
        const unsigned long long bal = __ballot(pred(lane) ? 1 : 0);
        return bal ? (int)__ffsll((long long)bal) - 1 : -1;
    };
    auto rd_of = [&](const uint32_t* row) { return [row](int k) { return row[k]; }; };
    cd_decode_image(cum + (int64_t)b * l * V, l, V, words, words_total, word_off[b], nwords[b], state + 4 * b, idx_out + (int64_t)b * l, err_out + b,
                    lane == 0, rd_of, first);
}

static inline bool cd_decode_args_ok(const void* cum, int l, int V, const void* words, int64_t words_total, const void* word_off, const void* nwords,
                                     const void* state, const void* idx_out, const void* err_out, int B) {
    if (!cum || !words || !word_off || !nwords || !state || !idx_out || !err_out) return false;
    return B > 0 && l > 0 && V > 0 && !(V & 255) && V <= 8192 && words_total >= 0;
}

extern "C" int varhip_rans_decode_u32(const uint32_t* cum, int l, int V, const uint32_t* words, int64_t words_total, const int64_t* word_off,
                                      const int64_t* nwords, uint32_t* state, int64_t* idx_out, int32_t* err_out, int B, varhip_stream_t stream) {
    if (!cd_decode_args_ok(cum, l, V, words, words_total, word_off, nwords, state, idx_out, err_out, B)) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    VhScope sc(VH_FAM_SAMPLER, st, 0, 8.0 * l * (double)B);
    hipLaunchKernelGGL(k_rans_decode, dim3((unsigned)B), dim3(64), 0, st, cum, l, V, words, words_total, word_off, nwords, state, idx_out, err_out, B);
    return vh_launch_status();
}

extern "C" int varhip_rans_decode_host(const uint32_t* cum, int l, int V, const uint32_t* words, int64_t words_total, const int64_t* word_off,
                                       const int64_t* nwords, uint32_t* state, int64_t* idx_out, int32_t* err_out, int B) {
    if (!cd_decode_args_ok(cum, l, V, words, words_total, word_off, nwords, state, idx_out, err_out, B)) return VARHIP_EINVAL;
    auto first = [](auto pred) {
        for (int i = 0; i < 64; ++i)
            if (pred(i)) return i;
        return -1;
    };
    auto rd_of = [](const uint32_t* row) { return [row](int k) { return row[k]; }; };
    for (int b = 0; b < B; ++b)
        cd_decode_image(cum + (int64_t)b * l * V, l, V, words, words_total, word_off[b], nwords[b], state + 4 * b, idx_out + (int64_t)b * l, err_out + b,
                        true, rd_of, first);
    return 0;
}
