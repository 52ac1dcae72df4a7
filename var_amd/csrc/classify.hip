// classify.hip — the pruning step of VAR.classify: per image, add one stage's per-token scores to the candidates' float64 running totals and
// keep the best `keep` candidates under the classification rule.
//   total[c] += tokens[c][t], t = t0 .. t1-1, one plain fp64 addition per token in ascending token order (the library builds with
//   -ffp-contract=off, so np.add.accumulate over float64 reproduces every total bit for bit)
//   rule: higher total first, NaN below everything (-inf included), equal totals (+0 and -0 alike, NaN and NaN alike) by lower index
// One workgroup per image.  Each total becomes a 64-bit key that orders the doubles as the rule does (NaN -> 0), staged in LDS; a candidate's
// rank is the number of candidates that precede it, counted against every key (the key read is a broadcast: all lanes of a wave read the same
// element).  Candidates with rank < keep are kept; their indices are written in ascending order through an exclusive scan of the per-thread
// counts.  At most cand^2 compares per image: not a hot spot (a boundary of VAR.classify at K = 1000 is ~10^6 compares per image).
#include "common.h"

#define CS_THREADS 256
#define CS_MAX_CAND 16384                         // keys: 128 KiB of LDS (+ 1 KiB of counts), below the 160 KiB of a CU
#define CS_PER_THREAD (CS_MAX_CAND / CS_THREADS)  // 64: a thread's kept flags fit one 64-bit mask

// monotone in the rule's order: non-NaN doubles map above 0 in their numeric order with -0 == +0, every NaN maps to 0
__device__ __forceinline__ uint64_t cs_key(double v) {
    if (v != v) return 0ull;
    if (v == 0.0) v = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(CS_THREADS) k_class_select(const float* __restrict__ tokens, int64_t ld_img, int64_t ld_cls, int cand, int t0,
                                                            int t1, double* __restrict__ totals, int keep, int nkept, int32_t* __restrict__ kept) {
    extern __shared__ __attribute__((aligned(16))) uint64_t cs_keys[];
    int* cs_cnt = (int*)(cs_keys + ((cand + 1) & ~1));                  // 16-byte aligned after the keys
    const int img = blockIdx.x, tid = threadIdx.x;
    const int per = (cand + CS_THREADS - 1) / CS_THREADS;               // a contiguous run of candidates per thread (<= 64)
    const int c0 = min(tid * per, cand), c1 = min(c0 + per, cand);
    double* tot = totals + (int64_t)img * cand;
    for (int c = c0; c < c1; ++c) {
        const float* row = tokens + (int64_t)img * ld_img + (int64_t)c * ld_cls;
        double acc = tot[c];
        for (int t = t0; t < t1; ++t) acc = acc + (double)row[t];
        tot[c] = acc;
        cs_keys[c] = cs_key(acc);
    }
    __syncthreads();
    uint64_t mask = 0;
    int n = 0;
    for (int c = c0; c < c1; ++c) {
        const uint64_t kc = cs_keys[c];
        int rank = 0;
        for (int d = 0; d < cand; ++d) {
            const uint64_t kd = cs_keys[d];
            rank += (kd > kc) | ((kd == kc) & (d < c));
        }
        if (rank < keep) { mask |= 1ull << (c - c0); ++n; }
    }
    cs_cnt[tid] = n;
    __syncthreads();
    int off = 0;
    for (int j = 0; j < tid; ++j) off += cs_cnt[j];
    int32_t* out = kept + (int64_t)img * nkept;
    for (int c = c0; c < c1; ++c)
        if ((mask >> (c - c0)) & 1ull) out[off++] = c;
}

extern "C" int varhip_class_select_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int cand, int t0, int t1,
                                       double* totals, int keep, int32_t* kept, varhip_stream_t stream) {
    if (!totals || !kept || images <= 0 || cand <= 0 || cand > CS_MAX_CAND || keep <= 0 || t0 < 0 || t1 < t0 ||
        (t1 > t0 && (!tokens || ld_cls < t1 || ld_img < (int64_t)cand * ld_cls)))
        return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const int nkept = keep < cand ? keep : cand;
    const size_t lds = sizeof(uint64_t) * (size_t)((cand + 1) & ~1) + sizeof(int) * CS_THREADS;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)k_class_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(uint64_t) * CS_MAX_CAND + sizeof(int) * CS_THREADS));
        attr_done = true;
    }
    VhScope sc(VH_FAM_OTHER, st, (double)images * cand * cand, (double)images * cand * (4.0 * (t1 - t0) + 16.0 + 4.0));
    hipLaunchKernelGGL(k_class_select, dim3((unsigned)images), dim3(CS_THREADS), lds, st, tokens, ld_img, ld_cls, cand, t0, t1, totals, keep,
                       nkept, kept);
    return vh_launch_status();
}
