// smcresample.hip — the resampling decision of VAR.sample_smc: per image, the particles' float64 log-weights take in one
// stage's per-token statistic, the effective sample size decides whether the image resamples, and systematic resampling with one Philox
// uniform per (image, boundary) yields the ancestor table in which survivors keep their own slots (include/var_hip.h states the contract).
//   * One workgroup per image.  What reads memory in bulk and what is independent per particle runs on all lanes: the token sums (particle c
//     on lane c % 256, its tokens in ascending order as the contract has it) and the weights w_c = vm_exp(logw_c - m).
//   * What the contract states as a sequence — the maximum, W and Q, the cumulative sum the thresholds are counted against, the filling of
//     the dead slots — runs on lane 0 over LDS copies, through the very functions the host twin runs (smc_max, smc_steps below): the two
//     sides cannot differ in the order of a single addition.  With n <= SMC_MAX_N that is at most a few thousand dependent LDS operations,
//     twice per sampling call; the particle counts this is called with are 4 to 64.
//   * float64 throughout, plain IEEE operations (the library builds with -ffp-contract=off; f64 division on gfx950 is correctly rounded),
//     vm_exp from include/var_math.h: the kernel and varhip_smc_resample_host_f32 produce the same bits.
#include "common.h"
#include "philox.h"

#define SMC_THREADS 256
#define SMC_MAX_N 2048          // particles per image: lw + w (float64) and the offspring counts (int32) of one image live in 40 KiB of LDS

// step 2: the maximum of the non-NaN log-weights -> true when it exists and is finite (the first of equal maxima is taken: -0 / +0 alike below)
__host__ __device__ static inline bool smc_max(const double* lw, int n, double* m_out) {
    bool any = false;
    double m = 0.0;
    for (int c = 0; c < n; ++c) {
        const double v = lw[c];
        if (v != v) continue;
        if (!any || v > m) { m = v; any = true; }
    }
    *m_out = m;
    return any && m > -__builtin_inf() && m < __builtin_inf();
}

// step 3
__host__ __device__ static inline double smc_weight(double lw, double m) {
    return lw != lw ? 0.0 : (double)vm_exp((float)(lw - m));
}

// steps 4 to 7 on the weights w[n] (o: n ints of scratch) -> did; writes ess, anc and, when the image resamples, the reset log-weights
__host__ __device__ static inline int smc_steps(int n, const double* w, int* o, uint64_t seed, int scale, double ess_frac, int32_t* anc,
                                                double* logw, double* ess_out) {
    double W = 0.0, Q = 0.0;
    for (int c = 0; c < n; ++c) {
        W = W + w[c];
        Q = Q + w[c] * w[c];
    }
    const double ess = W * W / Q;
    *ess_out = ess;
    if (!(ess_frac < 0.0 || ess < ess_frac * (double)n)) {
        for (int c = 0; c < n; ++c) anc[c] = c;
        return 0;
    }
    const VrPhilox r = vr_philox4x32_10(0u, 0u, (uint32_t)scale, 2u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = (double)(2u * (r.w[0] >> 9) + 1u) * 5.9604644775390625e-08;      // (2 (x >> 9) + 1) * 2^-24, exact
    const double step = W / (double)n;
    // T_j = (j + u) * step does not decrease in j and C_c does not decrease in c: the thresholds below C_c that no earlier particle took are
    // exactly those with C_{c-1} <= T_j < C_c
    int j = 0, last = 0;
    double C = 0.0;
    for (int c = 0; c < n; ++c) {
        if (w[c] > 0.0) last = c;
        C = C + w[c];
        int cnt = 0;
        while (j < n && ((double)j + u) * step < C) { ++cnt; ++j; }
        o[c] = cnt;
    }
    o[last] += n - j;                                    // thresholds not below C_{n-1}
    int d = 0;                                           // the next dead slot, ascending
    for (int c = 0; c < n; ++c) {
        if (o[c] < 1) continue;
        anc[c] = c;
        for (int k = o[c] - 1; k > 0; --k) {
            while (d < n && o[d] != 0) ++d;
            if (d >= n) break;                           // (cannot happen: the offspring counts add up to n)
            anc[d++] = c;
        }
    }
    for (int c = 0; c < n; ++c) logw[c] = 0.0;
    return 1;
}

__host__ __device__ static inline double smc_token_sum(const float* row, int t0, int t1) {
    double s = 0.0;
    for (int t = t0; t < t1; ++t) s = s + (double)row[t];
    return s;
}

__global__ void __launch_bounds__(SMC_THREADS) k_smc_resample(const float* __restrict__ tokens, int64_t ld_img, int64_t ld_cls, int n, int t0, int t1,
                                                             double beta, double* __restrict__ logw, const int64_t* __restrict__ seeds, int scale,
                                                             double ess_frac, int32_t* __restrict__ anc, int32_t* __restrict__ did,
                                                             double* __restrict__ ess, double* __restrict__ logw_seen) {
    __shared__ double s_lw[SMC_MAX_N], s_w[SMC_MAX_N];
    __shared__ int s_o[SMC_MAX_N];
    __shared__ double s_m;
    __shared__ int s_ok;
    const int img = blockIdx.x, tid = threadIdx.x;
    double* lw_g = logw + (int64_t)img * n;
    for (int c = tid; c < n; c += SMC_THREADS) {
        const double s = t1 > t0 ? smc_token_sum(tokens + (int64_t)img * ld_img + (int64_t)c * ld_cls, t0, t1) : 0.0;
        const double v = lw_g[c] + beta * s;
        lw_g[c] = v;
        if (logw_seen) logw_seen[(int64_t)img * n + c] = v;
        s_lw[c] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double m;
        s_ok = smc_max(s_lw, n, &m) ? 1 : 0;
        s_m = m;
    }
    __syncthreads();
    int32_t* anc_g = anc + (int64_t)img * n;
    if (!s_ok) {                                         // degenerate (uniform in the workgroup)
        for (int c = tid; c < n; c += SMC_THREADS) anc_g[c] = c;
        if (tid == 0) { did[img] = 0; ess[img] = 0.0; }
        return;
    }
    const double m = s_m;
    for (int c = tid; c < n; c += SMC_THREADS) s_w[c] = smc_weight(s_lw[c], m);
    __syncthreads();
    if (tid == 0) {
        double e;
        did[img] = smc_steps(n, s_w, s_o, (uint64_t)seeds[img], scale, ess_frac, anc_g, lw_g, &e);
        ess[img] = e;
    }
}

static inline bool smc_args_ok(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int n, int t0, int t1, const double* logw,
                               const int64_t* seeds, int scale, const int32_t* anc, const int32_t* did, const double* ess) {
    if (!logw || !seeds || !anc || !did || !ess || images < 1 || n < 1 || n > SMC_MAX_N || t0 < 0 || t1 < t0 || scale < 0) return false;
    if (t1 > t0 && (!tokens || ld_cls < t1 || ld_img < (int64_t)n * ld_cls)) return false;
    return true;
}

extern "C" int varhip_smc_resample_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int n, int t0, int t1, double beta,
                                       double* logw, const int64_t* seeds, int scale, double ess_frac, int32_t* anc, int32_t* did, double* ess,
                                       double* logw_seen, varhip_stream_t stream) {
    if (!smc_args_ok(tokens, ld_img, ld_cls, images, n, t0, t1, logw, seeds, scale, anc, did, ess)) return VARHIP_EINVAL;
    VhScope sc(VH_FAM_OTHER, (hipStream_t)stream, 0.0, (double)images * n * (4.0 * (t1 - t0) + 28.0));
    hipLaunchKernelGGL(k_smc_resample, dim3((unsigned)images), dim3(SMC_THREADS), 0, (hipStream_t)stream, tokens, ld_img, ld_cls, n, t0, t1, beta,
                       logw, seeds, scale, ess_frac, anc, did, ess, logw_seen);
    return vh_launch_status();
}

// ---- host twin (no GPU, no HIP call) ------------------------------------------------------------------------------------------------------
extern "C" int varhip_smc_resample_host_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int n, int t0, int t1, double beta,
                                            double* logw, const int64_t* seeds, int scale, double ess_frac, int32_t* anc, int32_t* did, double* ess,
                                            double* logw_seen) {
    if (!smc_args_ok(tokens, ld_img, ld_cls, images, n, t0, t1, logw, seeds, scale, anc, did, ess)) return VARHIP_EINVAL;
    double* w = (double*)malloc(sizeof(double) * (size_t)n);
    int* o = (int*)malloc(sizeof(int) * (size_t)n);
    if (!w || !o) { free(w); free(o); return VARHIP_EINVAL; }
    for (int img = 0; img < images; ++img) {
        double* lw = logw + (int64_t)img * n;
        int32_t* a = anc + (int64_t)img * n;
        for (int c = 0; c < n; ++c) {
            const double s = t1 > t0 ? smc_token_sum(tokens + (int64_t)img * ld_img + (int64_t)c * ld_cls, t0, t1) : 0.0;
            lw[c] = lw[c] + beta * s;
            if (logw_seen) logw_seen[(int64_t)img * n + c] = lw[c];
        }
        double m;
        if (!smc_max(lw, n, &m)) {
            for (int c = 0; c < n; ++c) a[c] = c;
            did[img] = 0;
            ess[img] = 0.0;
            continue;
        }
        for (int c = 0; c < n; ++c) w[c] = smc_weight(lw[c], m);
        did[img] = smc_steps(n, w, o, (uint64_t)seeds[img], scale, ess_frac, a, lw, &ess[img]);
    }
    free(w);
    free(o);
    return 0;
}
