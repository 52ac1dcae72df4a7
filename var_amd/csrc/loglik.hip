// loglik.hip — teacher-forced class scoring (fork eval_prob.py:441-463, var_analysis.py:322-349): the log-probability of the ground-truth
// token of every (image, class, token) row, reduced from the fp32 logits the head GEMM has just written, with the optional CFG combine.
//   z_v = logits[row][v]                                          (no guidance)
//   z_v = ca * cond[row][v] - cb * uncond[img(row)][v]            (guidance; each product and the difference rounded to fp32)
//   lp  = (z_gt - max z) - log(sum_v exp(z_v - max z))            (torch.log_softmax, then gather)
// A streaming row reduction, bound by the logits' bytes: one wave per row, four rows per 256-thread workgroup, no LDS and no barrier.
// Where the row fits (V <= 256 * NV, V % 4 == 0, 16-byte aligned rows) it is read once with dwordx4 loads into registers and both passes
// (max, then the exponential sum) run there; anything else re-reads the row from the caches for the second pass.
#include "common.h"
#include "rowlse.h"            // the row pass itself, shared with k_token_eval (evalstats.hip)

// NV > 0: the row in NV float4 registers per lane (element j * 256 + 4 * lane + c); NV == 0: any V, scalar loads, two passes over memory
template <int NV, bool CFG>
__global__ void __launch_bounds__(256) k_token_loglik(const float* __restrict__ logits, const int64_t* __restrict__ gt, int64_t ld_gt,
                                                      int images, int classes, int l, int V, float ca, float cb,
                                                      float* __restrict__ out, int64_t ld_oi, int64_t ld_oc) {
    const int lane = threadIdx.x & 63;
    // wave w scores (image, token, class) in that order: the `classes` waves that share one unconditional row run next to each other
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t per_img = (int64_t)l * classes;
    if (w >= per_img * images) return;                                  // (wave-uniform)
    const int img = (int)(w / per_img);
    const int t = (int)((w - img * per_img) / classes);
    const int k = (int)(w - img * per_img - (int64_t)t * classes);
    const float* lc = logits + (((int64_t)img * classes + k) * l + t) * V;
    const float* lu = logits + (((int64_t)images * classes + img) * l + t) * V;      // unconditional rows follow the class rows
    float m, s;
    if constexpr (NV > 0) {
        f32x4 z[NV];
        vh_row_load<NV, CFG>(z, lc, lu, ca, cb, V, lane);
        vh_row_max_expsum<NV>(z, m, s);
    } else {
        vh_row_max_expsum_mem<CFG>(lc, lu, ca, cb, V, lane, m, s);
    }
    s = vh_wave_sum(s);
    if (lane == 0) {
        const int64_t g = gt[(int64_t)img * ld_gt + t];
        // a token outside [0, V) is never read: it scores NaN (the host API rejects such tokens before any launch)
        const float lp = (g >= 0 && g < V) ? vh_row_logp(vh_row_z<CFG>(lc, lu, g, ca, cb), m, s) : NAN;
        out[(int64_t)img * ld_oi + (int64_t)k * ld_oc + t] = lp;
    }
}

template <int NV>
static void ll_launch(bool cfg, dim3 grid, hipStream_t st, const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l,
                      int V, float ca, float cb, float* out, int64_t ld_oi, int64_t ld_oc) {
    if (cfg) hipLaunchKernelGGL((k_token_loglik<NV, true>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, out, ld_oi, ld_oc);
    else hipLaunchKernelGGL((k_token_loglik<NV, false>), grid, dim3(256), 0, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, out, ld_oi, ld_oc);
}

extern "C" int varhip_token_loglik_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                                       int with_uncond, float ca, float cb, float* out, int64_t ld_out_img, int64_t ld_out_cls, varhip_stream_t stream) {
    if (!logits || !gt || !out || images <= 0 || classes <= 0 || l <= 0 || V <= 0 || ld_gt < l || ld_out_cls < l ||
        ld_out_img < (int64_t)classes * ld_out_cls)
        return VARHIP_EINVAL;
    const int64_t rows = (int64_t)images * classes * l;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffff) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && ((uintptr_t)logits & 15) == 0;
    // bytes: every class row once, and with guidance the images' unconditional rows once (re-read by the classes from the caches)
    const double bytes = 4.0 * V * (double)(rows + (with_uncond ? (int64_t)images * l : 0)) + 12.0 * rows;
    VhScope sc(VH_FAM_SAMPLER, st, 0, bytes);
    const dim3 grid((unsigned)blocks);
    if (vec && V <= 1024) ll_launch<4>(with_uncond != 0, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, out, ld_out_img, ld_out_cls);
    else if (vec && V <= 4096) ll_launch<16>(with_uncond != 0, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, out, ld_out_img, ld_out_cls);
    else ll_launch<0>(with_uncond != 0, grid, st, logits, gt, ld_gt, images, classes, l, V, ca, cb, out, ld_out_img, ld_out_cls);
    return vh_launch_status();
}
