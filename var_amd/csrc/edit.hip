// edit.hip — zero-shot image editing (VAR.autoregressive_infer_cfg_with_mask; reference demo_zero_shot_edit.ipynb, cell 2).
//
// varhip_edit_keep_u8: the pixel-grid edit mask resized to every scale in one launch, what replace_embedding's
//   F.interpolate(mask, (pn, pn), mode='bilinear', align_corners=False) > 0.5 computes per scale, with scales of pn * pn <= 3 kept whole.
//   One thread per (row, token) of the (B, L) keep map.  The arithmetic is upsample_bilinear2d's in fp32.  The source coordinate
//   scale * (d + 1/2) - 1/2 is one fused multiply-add, as torch's CPU build evaluates it: rounding the product first moves it onto a tap
//   (P = 16 -> pn = 13, d = 6: 7.5 instead of 7.5000005, so lambda = 1/2 exactly and a 0/1 edge falls to 0); the blend is plain fp32
//   operations in upsample_bilinear2d's order (DESIGN.md §16 records where this agrees with torch).
// varhip_quant_accum_edit_f32 / varhip_quant_accum_h_edit_f32: the quantizer step of quant.hip with the h_BChw replacement of
//   replace_embedding fused into its gather: a kept position reads codebook[gt], the others the sampled token's code (or the more_smooth
//   embedding h).  Phi and the f_hat accumulation are quant.hip's own launch (vh_quant_phi_accum), so the result is bitwise that of
//   token_select_i64 + quant_accum_f32, and of an overwrite of h + quant_accum_h_f32.
#include "common.h"

#define ED_MAX_S 32

struct EdScales {
    int pn[ED_MAX_S];
    int begin[ED_MAX_S + 1];          // token offset of every scale, begin[S] = L
    int S;
};

__global__ void k_edit_keep(const float* __restrict__ mask, int Bm, int h, int w, EdScales sc, int B, uint8_t* __restrict__ keep) {
    const int L = sc.begin[sc.S];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * L) return;
    const int b = (int)(i / L), t = (int)(i - (int64_t)b * L);
    int si = 0;
    while (t >= sc.begin[si + 1]) ++si;
    const int pn = sc.pn[si];
    if (pn * pn <= 3) { keep[i] = 1; return; }
    const int p = t - sc.begin[si], y = p / pn, x = p - y * pn;
    // area_pixel_compute_scale / area_pixel_compute_source_index (align_corners=False) and the four-tap blend of upsample_bilinear2d
    const float sh = (float)h / (float)pn, sw = (float)w / (float)pn;
    float fy = vm_fma(sh, (float)y + 0.5f, -0.5f); fy = fy < 0.f ? 0.f : fy;
    float fx = vm_fma(sw, (float)x + 0.5f, -0.5f); fx = fx < 0.f ? 0.f : fx;
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float l1h = fy - (float)y0, l0h = 1.f - l1h;
    const float l1w = fx - (float)x0, l0w = 1.f - l1w;
    const float* m = mask + (Bm == 1 ? (int64_t)0 : (int64_t)b) * h * w;
    const float x00 = m[(int64_t)y0 * w + x0], x01 = m[(int64_t)y0 * w + x1];
    const float x10 = m[(int64_t)y1 * w + x0], x11 = m[(int64_t)y1 * w + x1];
    const float top = l0w * x00 + l1w * x01;
    const float bot = l0w * x10 + l1w * x11;
    const float v = l0h * top + l1h * bot;
    keep[i] = v > 0.5f ? 1 : 0;
}

extern "C" int varhip_edit_keep_u8(const float* mask, int Bm, int h, int w, const int32_t* patch_nums, int S, int B, uint8_t* keep_out,
                                   varhip_stream_t stream) {
    if (!mask || !patch_nums || !keep_out || B <= 0 || h <= 0 || w <= 0 || S <= 0 || S > ED_MAX_S || (Bm != 1 && Bm != B)) return VARHIP_EINVAL;
    EdScales sc;
    sc.S = S;
    sc.begin[0] = 0;
    for (int s = 0; s < S; ++s) {
        const int pn = patch_nums[s];                   // host array
        if (pn <= 0 || pn > 4096) return VARHIP_EINVAL;
        sc.pn[s] = pn;
        sc.begin[s + 1] = sc.begin[s] + pn * pn;
        if (sc.begin[s + 1] > (1 << 26)) return VARHIP_EINVAL;
    }
    for (int s = S; s < ED_MAX_S; ++s) { sc.pn[s] = 0; sc.begin[s + 1] = sc.begin[S]; }
    const int64_t n = (int64_t)B * sc.begin[S];
    if ((n + 255) / 256 > 0x7fffffff) return VARHIP_EINVAL;
    VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 10.0 * n, 17.0 * n);
    hipLaunchKernelGGL(k_edit_keep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, Bm, h, w, sc, B, keep_out);
    return vh_launch_status();
}

// k_gather_up of quant.hip with the replacement: position pos of row b reads codebook[gt[b * ld + pos]] where keep[b * ld + pos] is set,
// else codebook[idx[b * pn * pn + pos]] (FROM_H: h[b * pn * pn + pos]).  Same taps, same fma chains.
template <bool FROM_H>
__global__ void k_gather_up_edit(const int64_t* __restrict__ idx, const float* __restrict__ h, const uint8_t* __restrict__ keep,
                                 const int64_t* __restrict__ gt, int64_t ld, const float* __restrict__ codebook, const int32_t* __restrict__ tap_idx,
                                 const float* __restrict__ tap_w, float* __restrict__ up, int B, int pn, int P, int Cv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // [B][P][P][Cv]
    if (i >= (int64_t)B * P * P * Cv) return;
    const int c = (int)(i % Cv); int64_t t = i / Cv; const int x = (int)(t % P); t /= P; const int y = (int)(t % P); const int b = (int)(t / P);
    const int64_t base = (int64_t)b * pn * pn, kb = (int64_t)b * ld;
    auto val = [&](int64_t pos) -> float {
        if (keep[kb + pos]) return codebook[gt[kb + pos] * Cv + c];
        return FROM_H ? h[(base + pos) * Cv + c] : codebook[idx[base + pos] * Cv + c];
    };
    if (pn == P) { up[i] = val(y * pn + x); return; }
    const int32_t* iy = tap_idx + y * 4; const float* wy = tap_w + y * 4;
    const int32_t* ix = tap_idx + x * 4; const float* wx = tap_w + x * 4;
    float rr[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t ro = (int64_t)iy[a] * pn;
        float acc = val(ro + ix[0]) * wx[0];
        acc = vm_fma(val(ro + ix[1]), wx[1], acc);
        acc = vm_fma(val(ro + ix[2]), wx[2], acc);
        acc = vm_fma(val(ro + ix[3]), wx[3], acc);
        rr[a] = acc;
    }
    float o = rr[0] * wy[0];
    o = vm_fma(rr[1], wy[1], o); o = vm_fma(rr[2], wy[2], o); o = vm_fma(rr[3], wy[3], o);
    up[i] = o;
}

template <bool FROM_H>
static int quant_accum_edit(const int64_t* idx, const float* h, const uint8_t* keep, const int64_t* gt, int64_t ld, const float* codebook,
                            const int32_t* tap_idx, const float* tap_w, const float* phi_w, const float* phi_b, float ratio, float* up,
                            float* f_hat, int B, int pn, int P, int Cv, hipStream_t stream) {
    if (B <= 0 || pn <= 0 || P <= 0 || pn > P || Cv <= 0 || Cv > 64 || !keep || !gt || !codebook || ld < (int64_t)pn * pn) return VARHIP_EINVAL;
    if ((FROM_H ? !h : !idx) || (pn != P && (!tap_idx || !tap_w))) return VARHIP_EINVAL;
    const int64_t tot = (int64_t)B * P * P * Cv;
    VhScope sc(VH_FAM_OTHER, stream, 2.0 * tot * 9 * Cv, 16.0 * tot);
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_gather_up_edit<FROM_H>, dim3(blocks), dim3(256), 0, stream, idx, h, keep, gt, ld, codebook, tap_idx, tap_w, up, B, pn, P, Cv);
    vh_quant_phi_accum(up, phi_w, phi_b, ratio, f_hat, B, P, Cv, stream);
    return vh_launch_status();
}

extern "C" int varhip_quant_accum_edit_f32(const int64_t* idx, const uint8_t* keep, const int64_t* gt, int64_t ld_gt, const float* codebook,
                                           const int32_t* tap_idx, const float* tap_w, const float* phi_w, const float* phi_b, float ratio,
                                           float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream) {
    return quant_accum_edit<false>(idx, nullptr, keep, gt, ld_gt, codebook, tap_idx, tap_w, phi_w, phi_b, ratio, up, f_hat, B, pn, P, Cv,
                                   (hipStream_t)stream);
}

extern "C" int varhip_quant_accum_h_edit_f32(const float* h, const uint8_t* keep, const int64_t* gt, int64_t ld_gt, const float* codebook,
                                             const int32_t* tap_idx, const float* tap_w, const float* phi_w, const float* phi_b, float ratio,
                                             float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream) {
    return quant_accum_edit<true>(nullptr, h, keep, gt, ld_gt, codebook, tap_idx, tap_w, phi_w, phi_b, ratio, up, f_hat, B, pn, P, Cv,
                                  (hipStream_t)stream);
}
