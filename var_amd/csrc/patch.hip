// patch.hip — activation patching (VAR.patch_effects): zero, mean or donor-copy column ranges of an activation matrix in place, between two
// of the launches of one AdaLN block (block.hip).  act is [rows * l][ld] fp32, row r, token t at (r * l + t) * ld; a directive (row, c0, c1,
// src) rewrites act[row][0 .. l - 1][c0 .. c1 - 1]:
//   src == -1   +0.0f
//   src == -2   the column's mean over the row's l tokens: s = act[0][c], s = s + act[t][c] for t = 1 .. l - 1 (fp32, ascending, one rounding
//               per add), m = s / (float)l (a correctly rounded fp32 division; l == 1: m = s, the bits stay)
//   src >= 0    act[src][t][c], token by token
// A bandwidth kernel: 16 bytes per lane, the 64 lanes of a wave on 64 consecutive column groups (1 KiB per request), no LDS, no barrier.
// Grid (directives, token slices, column groups / 64); the 4 waves of a workgroup and the token slices split the tokens of a zero or copy
// directive.  A mean directive is worked by wave 0 of token slice 0 alone: the lane that owns a column group walks t twice, first adding,
// then storing, so the sum has one order and nobody reads a token another wave has already replaced.
#include "common.h"

namespace {
// a directive that names anything outside the matrix is skipped whole (the same test on both sides)
__host__ __device__ inline bool pt_dir_ok(int row, int c0, int c1, int src, int rows, int width) {
    return row >= 0 && row < rows && src >= -2 && src < rows && c0 >= 0 && c1 <= width && c0 < c1 && (c0 & 3) == 0 && (c1 & 3) == 0;
}

inline bool pt_args_ok(const float* act, int64_t ld, int rows, int l, int width, const int32_t* dir, int n_dir) {
    return act && dir && n_dir > 0 && rows > 0 && l > 0 && width > 0 && width <= (1 << 22) && ld >= width && ld % 4 == 0 && (((uintptr_t)act) & 15) == 0;
}
}  // namespace

__global__ void __launch_bounds__(256) k_act_patch(float* __restrict__ act, int64_t ld, int rows, int l, int width, const int32_t* __restrict__ dir) {
    const int32_t* d = dir + 4 * (int64_t)blockIdx.x;
    const int row = d[0], c0 = d[1], c1 = d[2], src = d[3];                // (uniform: scalar loads)
    if (!pt_dir_ok(row, c0, c1, src, rows, width)) return;
    const int col = c0 + 4 * ((int)blockIdx.z * 64 + (int)(threadIdx.x & 63));
    if (col >= c1) return;                                              // c0, c1 are multiples of 4: a column group lies inside or outside
    const int wave = threadIdx.x >> 6;
    float* dst = act + (int64_t)row * l * ld + col;
    if (src == -2) {
        if (blockIdx.y != 0 || wave != 0) return;
        f32x4 s = *reinterpret_cast<const f32x4*>(dst);
        for (int t = 1; t < l; ++t) s = s + *reinterpret_cast<const f32x4*>(dst + (int64_t)t * ld);
        const float n = (float)l;
        const f32x4 m = {s[0] / n, s[1] / n, s[2] / n, s[3] / n};
        for (int t = 0; t < l; ++t) *reinterpret_cast<f32x4*>(dst + (int64_t)t * ld) = m;
        return;
    }
    const int step = 4 * (int)gridDim.y;
    if (src == -1) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int t = (int)blockIdx.y * 4 + wave; t < l; t += step) *reinterpret_cast<f32x4*>(dst + (int64_t)t * ld) = z;
    } else {
        const float* from = act + (int64_t)src * l * ld + col;
        for (int t = (int)blockIdx.y * 4 + wave; t < l; t += step)
            *reinterpret_cast<f32x4*>(dst + (int64_t)t * ld) = *reinterpret_cast<const f32x4*>(from + (int64_t)t * ld);
    }
}

extern "C" int varhip_act_patch_f32(float* act, int64_t ld, int rows, int l, int width, const int32_t* dir, int n_dir, varhip_stream_t stream) {
    if (n_dir == 0) return 0;
    if (!pt_args_ok(act, ld, rows, l, width, dir, n_dir)) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const int gz = (width / 4 + 63) / 64;                                // whole column groups of 4: c1 <= width is a multiple of 4
    if (gz == 0) return 0;                                               // width < 4: every directive is skipped
    const int gy = l >= 64 ? 16 : (l + 3) / 4;                           // 4 tokens per workgroup and step; at most 16 slices
    VhScope sc(VH_FAM_OTHER, st, 0, 0);                                  // (what a launch moves is in its device-side table)
    hipLaunchKernelGGL(k_act_patch, dim3((unsigned)n_dir, (unsigned)gy, (unsigned)gz), dim3(256), 0, st, act, ld, rows, l, width, dir);
    return vh_launch_status();
}

// ---- host twin (no GPU, no HIP call): the directives one after the other, the kernel's operations in the kernel's order -----------------------
// Additions and the division are single correctly rounded fp32 operations on both sides (-ffp-contract=off; nothing here can contract anyway).
extern "C" int varhip_act_patch_host_f32(float* act, int64_t ld, int rows, int l, int width, const int32_t* dir, int n_dir) {
    if (n_dir == 0) return 0;
    if (!pt_args_ok(act, ld, rows, l, width, dir, n_dir)) return VARHIP_EINVAL;
    for (int i = 0; i < n_dir; ++i) {
        const int row = dir[4 * i], c0 = dir[4 * i + 1], c1 = dir[4 * i + 2], src = dir[4 * i + 3];
        if (!pt_dir_ok(row, c0, c1, src, rows, width)) continue;
        float* dst = act + (int64_t)row * l * ld;
        for (int c = c0; c < c1; ++c) {
            if (src == -2) {
                float s = dst[c];
                for (int t = 1; t < l; ++t) s = s + dst[(int64_t)t * ld + c];
                const float m = s / (float)l;
                for (int t = 0; t < l; ++t) dst[(int64_t)t * ld + c] = m;
            } else {
                const float* from = src < 0 ? nullptr : act + (int64_t)src * l * ld;
                for (int t = 0; t < l; ++t) dst[(int64_t)t * ld + c] = from ? from[(int64_t)t * ld + c] : 0.f;
            }
        }
    }
    return 0;
}
