// kvcompact.hip — row compaction of the per-block KV caches (VAR.sample_best_of_pruned) and, at the end of the file, its in-place
// counterpart varhip_kv_resample (VAR.sample_smc), whose header states why no row is both read and written.
//
// varhip_kv_compact: dst[r, h, t, :] = src[idx[r], h, t, :] for r < rows_out, h < H, t < len, on every one of `nbuf` cache pairs laid out
//   [rows][H][Lmax][64] (SamplingEngine.workspace's kc[bi] / vc[bi]; elements of 4 or 2 bytes).  A pure copy: memory bound.
//   * The pointer pairs of all buffers ride in the kernel's argument block (KVC_MAX_BUF pairs, 1.5 KiB), so ONE launch serves the K and V caches of
//     every block up to depth 48 (d36: 72 buffers); a longer list is cut into launches of KVC_MAX_BUF buffers.
//   * The first `len` tokens of the H heads of one row are H runs of len * 64 elements, each contiguous and 16-byte aligned: the runs of one
//     (buffer, row) are cut into tiles of KVC_TILE 16-byte vectors.  A workgroup takes a tile; each lane issues its four loads (one
//     global_load_dwordx4 each, 64 bytes in flight per lane, 16 KiB per workgroup, up to 8 workgroups per CU) before its plain dwordx4 stores.
//   * The grid is min(tiles, 2048) workgroups striding over the tiles: at the row counts this is called with (tens of rows, 32 buffers) that is
//     thousands of tiles, enough for every CU.
//   * buffer, destination row and idx[r] are uniform in a workgroup (scalar registers); a lane's head and offset come from one 32-bit division.
//   * A source row outside [0, rows_src) copies nothing into its destination row (idx lives on the device: the host cannot refuse it).
#include "common.h"

#define KVC_MAX_BUF 96
#define KVC_TILE 1024           // 16-byte vectors per tile: 256 lanes x 4
#define KVC_MAX_GRID 2048

struct KvcPtrs {
    const uint4* src[KVC_MAX_BUF];
    uint4* dst[KVC_MAX_BUF];
};

// vector e of a row's copied part (head e / vpr, vector e % vpr of its run) -> its offset in the row's storage
__device__ __forceinline__ uint32_t kvc_off(uint32_t e, uint32_t vpr, uint32_t spr) {
    const uint32_t h = e / vpr;
    return h * spr + (e - h * vpr);
}

// tile `chunk` of a row's copied part, from row storage s to row storage d (two different rows: they share no byte)
__device__ __forceinline__ void kvc_tile(const uint4* __restrict__ s, uint4* __restrict__ d, uint32_t chunk, uint32_t row_vecs, uint32_t vpr, uint32_t spr) {
    const uint32_t e0 = chunk * KVC_TILE + threadIdx.x;
    if (chunk * KVC_TILE + KVC_TILE <= row_vecs) {           // a whole tile (uniform): the four loads are issued before the first store
        const uint32_t o0 = kvc_off(e0, vpr, spr), o1 = kvc_off(e0 + 256, vpr, spr), o2 = kvc_off(e0 + 512, vpr, spr), o3 = kvc_off(e0 + 768, vpr, spr);
        const uint4 v0 = s[o0], v1 = s[o1], v2 = s[o2], v3 = s[o3];
        d[o0] = v0; d[o1] = v1; d[o2] = v2; d[o3] = v3;
    } else {                                                 // the row's last tile
        for (uint32_t e = e0; e < row_vecs; e += 256) {
            const uint32_t o = kvc_off(e, vpr, spr);
            d[o] = s[o];
        }
    }
}

// vpr: vectors of one (row, head) run that are copied (len * 64 * elem / 16); spr: vectors between two heads in storage (Lmax * 64 * elem / 16)
__global__ __launch_bounds__(256) void k_kv_compact(KvcPtrs p, const int32_t* __restrict__ idx, int rows_src, int rows_out, int H,
                                                    uint32_t vpr, uint32_t spr, uint32_t tiles_per_row, uint32_t tiles) {
    const uint32_t row_vecs = (uint32_t)H * vpr;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t br = tile / tiles_per_row, chunk = tile - br * tiles_per_row;
        const uint32_t buf = br / (uint32_t)rows_out, r = br - buf * (uint32_t)rows_out;
        const int32_t sr = idx[r];
        if (sr < 0 || sr >= rows_src) continue;
        const uint4* __restrict__ s = p.src[buf] + (int64_t)sr * H * spr;
        uint4* __restrict__ d = p.dst[buf] + (int64_t)r * H * spr;
        kvc_tile(s, d, chunk, row_vecs, vpr, spr);
    }
}

extern "C" int varhip_kv_compact(const void* const* src, void* const* dst, int nbuf, const int32_t* idx, int rows_src, int rows_dst,
                                 int rows_out, int H, int Lmax, int len, int elem_bytes, varhip_stream_t stream) {
    if (!src || !dst || !idx || nbuf <= 0 || rows_src <= 0 || rows_dst <= 0 || H <= 0 || Lmax <= 0) return VARHIP_EINVAL;
    if ((elem_bytes != 2 && elem_bytes != 4) || len < 0 || len > Lmax || rows_out < 0 || rows_out > rows_dst) return VARHIP_EINVAL;
    const int64_t spr = (int64_t)Lmax * 64 * elem_bytes / 16, vpr = (int64_t)len * 64 * elem_bytes / 16;
    if ((int64_t)H * spr > 0x7fffffff) return VARHIP_EINVAL;                 // a row's vectors are indexed in 32 bits
    const int64_t src_bytes = (int64_t)rows_src * H * spr * 16, dst_bytes = (int64_t)rows_dst * H * spr * 16;
    for (int i = 0; i < nbuf; ++i)                                           // host arrays of device pointers
        if (!src[i] || !dst[i] || ((uintptr_t)src[i] & 15) || ((uintptr_t)dst[i] & 15)) return VARHIP_EINVAL;
    for (int i = 0; i < nbuf; ++i)
        for (int j = 0; j < nbuf; ++j) {                                     // no source may share a byte with any destination
            const uintptr_t s0 = (uintptr_t)src[i], d0 = (uintptr_t)dst[j];
            if (s0 < d0 + (uintptr_t)dst_bytes && d0 < s0 + (uintptr_t)src_bytes) return VARHIP_EINVAL;
        }
    if (len == 0 || rows_out == 0) return 0;
    const int64_t tiles_per_row = ((int64_t)H * vpr + KVC_TILE - 1) / KVC_TILE;
    const double bytes = 2.0 * nbuf * rows_out * H * (double)vpr * 16;
    if ((int64_t)(nbuf < KVC_MAX_BUF ? nbuf : KVC_MAX_BUF) * rows_out * tiles_per_row > 0x7fffffff) return VARHIP_EINVAL;
    for (int b0 = 0; b0 < nbuf; b0 += KVC_MAX_BUF) {
        const int nb = nbuf - b0 < KVC_MAX_BUF ? nbuf - b0 : KVC_MAX_BUF;
        const int64_t tiles = (int64_t)nb * rows_out * tiles_per_row;
        KvcPtrs p;
        for (int i = 0; i < KVC_MAX_BUF; ++i) {
            p.src[i] = i < nb ? (const uint4*)src[b0 + i] : nullptr;
            p.dst[i] = i < nb ? (uint4*)dst[b0 + i] : nullptr;
        }
        VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 0.0, bytes * nb / nbuf);
        hipLaunchKernelGGL(k_kv_compact, dim3((unsigned)(tiles < KVC_MAX_GRID ? tiles : KVC_MAX_GRID)), dim3(256), 0, (hipStream_t)stream,
                           p, idx, rows_src, rows_out, H, (uint32_t)vpr, (uint32_t)spr, (uint32_t)tiles_per_row, (uint32_t)tiles);
    }
    return vh_launch_status();
}

// ---- varhip_kv_resample: the in-place counterpart (VAR.sample_smc) --------------------------------------------------------
// buf[i][r][h][t][:] = buf[i][idx[r]][h][t][:] for every row r with idx[r] != r, inside the caches themselves.  Why that is safe without a second
// buffer: a row is copied FROM only if it is a fixed point of the table (idx[idx[r]] == idx[r], checked here, on the device, for every row that is
// written), and a row is written only if it is NOT a fixed point (idx[r] != r).  So no row is both read and written by one launch, whatever order
// the workgroups run in; rows that are fixed points are never written and rows that are written are never read.  A row whose entry is out of
// range or whose source is no fixed point is left alone and counted once in *bad (the workgroup that takes tile 0 of buffer 0 of that row adds
// 1 with a global atomic; cut launches count in the first one only).  k_kv_compact's memory shape: the pointer table in the argument block,
// tiles of KVC_TILE vectors, four loads before four stores, a grid striding over the tiles, and a workgroup-uniform skip of identity rows.
struct KvrPtrs {
    uint4* buf[KVC_MAX_BUF];
};

__global__ __launch_bounds__(256) void k_kv_resample(KvrPtrs p, const int32_t* __restrict__ idx, int rows, int H, uint32_t vpr, uint32_t spr,
                                                     uint32_t tiles_per_row, uint32_t tiles, int32_t* __restrict__ bad, int count_bad) {
    const uint32_t row_vecs = (uint32_t)H * vpr;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t br = tile / tiles_per_row, chunk = tile - br * tiles_per_row;
        const uint32_t buf = br / (uint32_t)rows, r = br - buf * (uint32_t)rows;
        const int32_t sr = idx[r];
        if (sr == (int32_t)r) continue;                      // a survivor: neither read as a destination nor written
        if (sr < 0 || sr >= rows || idx[sr] != sr) {         // (idx[sr] is read only for sr inside the table)
            if (count_bad && buf == 0 && chunk == 0 && threadIdx.x == 0) atomicAdd(bad, 1);
            continue;
        }
        uint4* base = p.buf[buf];
        kvc_tile(base + (int64_t)sr * H * spr, base + (int64_t)r * H * spr, chunk, row_vecs, vpr, spr);
    }
}

extern "C" int varhip_kv_resample(void* const* bufs, int nbuf, const int32_t* idx, int rows, int H, int Lmax, int len, int elem_bytes,
                                  int32_t* bad, varhip_stream_t stream) {
    if (!bufs || !idx || !bad || nbuf <= 0 || rows < 0 || H <= 0 || Lmax <= 0) return VARHIP_EINVAL;
    if ((elem_bytes != 2 && elem_bytes != 4) || len < 0 || len > Lmax) return VARHIP_EINVAL;
    const int64_t spr = (int64_t)Lmax * 64 * elem_bytes / 16, vpr = (int64_t)len * 64 * elem_bytes / 16;
    if ((int64_t)H * spr > 0x7fffffff) return VARHIP_EINVAL;                 // a row's vectors are indexed in 32 bits
    const uintptr_t buf_bytes = (uintptr_t)rows * H * spr * 16;
    for (int i = 0; i < nbuf; ++i)                                           // a host array of device pointers
        if (!bufs[i] || ((uintptr_t)bufs[i] & 15)) return VARHIP_EINVAL;
    for (int i = 0; i < nbuf; ++i)
        for (int j = i + 1; j < nbuf; ++j) {                                 // no two buffers may share a byte
            const uintptr_t a = (uintptr_t)bufs[i], b = (uintptr_t)bufs[j];
            if (a == b || (a < b + buf_bytes && b < a + buf_bytes)) return VARHIP_EINVAL;
        }
    if (len == 0 || rows == 0) return 0;
    const int64_t tiles_per_row = ((int64_t)H * vpr + KVC_TILE - 1) / KVC_TILE;
    if ((int64_t)(nbuf < KVC_MAX_BUF ? nbuf : KVC_MAX_BUF) * rows * tiles_per_row > 0x7fffffff) return VARHIP_EINVAL;
    for (int b0 = 0; b0 < nbuf; b0 += KVC_MAX_BUF) {
        const int nb = nbuf - b0 < KVC_MAX_BUF ? nbuf - b0 : KVC_MAX_BUF;
        const int64_t tiles = (int64_t)nb * rows * tiles_per_row;
        KvrPtrs p;
        for (int i = 0; i < KVC_MAX_BUF; ++i) p.buf[i] = i < nb ? (uint4*)bufs[b0 + i] : nullptr;
        VhScope scope(VH_FAM_OTHER, (hipStream_t)stream, 0.0, 2.0 * nb * rows * H * (double)vpr * 16);      // (an upper bound: the rows that move are the device's to know)
        hipLaunchKernelGGL(k_kv_resample, dim3((unsigned)(tiles < KVC_MAX_GRID ? tiles : KVC_MAX_GRID)), dim3(256), 0, (hipStream_t)stream,
                           p, idx, rows, H, (uint32_t)vpr, (uint32_t)spr, (uint32_t)tiles_per_row, (uint32_t)tiles, bad, b0 == 0 ? 1 : 0);
    }
    return vh_launch_status();
}
