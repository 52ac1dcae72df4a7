// evidence.hip — the spatial read-out of class scoring (VAR.evidence_maps): per-pixel class evidence from the (N, K, L) per-token
// scores, reduced behind the maps (min / max, arg-max class, margin, won area) and drawn as colour overlays, without holding (N, K, size, size).
//   m[n,k,y,x] = sum over the selected scales s, in increasing order from 0.0f, of  v_s * w_s,
//   v_s = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)   (a b / c d: the four taps of scale s, axis tables built by the caller)
// every product and sum one fp32 rounding (__fmul_rn / __fadd_rn; the library also builds with -ffp-contract=off): both kernels evaluate m with
// the one device function below, and evidence_maps_torch (var_amd/models/var.py) restates it operation by operation.
// k_evidence_reduce: a workgroup owns 256 consecutive pixels of one image and loops over the K classes.  Class k's tokens [first, first + nst)
//   (the selected scales and whatever lies between them) are staged in LDS with coalesced loads, class k + 1 fetched into registers under
//   class k's arithmetic and written to the other buffer: one barrier per class.  Each thread keeps its pixel's min, max, best, second best and
//   best index; min / max leave the workgroup as one integer atomic each on the order-preserving unsigned encoding of the floats (exact, order
//   independent), the won area through an LDS histogram (K <= 4096; beyond that one global integer atomic per pixel).
// k_evidence_overlay: one workgroup per (image, class, 1024 pixels); m is recomputed, normalised with lo / hi, coloured through the table
//   below and blended with the image in float64 as numpy does; four pixels = 12 bytes = three dwords per thread, 4-byte aligned in the whole
//   (N, K, size, size, 3) array: the pixels of a map in front of the first aligned group and behind the last one are stored byte by byte.
#include "common.h"

#define EV_THREADS 256
#define EV_MAX_SCALES 16
#define EV_MAX_STAGE 4096                       // floats of one class's staged tokens (two buffers: 32 KiB of LDS)
#define EV_HIST 4096                            // classes of the LDS area histogram
#define EV_MAX_SIZE 4096

// matplotlib's 'jet' at its 256 entries as (lut[:, :3] * 255).astype(uint8): generated once with matplotlib 3.10.8
// (tests/test_evidence_cpu.py compares it with the installed matplotlib's)
#define EV_JET_VALUES \
      0,   0, 127,   0,   0, 132,   0,   0, 136,   0,   0, 141,   0,   0, 145,   0,   0, 150,   0,   0, 154,   0,   0, 159, \
      0,   0, 163,   0,   0, 168,   0,   0, 172,   0,   0, 177,   0,   0, 182,   0,   0, 186,   0,   0, 191,   0,   0, 195, \
      0,   0, 200,   0,   0, 204,   0,   0, 209,   0,   0, 213,   0,   0, 218,   0,   0, 222,   0,   0, 227,   0,   0, 232, \
      0,   0, 236,   0,   0, 241,   0,   0, 245,   0,   0, 250,   0,   0, 254,   0,   0, 255,   0,   0, 255,   0,   0, 255, \
      0,   0, 255,   0,   4, 255,   0,   8, 255,   0,  12, 255,   0,  16, 255,   0,  20, 255,   0,  24, 255,   0,  28, 255, \
      0,  32, 255,   0,  36, 255,   0,  40, 255,   0,  44, 255,   0,  48, 255,   0,  52, 255,   0,  56, 255,   0,  60, 255, \
      0,  64, 255,   0,  68, 255,   0,  72, 255,   0,  76, 255,   0,  80, 255,   0,  84, 255,   0,  88, 255,   0,  92, 255, \
      0,  96, 255,   0, 100, 255,   0, 104, 255,   0, 108, 255,   0, 112, 255,   0, 116, 255,   0, 120, 255,   0, 124, 255, \
      0, 128, 255,   0, 132, 255,   0, 136, 255,   0, 140, 255,   0, 144, 255,   0, 148, 255,   0, 152, 255,   0, 156, 255, \
      0, 160, 255,   0, 164, 255,   0, 168, 255,   0, 172, 255,   0, 176, 255,   0, 180, 255,   0, 184, 255,   0, 188, 255, \
      0, 192, 255,   0, 196, 255,   0, 200, 255,   0, 204, 255,   0, 208, 255,   0, 212, 255,   0, 216, 255,   0, 220, 254, \
      0, 224, 250,   0, 228, 247,   2, 232, 244,   5, 236, 241,   8, 240, 237,  12, 244, 234,  15, 248, 231,  18, 252, 228, \
     21, 255, 225,  24, 255, 221,  28, 255, 218,  31, 255, 215,  34, 255, 212,  37, 255, 208,  41, 255, 205,  44, 255, 202, \
     47, 255, 199,  50, 255, 195,  54, 255, 192,  57, 255, 189,  60, 255, 186,  63, 255, 183,  66, 255, 179,  70, 255, 176, \
     73, 255, 173,  76, 255, 170,  79, 255, 166,  83, 255, 163,  86, 255, 160,  89, 255, 157,  92, 255, 154,  95, 255, 150, \
     99, 255, 147, 102, 255, 144, 105, 255, 141, 108, 255, 137, 112, 255, 134, 115, 255, 131, 118, 255, 128, 121, 255, 125, \
    124, 255, 121, 128, 255, 118, 131, 255, 115, 134, 255, 112, 137, 255, 108, 141, 255, 105, 144, 255, 102, 147, 255,  99, \
    150, 255,  95, 154, 255,  92, 157, 255,  89, 160, 255,  86, 163, 255,  83, 166, 255,  79, 170, 255,  76, 173, 255,  73, \
    176, 255,  70, 179, 255,  66, 183, 255,  63, 186, 255,  60, 189, 255,  57, 192, 255,  54, 195, 255,  50, 199, 255,  47, \
    202, 255,  44, 205, 255,  41, 208, 255,  37, 212, 255,  34, 215, 255,  31, 218, 255,  28, 221, 255,  24, 224, 255,  21, \
    228, 255,  18, 231, 255,  15, 234, 255,  12, 237, 255,   8, 241, 252,   5, 244, 248,   2, 247, 244,   0, 250, 240,   0, \
    254, 237,   0, 255, 233,   0, 255, 229,   0, 255, 226,   0, 255, 222,   0, 255, 218,   0, 255, 215,   0, 255, 211,   0, \
    255, 207,   0, 255, 203,   0, 255, 200,   0, 255, 196,   0, 255, 192,   0, 255, 189,   0, 255, 185,   0, 255, 181,   0, \
    255, 177,   0, 255, 174,   0, 255, 170,   0, 255, 166,   0, 255, 163,   0, 255, 159,   0, 255, 155,   0, 255, 152,   0, \
    255, 148,   0, 255, 144,   0, 255, 140,   0, 255, 137,   0, 255, 133,   0, 255, 129,   0, 255, 126,   0, 255, 122,   0, \
    255, 118,   0, 255, 115,   0, 255, 111,   0, 255, 107,   0, 255, 103,   0, 255, 100,   0, 255,  96,   0, 255,  92,   0, \
    255,  89,   0, 255,  85,   0, 255,  81,   0, 255,  77,   0, 255,  74,   0, 255,  70,   0, 255,  66,   0, 255,  63,   0, \
    255,  59,   0, 255,  55,   0, 255,  52,   0, 255,  48,   0, 255,  44,   0, 255,  40,   0, 255,  37,   0, 255,  33,   0, \
    255,  29,   0, 255,  26,   0, 255,  22,   0, 254,  18,   0, 250,  15,   0, 245,  11,   0, 241,   7,   0, 236,   3,   0, \
    232,   0,   0, 227,   0,   0, 222,   0,   0, 218,   0,   0, 213,   0,   0, 209,   0,   0, 204,   0,   0, 200,   0,   0, \
    195,   0,   0, 191,   0,   0, 186,   0,   0, 182,   0,   0, 177,   0,   0, 172,   0,   0, 168,   0,   0, 163,   0,   0, \
    159,   0,   0, 154,   0,   0, 150,   0,   0, 145,   0,   0, 141,   0,   0, 136,   0,   0, 132,   0,   0, 127,   0,   0

static const uint8_t EV_JET_HOST[768] = {EV_JET_VALUES};
__device__ const uint8_t EV_JET[768] = {EV_JET_VALUES};

struct EvScales {                               // the selected scales, by value in the kernel arguments
    int ns;
    int pn[EV_MAX_SCALES];
    int off[EV_MAX_SCALES];                     // first token of the scale inside the staged range
    float w[EV_MAX_SCALES];
};

template <int NS> struct EvTaps {               // one pixel's taps: offsets into the staged range and the four axis weights, per scale
    int o00[NS], o01[NS], o10[NS], o11[NS];
    float l0x[NS], l1x[NS], l0y[NS], l1y[NS];
};

// ax_i: [ns][size][2] int32 (i0, i1), ax_l: [ns][size] fp32 l1 (l0 = 1 - l1, one rounding).  Indices are clamped into the scale: whatever the
// tables hold, every offset stays inside the staged range.
template <int NS>
__device__ __forceinline__ void ev_taps(EvTaps<NS>& t, const EvScales& sc, const int* __restrict__ ax_i, const float* __restrict__ ax_l, int size,
                                        int y, int x) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < sc.ns) {
            const int* ai = ax_i + (int64_t)s * size * 2;
            const float* al = ax_l + (int64_t)s * size;
            const int pn = sc.pn[s], hi = pn - 1;
            const int y0 = min(max(ai[2 * y], 0), hi), y1 = min(max(ai[2 * y + 1], 0), hi);
            const int x0 = min(max(ai[2 * x], 0), hi), x1 = min(max(ai[2 * x + 1], 0), hi);
            const float ly = al[y], lx = al[x];
            t.o00[s] = sc.off[s] + y0 * pn + x0; t.o01[s] = sc.off[s] + y0 * pn + x1;
            t.o10[s] = sc.off[s] + y1 * pn + x0; t.o11[s] = sc.off[s] + y1 * pn + x1;
            t.l1x[s] = lx; t.l0x[s] = __fsub_rn(1.0f, lx);
            t.l1y[s] = ly; t.l0y[s] = __fsub_rn(1.0f, ly);
        }
    }
}

// THE map value: both kernels and the torch twin compute exactly this sequence of roundings
template <int NS>
__device__ __forceinline__ float ev_value(const EvTaps<NS>& t, const EvScales& sc, const float* st) {
    float m = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < sc.ns) {
            const float a = st[t.o00[s]], b = st[t.o01[s]], c = st[t.o10[s]], d = st[t.o11[s]];
            const float top = __fadd_rn(__fmul_rn(t.l0x[s], a), __fmul_rn(t.l1x[s], b));
            const float bot = __fadd_rn(__fmul_rn(t.l0x[s], c), __fmul_rn(t.l1x[s], d));
            const float v = __fadd_rn(__fmul_rn(t.l0y[s], top), __fmul_rn(t.l1y[s], bot));
            m = __fadd_rn(m, __fmul_rn(v, sc.w[s]));
        }
    }
    return m;
}

// floats -> unsigned integers in the same order (-inf lowest, +inf highest; -0 below +0), and back
__device__ __forceinline__ uint32_t ev_enc(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ev_dec(uint32_t u) {
    return __uint_as_float((u >> 31) ? (u & 0x7FFFFFFFu) : ~u);
}

__global__ void __launch_bounds__(EV_THREADS) k_evidence_init(uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, int* __restrict__ area, int images,
                                                             int64_t cells) {
    const int64_t i = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < cells) area[i] = 0;
    if (i < images) { lo[i] = 0xFFFFFFFFu; hi[i] = 0u; }
}

__global__ void __launch_bounds__(EV_THREADS) k_evidence_decode(uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, int images) {
    const int i = blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < images) {
        ((float*)lo)[i] = ev_dec(lo[i]);
        ((float*)hi)[i] = ev_dec(hi[i]);
    }
}

template <int NS, int R>
__global__ void __launch_bounds__(EV_THREADS) k_evidence_reduce(const float* __restrict__ scores, int64_t ld_img, int64_t ld_cls, int K, EvScales sc,
                                                               int first, int nst, const int* __restrict__ ax_i, const float* __restrict__ ax_l,
                                                               int size, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi,
                                                               int* __restrict__ pred, float* __restrict__ margin, int* __restrict__ area,
                                                               float* __restrict__ maps) {
    __shared__ float st[2][EV_THREADS * R];
    __shared__ int hist[EV_HIST];
    __shared__ float red[8];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int npix = size * size;
    const int p = blockIdx.x * EV_THREADS + tid;
    const bool live = p < npix;
    const int pc = live ? p : npix - 1;                           // threads past the image compute its last pixel and commit nothing
    const int y = pc / size, x = pc - y * size;
    EvTaps<NS> t;
    ev_taps<NS>(t, sc, ax_i, ax_l, size, y, x);
    const bool lds_hist = K <= EV_HIST;
    if (lds_hist)
        for (int i = tid; i < K; i += EV_THREADS) hist[i] = 0;
    const float* row = scores + (int64_t)n * ld_img + first;
    float pf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + EV_THREADS * r;
        st[0][i] = i < nst ? row[i] : 0.0f;
    }
    __syncthreads();
    const float inf = __builtin_inff();
    float mn = inf, mx = -inf, best = -inf, second = -inf;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
        const bool more = k + 1 < K;
        if (more) {                                               // class k + 1 on its way while class k is evaluated
            const float* nr = row + (int64_t)(k + 1) * ld_cls;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = tid + EV_THREADS * r;
                pf[r] = i < nst ? nr[i] : 0.0f;
            }
        }
        const float m = ev_value<NS>(t, sc, st[k & 1]);
        mn = fminf(mn, m); mx = fmaxf(mx, m);
        if (m > best) { second = best; best = m; bi = k; }        // strict: the lowest index wins an exact tie
        else if (m > second) second = m;
        if (maps && live) maps[((int64_t)n * K + k) * npix + p] = m;
        if (more) {
#pragma unroll
            for (int r = 0; r < R; ++r) st[(k + 1) & 1][tid + EV_THREADS * r] = pf[r];
        }
        __syncthreads();                                          // buffer (k + 1) & 1 is full, every read of buffer k & 1 is done
    }
    if (live) {
        pred[(int64_t)n * npix + p] = bi;
        margin[(int64_t)n * npix + p] = __fsub_rn(best, second);  // K == 1: best - (-inf) = +inf
        if (lds_hist) atomicAdd(&hist[bi], 1);
        else atomicAdd(&area[(int64_t)n * K + bi], 1);
    } else {
        mn = inf; mx = -inf;
    }
    mx = vh_wave_max(mx);
    mn = -vh_wave_max(-mn);
    if ((tid & 63) == 0) { red[tid >> 6] = mx; red[4 + (tid >> 6)] = mn; }
    __syncthreads();
    if (tid == 0) {
        atomicMax(&hi[n], ev_enc(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
        atomicMin(&lo[n], ev_enc(fminf(fminf(red[4], red[5]), fminf(red[6], red[7]))));
    }
    if (lds_hist)
        for (int i = tid; i < K; i += EV_THREADS) {
            const int c = hist[i];
            if (c) atomicAdd(&area[(int64_t)n * K + i], c);
        }
}

// one pixel of one class map -> its three overlay bytes
template <int NS>
__device__ __forceinline__ void ev_pixel(uint8_t* rgb, int p, int n, const EvScales& sc, const float* st, const uint8_t* jet,
                                         const int* __restrict__ ax_i, const float* __restrict__ ax_l, int size, float lo, float range,
                                         const float* __restrict__ image, int pm1, double alpha, double oma) {
    const int y = p / size, x = p - y * size;
    EvTaps<NS> t;
    ev_taps<NS>(t, sc, ax_i, ax_l, size, y, x);
    const float m = ev_value<NS>(t, sc, st);
    float v = __fsub_rn(m, lo);
    if (range != 0.0f) v = __fdiv_rn(v, range);
    const int bin = (int)fminf(fmaxf(__fmul_rn(v, 256.0f), 0.0f), 255.0f);      // min(int(v * 256), 255); a NaN lands in bin 0
    const int64_t npix = (int64_t)size * size;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = image[((int64_t)n * 3 + c) * npix + p];
        if (pm1) f = __fdiv_rn(__fadd_rn(f, 1.0f), 2.0f);
        const double i8 = (double)(int)fminf(fmaxf(__fmul_rn(f, 255.0f), 0.0f), 255.0f);   // the image as uint8, truncated
        const double o = __dadd_rn(__dmul_rn(i8, oma), __dmul_rn((double)jet[bin * 3 + c], alpha));
        rgb[c] = (uint8_t)(int)fmin(fmax(o, 0.0), 255.0);
    }
}

template <int NS, int R>
__global__ void __launch_bounds__(EV_THREADS) k_evidence_overlay(const float* __restrict__ scores, int64_t ld_img, int64_t ld_cls, int K, EvScales sc,
                                                                int first, int nst, const int* __restrict__ ax_i, const float* __restrict__ ax_l,
                                                                int size, const float* __restrict__ lo, const float* __restrict__ hi,
                                                                const float* __restrict__ image, int pm1, double alpha, uint8_t* __restrict__ out) {
    __shared__ float st[EV_THREADS * R];
    __shared__ uint8_t jet[768];
    const int j = blockIdx.x, n = j / K, k = j - n * K, tid = threadIdx.x;
    const float* row = scores + (int64_t)n * ld_img + (int64_t)k * ld_cls + first;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + EV_THREADS * r;
        st[i] = i < nst ? row[i] : 0.0f;
    }
    for (int i = tid; i < 768; i += EV_THREADS) jet[i] = EV_JET[i];
    __syncthreads();
    const int npix = size * size;
    const int64_t g0 = (int64_t)j * npix;                          // the map's first pixel in the whole output
    const int head = min((int)((4 - (g0 & 3)) & 3), npix);         // pixels in front of the first 4-byte aligned group of four
    const int nq = (npix - head) >> 2, tail0 = head + 4 * nq;
    const float lo_n = lo[n], range = __fsub_rn(hi[n], lo_n);
    const double oma = __dsub_rn(1.0, alpha);
    const int q = blockIdx.y * EV_THREADS + tid;
    if (q < nq) {
        const int p0 = head + 4 * q;
        uint8_t b[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) ev_pixel<NS>(b + 3 * i, p0 + i, n, sc, st, jet, ax_i, ax_l, size, lo_n, range, image, pm1, alpha, oma);
        uint32_t* dst = (uint32_t*)(out + (g0 + p0) * 3);          // (g0 + p0) % 4 == 0
        dst[0] = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
        dst[1] = b[4] | b[5] << 8 | b[6] << 16 | (uint32_t)b[7] << 24;
        dst[2] = b[8] | b[9] << 8 | b[10] << 16 | (uint32_t)b[11] << 24;
    }
    if (blockIdx.y == 0) {                                         // at most three pixels in front, at most three behind
        int p = -1;
        if (tid < head) p = tid;
        else if (tid >= 4 && tid - 4 < npix - tail0) p = tail0 + tid - 4;
        if (p >= 0) {
            uint8_t b[3];
            ev_pixel<NS>(b, p, n, sc, st, jet, ax_i, ax_l, size, lo_n, range, image, pm1, alpha, oma);
            uint8_t* dst = out + (g0 + p) * 3;
            dst[0] = b[0]; dst[1] = b[1]; dst[2] = b[2];
        }
    }
}

// the host arrays of a call -> EvScales, the staged range and the template bucket (0: <= 5 scales in <= 256 floats, 1: <= 10 in <= 768,
// 2: <= 16 in <= 4096); -1: refused
static int ev_setup(EvScales& sc, int& first, int& nst, int nscales, const int* pn, const int* begin, const float* w, int64_t ld_cls) {
    if (!pn || !begin || !w || nscales < 1 || nscales > EV_MAX_SCALES) return -1;
    int64_t end = -1;
    for (int s = 0; s < nscales; ++s) {
        if (pn[s] < 1 || pn[s] > 64 || begin[s] < 0 || (int64_t)begin[s] < end || !(w[s] == w[s])) return -1;
        end = (int64_t)begin[s] + pn[s] * pn[s];
    }
    if (end > ld_cls || end - begin[0] > EV_MAX_STAGE) return -1;
    first = begin[0]; nst = (int)(end - begin[0]);
    sc.ns = nscales;
    for (int s = 0; s < EV_MAX_SCALES; ++s) {
        sc.pn[s] = s < nscales ? pn[s] : 1;
        sc.off[s] = s < nscales ? begin[s] - first : 0;
        sc.w[s] = s < nscales ? w[s] : 0.0f;
    }
    return (nscales <= 5 && nst <= 256) ? 0 : (nscales <= 10 && nst <= 768) ? 1 : 2;
}

extern "C" int varhip_evidence_reduce_f32(const float* scores, int64_t ld_img, int64_t ld_cls, int images, int classes,
                                          int nscales, const int* pn, const int* begin, const float* w,
                                          const int* ax_i, const float* ax_l, int size,
                                          float* lo, float* hi, int* pred, float* margin, int* area, float* maps, varhip_stream_t stream) {
    if (!scores || !ax_i || !ax_l || !lo || !hi || !pred || !margin || !area || images < 1 || images > 65535 || classes < 1 ||
        size < 1 || size > EV_MAX_SIZE || ld_cls < 1 || ld_img < (int64_t)classes * ld_cls)
        return VARHIP_EINVAL;
    EvScales sc;
    int first = 0, nst = 0;
    const int bucket = ev_setup(sc, first, nst, nscales, pn, begin, w, ld_cls);
    if (bucket < 0) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)images * classes;
    const int npix = size * size;
    VhScope scope(VH_FAM_OTHER, st, 11.0 * nscales * cells * npix, 4.0 * cells * nst + 8.0 * images * npix + (maps ? 4.0 * cells * npix : 0.0));
    uint32_t* lo_u = (uint32_t*)lo;
    uint32_t* hi_u = (uint32_t*)hi;
    hipLaunchKernelGGL(k_evidence_init, dim3((unsigned)((cells + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, st, lo_u, hi_u, area, images, cells);
    const dim3 grid((unsigned)((npix + EV_THREADS - 1) / EV_THREADS), (unsigned)images);
#define EV_REDUCE(NS, R) hipLaunchKernelGGL((k_evidence_reduce<NS, R>), grid, dim3(EV_THREADS), 0, st, scores, ld_img, ld_cls, classes, sc, first, nst, \
                                            ax_i, ax_l, size, lo_u, hi_u, pred, margin, area, maps)
    if (bucket == 0) EV_REDUCE(5, 1);
    else if (bucket == 1) EV_REDUCE(10, 3);
    else EV_REDUCE(16, 16);
#undef EV_REDUCE
    hipLaunchKernelGGL(k_evidence_decode, dim3((unsigned)((images + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, st, lo_u, hi_u, images);
    return vh_launch_status();
}

extern "C" int varhip_evidence_overlay_u8(const float* scores, int64_t ld_img, int64_t ld_cls, int images, int classes,
                                          int nscales, const int* pn, const int* begin, const float* w,
                                          const int* ax_i, const float* ax_l, int size,
                                          const float* lo, const float* hi, const float* image, int image_pm1, double alpha,
                                          uint8_t* out, varhip_stream_t stream) {
    if (!scores || !ax_i || !ax_l || !lo || !hi || !image || !out || images < 1 || classes < 1 || (int64_t)images * classes > 0x7FFFFFFF ||
        size < 1 || size > EV_MAX_SIZE || ld_cls < 1 || ld_img < (int64_t)classes * ld_cls || !(alpha >= 0.0 && alpha <= 1.0) ||
        (image_pm1 != 0 && image_pm1 != 1))
        return VARHIP_EINVAL;
    EvScales sc;
    int first = 0, nst = 0;
    const int bucket = ev_setup(sc, first, nst, nscales, pn, begin, w, ld_cls);
    if (bucket < 0) return VARHIP_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)images * classes;
    const int npix = size * size;
    VhScope scope(VH_FAM_OTHER, st, 11.0 * nscales * cells * npix, 4.0 * cells * nst + 12.0 * images * npix + 3.0 * cells * npix);
    const int groups = npix / 4 > 0 ? npix / 4 : 1;
    const dim3 grid((unsigned)cells, (unsigned)((groups + EV_THREADS - 1) / EV_THREADS));
#define EV_OVERLAY(NS, R) hipLaunchKernelGGL((k_evidence_overlay<NS, R>), grid, dim3(EV_THREADS), 0, st, scores, ld_img, ld_cls, classes, sc, first, nst, \
                                             ax_i, ax_l, size, lo, hi, image, image_pm1, alpha, out)
    if (bucket == 0) EV_OVERLAY(5, 1);
    else if (bucket == 1) EV_OVERLAY(10, 3);
    else EV_OVERLAY(16, 16);
#undef EV_OVERLAY
    return vh_launch_status();
}

// the colour table as the kernels hold it: 768 bytes, (entry, channel); a plain host function
extern "C" int varhip_evidence_jet_host(uint8_t* out) {
    if (!out) return VARHIP_EINVAL;
    for (int i = 0; i < 768; ++i) out[i] = EV_JET_HOST[i];
    return 0;
}
