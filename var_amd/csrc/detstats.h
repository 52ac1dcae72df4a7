// detstats.h — the order-free and fixed-order reductions shared by k_vq_scale_stats (vqstats.hip) and the kernels of evalstats.hip.
// Float64 sums: a wave adds its 64 lanes by the xor butterfly 32, 16, 8, 4, 2, 1 (both partners add the same pair: identical bits in every
// lane), a workgroup its four waves as ((w0 + w1) + w2) + w3; no floating-point atomics anywhere.
// Histogram: integer atomics only (integer adds commute: exact and independent of the order of execution), first in the workgroup's LDS
// when the bins fit, then one global integer add per non-zero bin; larger histograms are counted straight in global memory.
#pragma once
#include "common.h"

__device__ __forceinline__ double vh_wave_sum_f64(double p) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    return p;
}
// 256 threads; every thread returns the same value.  red: 4 doubles of LDS.
__device__ __forceinline__ double vh_block_sum256_f64(double p, double* red) {
    p = vh_wave_sum_f64(p);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = p;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

#define VH_HIST_LDS_BINS 8192     // up to this many bins are counted in LDS first (32 KB of uint32)

// A 256-thread workgroup counts the indices at(i), i in [i0, min(i0 + 1024, n_idx)), into hits[0, V).  bins: VH_HIST_LDS_BINS uint32 of LDS.
// An index outside [0, V) is neither dereferenced nor counted; returns how many of them this thread met.  Every thread of the workgroup must
// call it (barriers inside; i0 and V are uniform).
template <typename F>
__device__ __forceinline__ int vh_hist_block1024(F at, int64_t i0, int64_t n_idx, int V, unsigned long long* __restrict__ hits, unsigned int* bins) {
    const int tid = threadIdx.x;
    const bool lds = V <= VH_HIST_LDS_BINS;
    if (lds) {
        for (int v = tid; v < V; v += 256) bins[v] = 0u;
        __syncthreads();
    }
    int nbad = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k * 256 + tid;
        if (i >= n_idx) break;
        const int64_t v = at(i);
        if (v < 0 || v >= (int64_t)V) { ++nbad; continue; }                 // never dereferenced, never counted
        if (lds) atomicAdd(&bins[v], 1u); else atomicAdd(&hits[v], 1ull);
    }
    if (lds) {
        __syncthreads();
        for (int v = tid; v < V; v += 256) { const unsigned int c = bins[v]; if (c) atomicAdd(&hits[v], (unsigned long long)c); }
    }
    return nbad;
}
