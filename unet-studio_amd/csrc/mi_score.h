// What the kernels over intensity codes share (kernels_coreg.hip, include/unet_coreg.h; kernels_cowarp.hip, include/unet_cowarp.h):
// a code as read, the integer logarithm L, and the mutual-information score of joint histograms by one block.  Device code only, all
// inlined (kernels_coreg.hip's emitted kernels did not change by the move).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unet {

constexpr int CO_T = 256;        // threads per block of every kernel that scores
constexpr int CO_MAXK = 25;      // UNET_COREG_MAX_MAPS
constexpr int CO_MAXBINS = 32;   // UNET_COREG_MAX_BINS

// a code as read: a value above bins reads as bins ("none")
__device__ __forceinline__ unsigned co_read(const uint8_t* __restrict__ p, int64_t i, unsigned bins) {
    const unsigned v = p[i];
    return v > bins ? bins : v;
}

// L(n): 65536 * log2(n) truncated, in fixed point; L(0) = 0.  16 squarings, each yielding one bit of the fraction
__device__ __forceinline__ int co_ilog(unsigned n) {
    if (n == 0u) return 0;
    const int e = 31 - __clz((int)n);
    unsigned x = n << (31 - e), f = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned long long y = ((unsigned long long)x * x) >> 31;
        if (y >> 32) {
            f = 2u * f + 1u;
            x = (unsigned)(y >> 1);
        } else {
            f = 2u * f;
            x = (unsigned)y;
        }
    }
    return (int)(((unsigned)e << 16) | f);
}

struct CoScoreLds {
    int lr[CO_MAXK * CO_MAXBINS], lc[CO_MAXK * CO_MAXBINS], ln[CO_MAXK];   // L of the row sums, the column sums, the totals
    unsigned rs[CO_MAXK * CO_MAXBINS];                                      // the row sums
    unsigned long long score[CO_MAXK];
};

// Every thread of a CO_T block: sh.score[k] = the score of hist[k], k < K.  Ends on a barrier
__device__ __forceinline__ void co_scores(const uint32_t* __restrict__ hist, int K, int bins, CoScoreLds& sh) {
    const int cols = bins + 1, cells = bins * cols, KB = K * bins;
    for (int e = threadIdx.x; e < 2 * KB; e += CO_T) {   // e < KB: a row sum; otherwise a column sum
        const bool is_row = e < KB;
        const int o = is_row ? e : e - KB, k = o / bins, i = o - k * bins;
        const uint32_t* h = hist + (size_t)k * cells + (is_row ? i * cols : i);
        unsigned sum = 0u;
        const int n = is_row ? cols : bins, stride = is_row ? 1 : cols;
        for (int j = 0; j < n; ++j) sum += h[j * stride];
        if (is_row) {
            sh.rs[o] = sum;
            sh.lr[o] = co_ilog(sum);
        } else {
            sh.lc[o] = co_ilog(sum);
        }
    }
    if ((int)threadIdx.x < K) sh.score[threadIdx.x] = 0ull;
    __syncthreads();
    if ((int)threadIdx.x < K) {
        unsigned total = 0u;
        for (int a = 0; a < bins; ++a) total += sh.rs[threadIdx.x * bins + a];
        sh.ln[threadIdx.x] = co_ilog(total);
    }
    __syncthreads();
    const int inner = bins * bins;   // the cells with b < bins
    for (int k = 0; k < K; ++k) {
        long long part = 0;
        for (int e = threadIdx.x; e < inner; e += CO_T) {
            const int a = e / bins, b = e - a * bins;
            const unsigned n = hist[(size_t)k * cells + a * cols + b];
            if (n) part += (long long)n * (long long)(co_ilog(n) + sh.ln[k] - sh.lr[k * bins + a] - sh.lc[k * bins + b]);
        }
        if (part) atomicAdd(&sh.score[k], (unsigned long long)part);   // two's complement: the wrapped sum is the signed sum
    }
    __syncthreads();
}

}  // namespace unet
