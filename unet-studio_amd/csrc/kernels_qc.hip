// Quality control (qc.cpp:86-135, shift_subject_label train.cpp:248-256) in one streaming pass over the level-0 logits:
// label shift + cast + validity, the collapsed candidates, argmax, and the two per-class histograms of qc.cpp:119-135.
//
// The counts are integers, so any summation order gives the same result.  Every block owns one column of uint32 partial counts
// in the caller's scratch (layout [value][block], value = voxels[0..C') then wrong[0..C')); a second launch sums each value over
// the blocks and WRITES the uint64 result.  There is no global atomic shared between blocks: most voxels land in one class
// (background), and same-address atomics from every block serialise (folded statistics rows).
//
// Inside a block the per-voxel bins are accumulated by one of three schemes, picked by the merged class count C':
//   REG  (C' <= 8):    per-lane register counters, summed over the wave by shuffles and over the 4 waves through LDS at the end
//   LDS  (C' <= 4096): a block histogram in LDS; lanes of a wave with the same (bin, wrong) key add once, by the leader lane
//   GMEM (larger):     the same wave-aggregated adds, straight into the block's own column of the scratch (no other block touches it)
#include "device_util.h"

namespace unet {

namespace {

constexpr int QC_T = 256;            // threads per block
constexpr int QC_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; the grid strides over the rest
constexpr int QC_REG = 8;            // register counters up to this many merged classes
constexpr int QC_LDS = 4096;         // LDS histogram up to this many (2 x 4096 x 4 B = 32 KB)
enum { QC_MODE_REG = 0, QC_MODE_LDS = 1, QC_MODE_GMEM = 2 };

template <int VEC> __device__ __forceinline__ void ldv(const float* __restrict__ p, int64_t i, float (&x)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = *(const float4*)(p + i);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = p[i];
    }
}

// torch.argmax order: a candidate replaces the best one when it is larger or NaN, unless the best one already is NaN (first NaN wins,
// first index wins a tie).  The same rule is torch.amax's NaN propagation.
__device__ __forceinline__ bool qc_takes(float x, float best) { return !(best != best) && !(x <= best); }

// bin t' in [0, C') of one voxel, or -1 when its label is not a class (qc.cpp:86,103,113-114)
__device__ __forceinline__ int qc_bin(float l, float img, int C, int k, int shift) {
    if (shift > 0) l = l != 0.f ? l + (float)shift : (img > 0.f ? 1.f : 0.f);   // train.cpp:251-255, in float
    if (!(l > -1.f && l < (float)C)) return -1;                                   // (int64)l outside [0, C); NaN too
    const int t = (int)l;                                                         // .to(torch::kLong): toward zero
    return k ? max(t - k + 1, 0) : t;
}

// argmax over [lse(l_0..l_{k-1}), l_k, .., l_{C-1}] (k > 0) or [l_0, .., l_{C-1}] for VEC consecutive voxels from v
template <int VEC>
__device__ __forceinline__ void qc_argmax(const float* __restrict__ lg, int64_t S, int64_t v, int C, int k, int (&arg)[VEC]) {
    float best[VEC], x[VEC];
    int c0 = 1;
    if (k) {   // torch::logsumexp: amax (NaN propagates), an infinite max replaced by 0, then max + log(sum(exp(x - max)))
        float mx[VEC], s[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) { mx[j] = -INFINITY; s[j] = 0.f; }
#pragma unroll 4
        for (int c = 0; c < k; ++c) {
            ldv<VEC>(lg, (int64_t)c * S + v, x);
#pragma unroll
            for (int j = 0; j < VEC; ++j) mx[j] = qc_takes(x[j], mx[j]) ? x[j] : mx[j];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) mx[j] = fabsf(mx[j]) == INFINITY ? 0.f : mx[j];
#pragma unroll 4
        for (int c = 0; c < k; ++c) {
            ldv<VEC>(lg, (int64_t)c * S + v, x);
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] += __expf(x[j] - mx[j]);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) best[j] = mx[j] + __logf(s[j]);
        c0 = k;
    } else {
        ldv<VEC>(lg, v, best);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) arg[j] = 0;
#pragma unroll 4
    for (int c = c0; c < C; ++c) {
        ldv<VEC>(lg, (int64_t)c * S + v, x);
        const int i = c - c0 + 1;
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (qc_takes(x[j], best[j])) { best[j] = x[j]; arg[j] = i; }
    }
}

template <int VEC, int MODE>
__global__ void __launch_bounds__(QC_T) k_qc_partial(const float* __restrict__ logits, const float* __restrict__ label,
                                                     const float* __restrict__ image0, int C, int k, int shift, int64_t S,
                                                     unsigned* __restrict__ partial) {
    extern __shared__ unsigned qsh[];   // LDS: the block histogram [2 C']; REG: the 4 waves' sums [4][2 QC_REG]
    const int Cp = k ? C - k + 1 : C, nblk = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned nv[QC_REG], nw[QC_REG];
#pragma unroll
    for (int c = 0; c < QC_REG; ++c) { nv[c] = 0; nw[c] = 0; }
    if constexpr (MODE == QC_MODE_LDS)
        for (int i = threadIdx.x; i < 2 * Cp; i += QC_T) qsh[i] = 0;
    if constexpr (MODE == QC_MODE_GMEM)
        for (int i = threadIdx.x; i < 2 * Cp; i += QC_T) partial[(int64_t)i * nblk + blockIdx.x] = 0;
    if constexpr (MODE != QC_MODE_REG) __syncthreads();

    // block-uniform trip count: the wave-aggregated adds below use ballots over all 64 lanes
    const int64_t step = (int64_t)nblk * QC_T * VEC;
    for (int64_t base = (int64_t)blockIdx.x * QC_T * VEC; base < S; base += step) {
        const int64_t v = base + (int64_t)threadIdx.x * VEC;   // VEC == 4 only when S % 4 == 0: a group is wholly in or out
        int bin[VEC], arg[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) { bin[j] = -1; arg[j] = 0; }
        if (v < S) {
            float l[VEC], im[VEC];
            ldv<VEC>(label, v, l);
            if (shift > 0) ldv<VEC>(image0, v, im);
            else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) im[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) bin[j] = qc_bin(l[j], im[j], C, k, shift);
            qc_argmax<VEC>(logits, S, v, C, k, arg);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int b = bin[j];
            const bool wrong = b >= 0 && arg[j] != b;   // qc.cpp:127-131 (invalid voxels: the dropped bin C')
            if constexpr (MODE == QC_MODE_REG) {
#pragma unroll
                for (int c = 0; c < QC_REG; ++c) {
                    nv[c] += b == c ? 1u : 0u;
                    nw[c] += (b == c && wrong) ? 1u : 0u;
                }
            } else {
                const int key = b < 0 ? -1 : 2 * b + (wrong ? 1 : 0);
                unsigned long long todo = __ballot(key >= 0);
                while (todo) {   // wave-uniform: one add per distinct key of the wave
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lk = __shfl(key, leader);
                    const unsigned long long same = __ballot(key == lk);
                    if (lane == leader) {
                        const unsigned n = (unsigned)__popcll(same);
                        if constexpr (MODE == QC_MODE_LDS) {
                            atomicAdd(&qsh[lk >> 1], n);
                            if (lk & 1) atomicAdd(&qsh[Cp + (lk >> 1)], n);
                        } else {
                            atomicAdd(&partial[(int64_t)(lk >> 1) * nblk + blockIdx.x], n);
                            if (lk & 1) atomicAdd(&partial[(int64_t)(Cp + (lk >> 1)) * nblk + blockIdx.x], n);
                        }
                    }
                    todo &= ~same;
                }
            }
        }
    }

    if constexpr (MODE == QC_MODE_REG) {
        auto wsum = [](unsigned x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; };
#pragma unroll
        for (int c = 0; c < QC_REG; ++c) {
            if (c < Cp) {
                const unsigned a = wsum(nv[c]), b = wsum(nw[c]);
                if (lane == 0) { qsh[wave * 2 * QC_REG + c] = a; qsh[wave * 2 * QC_REG + QC_REG + c] = b; }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * Cp) {
            const int i = threadIdx.x < Cp ? threadIdx.x : QC_REG + threadIdx.x - Cp;
            unsigned s = 0;
            for (int w = 0; w < QC_T / 64; ++w) s += qsh[w * 2 * QC_REG + i];
            partial[(int64_t)threadIdx.x * nblk + blockIdx.x] = s;
        }
    } else if constexpr (MODE == QC_MODE_LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * Cp; i += QC_T) partial[(int64_t)i * nblk + blockIdx.x] = qsh[i];
    }
}

// one wave per value: the nblk block columns summed in uint64, the result written (not accumulated)
__global__ void __launch_bounds__(QC_T) k_qc_finalize(const unsigned* __restrict__ partial, int nblk, int nval,
                                                      unsigned long long* __restrict__ counts) {
    const int i = blockIdx.x * (QC_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nval) return;   // wave-uniform
    // 8 independent loads in flight per lane (the columns were written by blocks on every XCD: each load misses this XCD's L2).
    // Measured 11 us at 12 values and 15 us at 260, the same as with one load per trip: the bound is not the loads
    const unsigned* col = partial + (int64_t)i * nblk;
    unsigned long long a = 0;
    for (int b0 = 0; b0 < nblk; b0 += 64 * 8) {
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int b = b0 + u * 64 + lane;
            v[u] = b < nblk ? col[b] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) counts[i] = a;
}

int qc_blocks(int64_t S, int vec) {
    const int64_t nb = (S + (int64_t)QC_T * vec - 1) / ((int64_t)QC_T * vec);
    return (int)(nb > QC_MAX_BLOCKS ? QC_MAX_BLOCKS : nb);
}

template <int VEC>
void launch_qc_partial(const float* logits, const float* label, const float* image0, int C, int k, int shift, int64_t S,
                       unsigned* partial, int nblk, hipStream_t s) {
    const int Cp = k ? C - k + 1 : C;
    if (Cp <= QC_REG)
        k_qc_partial<VEC, QC_MODE_REG><<<nblk, QC_T, 4 * 2 * QC_REG * sizeof(unsigned), s>>>(logits, label, image0, C, k, shift, S, partial);
    else if (Cp <= QC_LDS)
        k_qc_partial<VEC, QC_MODE_LDS><<<nblk, QC_T, 2 * Cp * sizeof(unsigned), s>>>(logits, label, image0, C, k, shift, S, partial);
    else
        k_qc_partial<VEC, QC_MODE_GMEM><<<nblk, QC_T, 0, s>>>(logits, label, image0, C, k, shift, S, partial);
}

}  // namespace

size_t qc_scratch_bytes(int out_c, int64_t S, int collapse) {
    const int Cp = collapse ? out_c - collapse + 1 : out_c;
    return (size_t)qc_blocks(S, 1) * 2 * Cp * sizeof(unsigned);   // the scalar path's grid: never fewer blocks than the vector path's
}

void launch_qc_counts(const float* logits, const float* label, const float* image0, int out_c, int64_t S, int collapse, int shift,
                      uint64_t* counts, void* scratch, hipStream_t s) {
    const int Cp = collapse ? out_c - collapse + 1 : out_c;
    // 16-B loads when every plane starts 16-B aligned: aligned base pointers and S % 4 == 0 (the channel stride)
    const bool v4 = S % 4 == 0 && ((uintptr_t)logits | (uintptr_t)label | (uintptr_t)(shift > 0 ? image0 : nullptr)) % 16 == 0;
    const int nblk = qc_blocks(S, v4 ? 4 : 1);
    unsigned* partial = (unsigned*)scratch;
    if (v4) launch_qc_partial<4>(logits, label, image0, out_c, collapse, shift, S, partial, nblk, s);
    else launch_qc_partial<1>(logits, label, image0, out_c, collapse, shift, S, partial, nblk, s);
    k_qc_finalize<<<cdiv64(2 * Cp, QC_T / 64), QC_T, 0, s>>>(partial, nblk, 2 * Cp, (unsigned long long*)counts);
}

}  // namespace unet
