// Per-sample preparation of the template/subject training feed (train.cpp:229-257,413-419,615-617; include/unet_feed.h):
// the label maximum read as int, tipl::normalize, shift_subject_label and the cast toward zero to int64.
//
// The maximum is a two-launch reduction: every block writes the max of its part of the volume to its own slot of the caller's
// scratch, and a one-block finishing kernel reduces the slots and writes the max (float, for normalize) and, when asked, the max
// read as int.  There is no global atomic shared between blocks.  The elementwise kernels read the max from the device, so a
// normalizing call never syncs with the host.
//
// Loads and stores are 16 B wide when every array the kernel touches is 16-B aligned; the last voxels % 4 voxels then go to the
// scalar tail of block 0.  Any other alignment runs the scalar path.
#include <climits>

#include "device_util.h"

namespace unet {

namespace {

constexpr int FEED_T = 256;            // threads per block
constexpr int FEED_MAX_BLOCKS = 1024;  // 256 CUs x 4 blocks; the grid strides over the rest

int feed_blocks(int64_t n) {
    const int64_t nb = (n + FEED_T - 1) / FEED_T;
    return (int)(nb < 1 ? 1 : nb > FEED_MAX_BLOCKS ? FEED_MAX_BLOCKS : nb);
}

__device__ __forceinline__ float block_max(float m) {
    __shared__ float wmax[FEED_T / 64];
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (int w = 1; w < FEED_T / 64; ++w) m = fmaxf(m, wmax[w]);
    return m;
}

// the max of label[0..S) per block (fmaxf: a NaN voxel is skipped); VEC == 4: label is 16-B aligned, block 0 also takes the tail
template <int VEC>
__global__ void __launch_bounds__(FEED_T) k_feed_max_partial(const float* __restrict__ label, int64_t S, float* __restrict__ partial) {
    float m = -INFINITY;
    const int64_t nv = S / VEC, stride = (int64_t)gridDim.x * FEED_T;
    for (int64_t i = (int64_t)blockIdx.x * FEED_T + threadIdx.x; i < nv; i += stride) {
        if constexpr (VEC == 4) {
            const float4 q = ((const float4*)label)[i];
            m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
        } else {
            m = fmaxf(m, label[i]);
        }
    }
    if (VEC > 1 && blockIdx.x == 0 && (int64_t)threadIdx.x < S - nv * VEC) m = fmaxf(m, label[nv * VEC + threadIdx.x]);
    m = block_max(m);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// max over the nblk partials -> *max_out (float) and *imax_out (the max read as int: toward zero, clamped to int; may be null)
__global__ void __launch_bounds__(FEED_T) k_feed_max_finish(const float* __restrict__ partial, int nblk, float* __restrict__ max_out,
                                                            int* __restrict__ imax_out) {
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += FEED_T) m = fmaxf(m, partial[i]);
    m = block_max(m);
    if (threadIdx.x == 0) {
        *max_out = m;
        if (imax_out) {
            const float t = truncf(m);   // max(trunc(l)) == trunc(max(l)): trunc is monotone
            *imax_out = t >= 2147483647.f ? INT_MAX : t <= -2147483648.f ? INT_MIN : (int)t;
        }
    }
}

// tipl::normalize (l / max when max > 0; maxp null: no normalization), then shift_subject_label (shift > 0), in float
__device__ __forceinline__ float feed_label(float l, float img, float m, int shift) {
    if (m > 0.f) l = l / m;
    if (shift > 0) l = l != 0.f ? l + (float)shift : (img > 0.f ? 1.f : 0.f);
    return l;
}

template <int VEC>
__global__ void __launch_bounds__(FEED_T) k_feed_prepare(const float* __restrict__ image0, float* __restrict__ label, int64_t S,
                                                         const float* __restrict__ maxp, int shift) {
    const float m = maxp ? *maxp : 0.f;
    const int64_t nv = S / VEC, stride = (int64_t)gridDim.x * FEED_T;
    for (int64_t i = (int64_t)blockIdx.x * FEED_T + threadIdx.x; i < nv; i += stride) {
        if constexpr (VEC == 4) {
            float4 q = ((const float4*)label)[i];
            float4 g = shift > 0 ? ((const float4*)image0)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            q.x = feed_label(q.x, g.x, m, shift);
            q.y = feed_label(q.y, g.y, m, shift);
            q.z = feed_label(q.z, g.z, m, shift);
            q.w = feed_label(q.w, g.w, m, shift);
            ((float4*)label)[i] = q;
        } else {
            label[i] = feed_label(label[i], shift > 0 ? image0[i] : 0.f, m, shift);
        }
    }
    if (VEC > 1 && blockIdx.x == 0 && (int64_t)threadIdx.x < S - nv * VEC) {
        const int64_t i = nv * VEC + threadIdx.x;
        label[i] = feed_label(label[i], shift > 0 ? image0[i] : 0.f, m, shift);
    }
}

// .to(torch::kLong) of the (optionally normalized) label: toward zero
template <int VEC>
__global__ void __launch_bounds__(FEED_T) k_feed_target(const float* __restrict__ label, int64_t S, const float* __restrict__ maxp,
                                                        long long* __restrict__ target) {
    const float m = maxp ? *maxp : 0.f;
    const int64_t nv = S / VEC, stride = (int64_t)gridDim.x * FEED_T;
    for (int64_t i = (int64_t)blockIdx.x * FEED_T + threadIdx.x; i < nv; i += stride) {
        if constexpr (VEC == 4) {
            const float4 q = ((const float4*)label)[i];
            longlong2* t = (longlong2*)target + 2 * i;
            t[0] = make_longlong2((long long)feed_label(q.x, 0.f, m, 0), (long long)feed_label(q.y, 0.f, m, 0));
            t[1] = make_longlong2((long long)feed_label(q.z, 0.f, m, 0), (long long)feed_label(q.w, 0.f, m, 0));
        } else {
            target[i] = (long long)feed_label(label[i], 0.f, m, 0);
        }
    }
    if (VEC > 1 && blockIdx.x == 0 && (int64_t)threadIdx.x < S - nv * VEC) {
        const int64_t i = nv * VEC + threadIdx.x;
        target[i] = (long long)feed_label(label[i], 0.f, m, 0);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// scratch: [0, 256) the float max and the spare slots, [256, ...) one float partial per block
float* feed_max_slot(void* scratch) { return (float*)scratch; }
float* feed_partials(void* scratch) { return (float*)((char*)scratch + 256); }

void launch_feed_max(const float* label, int64_t S, void* scratch, int* imax_out, hipStream_t s) {
    const bool v4 = aligned16(label);
    const int nblk = feed_blocks(v4 ? S / 4 : S);
    if (v4) k_feed_max_partial<4><<<nblk, FEED_T, 0, s>>>(label, S, feed_partials(scratch));
    else k_feed_max_partial<1><<<nblk, FEED_T, 0, s>>>(label, S, feed_partials(scratch));
    k_feed_max_finish<<<1, FEED_T, 0, s>>>(feed_partials(scratch), nblk, feed_max_slot(scratch), imax_out);
}

}  // namespace

size_t feed_scratch_bytes(int64_t S) { return 256 + (size_t)feed_blocks(S) * sizeof(float); }   // the scalar grid: the larger one

void launch_feed_label_max(const float* label, int64_t S, int* out_max, void* scratch, hipStream_t s) {
    launch_feed_max(label, S, scratch, out_max, s);
}

void launch_feed_prepare(const float* image0, float* label, int64_t S, int normalize, int shift, int* label_max, void* scratch,
                         hipStream_t s) {
    if (normalize || label_max) launch_feed_max(label, S, scratch, label_max, s);
    if (!normalize && shift <= 0) return;   // nothing to rewrite
    const float* maxp = normalize ? feed_max_slot(scratch) : nullptr;
    const bool v4 = aligned16(label) && (shift <= 0 || aligned16(image0));
    const int nblk = feed_blocks(v4 ? S / 4 : S);
    if (v4) k_feed_prepare<4><<<nblk, FEED_T, 0, s>>>(image0, label, S, maxp, shift);
    else k_feed_prepare<1><<<nblk, FEED_T, 0, s>>>(image0, label, S, maxp, shift);
}

void launch_feed_target(const float* label, int64_t S, int normalize, int64_t* target, void* scratch, hipStream_t s) {
    if (normalize) launch_feed_max(label, S, scratch, nullptr, s);
    const float* maxp = normalize ? feed_max_slot(scratch) : nullptr;
    const bool v4 = aligned16(label) && aligned16(target);
    const int nblk = feed_blocks(v4 ? S / 4 : S);
    if (v4) k_feed_target<4><<<nblk, FEED_T, 0, s>>>(label, S, maxp, (long long*)target);
    else k_feed_target<1><<<nblk, FEED_T, 0, s>>>(label, S, maxp, (long long*)target);
}

}  // namespace unet
