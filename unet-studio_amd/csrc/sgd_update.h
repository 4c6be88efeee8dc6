// The optimizer arithmetic shared by k_sgd (kernels_elem.hip) and k_sgd_pack (kernels_sgd_pack.hip): both must give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace unet {

// Total gradient norm from the k_sumsq_partial partials and the clip coefficient (train.cpp:759-764).  Every thread of the block calls
// it (blockDim.x >= 256); threads 0..255 add the partials in a fixed order, so the sum has the same bits at any block size.
// red: 256 doubles and s_coef: one float of LDS.  Block 0 writes the norm to norm_out.
__device__ __forceinline__ float sgd_clip_coef(const float* __restrict__ partial, int nblk, float clip_norm, float* norm_out, double* red,
                                               float* s_coef) {
    const int tid = threadIdx.x;
    if (tid < 256) {
        double part = 0.0;
        for (int b = tid; b < nblk; b += 256) part += partial[b];
        red[tid] = part;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        float norm = (float)sqrt(red[0]);
        float coef = clip_norm / (norm + 1e-6f);
        *s_coef = coef > 1.f ? 1.f : coef;
        if (blockIdx.x == 0 && norm_out) *norm_out = norm;
    }
    __syncthreads();
    return *s_coef;
}

// weight decay, Nesterov momentum, parameter update and zero_grad of one element (unet.cpp:254-275); coef = clip coefficient * grad_scale
struct SgdUpdate {
    float coef, lr, momentum;
    int nesterov;
    __device__ __forceinline__ void operator()(float& pv, float& gv, float& mv, float wd) const {
        float d = fmaf(wd, pv, gv * coef);
        float b = fmaf(momentum, mv, d);
        mv = b;
        pv = pv - lr * (nesterov ? fmaf(momentum, b, d) : b);
        gv = 0.f;
    }
};

}  // namespace unet
