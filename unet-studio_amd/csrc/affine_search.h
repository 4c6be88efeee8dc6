// What the two affine pattern searches share (kernels_register.hip: tissue maps, include/unet_register.h; kernels_coreg.hip:
// intensity codes, include/unet_coreg.h): the position of a voxel under a 12-float map, the merging of equal histogram keys in
// registers, and the arithmetic of the search state.  Device code only, all inlined.  Plan is a struct with step[12],
// stages[][3] and the centre voxel cx, cy, cz; State one with cand[], K and stride.
#pragma once
#include <hip/hip_runtime.h>

namespace unet {

struct AffPos {
    float qx, qy, qz;   // position + 0.5
    bool in;
};
// map(x, y, z) + 0.5 in fp32, left to right, no fused multiply-add, and the inside test against float(dim); a NaN is outside
__device__ __forceinline__ AffPos aff_locate(const float* m, int xi, int yi, int zi, int tw, int th, int td) {
#pragma clang fp contract(off)
    const float x = (float)xi, y = (float)yi, z = (float)zi;
    AffPos p;
    p.qx = (((m[0] * x + m[1] * y) + m[2] * z) + m[9]) + 0.5f;
    p.qy = (((m[3] * x + m[4] * y) + m[5] * z) + m[10]) + 0.5f;
    p.qz = (((m[6] * x + m[7] * y) + m[8] * z) + m[11]) + 0.5f;
    p.in = p.qx >= 0.f && p.qy >= 0.f && p.qz >= 0.f && p.qx < (float)tw && p.qy < (float)th && p.qz < (float)td;
    return p;
}

// A run of equal keys in registers (kernels_atlas.hip's): push() adds to the open run or hands the closed one to add(key, n)
struct AffRun {
    unsigned key, n;
    template <typename Add> __device__ __forceinline__ void push(unsigned k, Add add) {
        if (k == key) {
            ++n;
        } else {
            if (n) add(key, n);
            key = k;
            n = 1u;
        }
    }
    template <typename Add> __device__ __forceinline__ void close(Add add) {
        if (n) add(key, n);
        n = 0u;
    }
};

// the index of the j-th parameter with step > 0 (12 when there is none)
template <typename Plan> __device__ __forceinline__ int aff_param(const Plan& p, int j) {
    int i = 0;
    for (; i < 12; ++i)
        if (p.step[i] > 0.f && j-- == 0) break;
    return i;
}

// c[i] moved by one step of level l: sign > 0 adds ldexpf(step[i], -l), sign < 0 subtracts it (one fp32 operation)
__device__ __forceinline__ float aff_move(float c, float step, int level, int sign) {
    const float d = ldexpf(step, -level);
    return sign > 0 ? c + d : c - d;
}

// the map of a state: the matrix unchanged, t_r = u_r - ((c[3r]*cx + c[3r+1]*cy) + c[3r+2]*cz)
template <typename Plan> __device__ __forceinline__ void aff_state_map(const float (&c)[12], const Plan& p, float* map) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 9; ++e) map[e] = c[e];
#pragma unroll
    for (int r = 0; r < 3; ++r) map[9 + r] = c[9 + r] - ((c[3 * r] * p.cx + c[3 * r + 1] * p.cy) + c[3 * r + 2] * p.cz);
}

// Every thread of the block: thread k < K writes the map of candidate k of (stage g, level l); thread 0 the K and the stride.
// lc: the state's parameters in LDS
template <typename State, typename Plan> __device__ __forceinline__ void aff_candidates(State* st, const float* lc, const Plan& p, int g, int l) {
    int P = 0;
    for (int i = 0; i < 12; ++i) P += p.step[i] > 0.f ? 1 : 0;
    const int K = 1 + 2 * P, k = threadIdx.x;
    if (k < K) {
        const int i = k ? aff_param(p, (k - 1) >> 1) : 12, sign = (k & 1) ? 1 : -1;
        const float step = i < 12 ? p.step[i] : 0.f;
        float c[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) c[e] = e == i ? aff_move(lc[e], step, l, sign) : lc[e];
        float map[12];
        aff_state_map(c, p, map);
#pragma unroll
        for (int e = 0; e < 12; ++e) st->cand[k * 12 + e] = map[e];
    }
    if (k == 0) {
        st->K = K;
        st->stride = p.stages[g][0];
    }
}

}  // namespace unet
