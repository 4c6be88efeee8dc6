// Device helpers shared by the kernel files (gfx950 only).
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

namespace unet {

typedef __hip_bfloat16 bf16;

template <typename T> __device__ __forceinline__ float ld(const T* p, int64_t i);
template <> __device__ __forceinline__ float ld<float>(const float* p, int64_t i) { return p[i]; }
template <> __device__ __forceinline__ float ld<bf16>(const bf16* p, int64_t i) { return __bfloat162float(p[i]); }
template <typename T> __device__ __forceinline__ void st(T* p, int64_t i, float v);
template <> __device__ __forceinline__ void st<float>(float* p, int64_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st<bf16>(bf16* p, int64_t i, float v) { p[i] = __float2bfloat16(v); }

// activations of unet.cpp:91-98
__device__ __forceinline__ float act_f(float v, int act) {
    switch (act) {
        case 1: return v > 0.f ? v : 0.f;
        case 2: return v > 0.f ? v : 0.01f * v;
        case 3: return v > 0.f ? v : expm1f(v);
        default: return v;
    }
}
__device__ __forceinline__ float act_d(float v, int act) {
    switch (act) {
        case 1: return v > 0.f ? 1.f : 0.f;
        case 2: return v > 0.f ? 1.f : 0.01f;
        case 3: return v > 0.f ? 1.f : expf(v);
        default: return 1.f;
    }
}

template <typename T> __device__ __forceinline__ float view_ld(const SrcDesc& s, int64_t voxel, int c) {
    float v = ld<T>((const T*)s.ptr, voxel * s.C + c);
    // one rounding, spelled out: the vectorised copies (k_apply_view8*) and every backward kernel evaluate the pre-activation with fmaf,
    // and the forward must land on the same side of an activation's kink as they do whatever the contraction mode of the including file
    if (s.scale) v = fmaf(v, s.scale[c], s.shift[c]);
    return act_f(v, s.act);
}

#define UNET_DISPATCH(dtype, CALL)                 \
    do {                                           \
        if ((dtype) == 0) { typedef float T; CALL; } \
        else { typedef bf16 T; CALL; }             \
    } while (0)

// 3x3x3 binomial (1,2,1)^3/64 at (x, y, z) of a W x H x D volume (x fastest), border voxels replicated, taps accumulated in
// (kz, ky, kx) order; load(i) returns voxel i (volumes < 2^31 voxels).  The stand-in for tipl::filter::gaussian (TIPL, absent:
// parity unpinned) shared by simulate_modality (kernels_augment.hip) and the post-processing chain (kernels_postproc.hip).
template <typename Load>
__device__ __forceinline__ float binomial3(int W, int H, int D, int x, int y, int z, Load load) {
#pragma clang fp contract(off)   // w * v then + in fp32, as the numpy restatement (oracle/augment_ref.py:_smooth) rounds
    float acc = 0.f;
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
        const int zz = min(max(z + kz - 1, 0), D - 1);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = min(max(y + ky - 1, 0), H - 1);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = min(max(x + kx - 1, 0), W - 1);
                const float v = load((unsigned)((zz * H + yy) * W + xx));
                const float w = (float)((kz == 1 ? 2 : 1) * (ky == 1 ? 2 : 1) * (kx == 1 ? 2 : 1)) * (1.0f / 64.0f);
                acc += w * v;
            }
        }
    }
    return acc;
}

// ---- the gather passes' thread -> voxel map (kernels_augment.hip, kernels_space.hip) ---------------------------------------------
// A block of 256 threads on a 16 x 4 x 4 brick; gx, gy: bricks along x and y.  The grid is the brick count rounded up to a multiple
// of 8, and bricks are numbered so that each XCD (blocks are dealt round-robin to the 8 XCDs) works through one contiguous z-range
// of the volume.  Returns false for a thread whose voxel is outside the volume (x = y = z = 0 for a block with no brick).
constexpr int BRICK_X = 16, BRICK_Y = 4, BRICK_Z = 4;

__device__ __forceinline__ bool brick_walk(int W, int H, int D, int gx, int gy, int& x, int& y, int& z) {
    const unsigned nb = gridDim.x, per = (nb + 7) / 8;
    const unsigned b = (blockIdx.x & 7) * per + (blockIdx.x >> 3);   // uniform
    if (b >= nb) { x = y = z = 0; return false; }                     // only when nb is not a multiple of 8: ids >= nb idle
    const unsigned bx = b % gx, r = b / gx, by = r % gy, bz = r / gy;
    x = bx * BRICK_X + (threadIdx.x & (BRICK_X - 1));
    y = by * BRICK_Y + ((threadIdx.x / BRICK_X) & (BRICK_Y - 1));
    z = bz * BRICK_Z + threadIdx.x / (BRICK_X * BRICK_Y);
    return x < W && y < H && z < D;
}

// ---- the sampler (this project's stand-in for tipl::compose_mapping / tipl::resample; oracle/augment_ref.py _locate, _trilinear,
// _majority restate it).  FMA contraction is off inside the bodies, whatever the including file's mode, so the restatement rounds
// identically.
struct Tri {   // trilinear footprint: the 8 corner offsets (corner i: bit 0 = x, bit 1 = y, bit 2 = z; upper neighbours clamped), fractions
    unsigned o[8];
    float tx, ty, tz;
    bool ok;
};

// 32-bit offsets inside one volume (the launchers check D*H*W < 2^31): the loads become base + 32-bit-offset accesses and the
// address arithmetic stays off the quarter-rate 64-bit multiplier
__device__ __forceinline__ Tri locate(float x, float y, float z, int W, int H, int D) {
#pragma clang fp contract(off)
    Tri t;
    // NaN positions (a distortion focus's own centre voxel, .cu:151: 0/0) fail these comparisons, as out-of-volume ones do
    t.ok = (x >= 0.f) && (y >= 0.f) && (z >= 0.f) && (x <= (float)(W - 1)) && (y <= (float)(H - 1)) && (z <= (float)(D - 1));
    if (!t.ok) return t;
    float fx = floorf(x), fy = floorf(y), fz = floorf(z);
    t.tx = x - fx; t.ty = y - fy; t.tz = z - fz;
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1), z1 = min(z0 + 1, D - 1);
    const unsigned r00 = (unsigned)(z0 * H + y0) * (unsigned)W, r10 = (unsigned)(z0 * H + y1) * (unsigned)W,
                   r01 = (unsigned)(z1 * H + y0) * (unsigned)W, r11 = (unsigned)(z1 * H + y1) * (unsigned)W;
    t.o[0] = r00 + x0; t.o[1] = r00 + x1; t.o[2] = r10 + x0; t.o[3] = r10 + x1;
    t.o[4] = r01 + x0; t.o[5] = r01 + x1; t.o[6] = r11 + x0; t.o[7] = r11 + x1;
    return t;
}

__device__ __forceinline__ float lerp1(float t, float a, float b) {
#pragma clang fp contract(off)
    return a + t * (b - a);
}

__device__ __forceinline__ float trilinear(const Tri& t, const float* __restrict__ vol) {
    float c00 = lerp1(t.tx, vol[t.o[0]], vol[t.o[1]]);
    float c10 = lerp1(t.tx, vol[t.o[2]], vol[t.o[3]]);
    float c01 = lerp1(t.tx, vol[t.o[4]], vol[t.o[5]]);
    float c11 = lerp1(t.tx, vol[t.o[6]], vol[t.o[7]]);
    return lerp1(t.tz, lerp1(t.ty, c00, c10), lerp1(t.ty, c01, c11));
}

// label resampling for class ids: the value holding the largest total trilinear weight among the 8 corners
// (first corner wins ties; corner order x fastest)
__device__ __forceinline__ float majority(const Tri& t, const float* __restrict__ vol) {
#pragma clang fp contract(off)
    float v[8], w[8];
    float wx[2] = {1.0f - t.tx, t.tx}, wy[2] = {1.0f - t.ty, t.ty}, wz[2] = {1.0f - t.tz, t.tz};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = vol[t.o[i]];
        w[i] = wx[i & 1] * wy[(i >> 1) & 1] * wz[i >> 2];
    }
    float best = v[0], best_score = -1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += (v[i] == v[j]) ? w[i] : 0.f;
        if (s > best_score) { best_score = s; best = v[j]; }
    }
    return best;
}

// ---- the softmax / create_mask accumulator of the post-processing pass (kernels_postproc.hip, kernels_space.hip) -------------------
// one channel into the online state: m the running max, s = sum exp(x - m), sf the same over the foreground (fgc = 1).
// -inf adds nothing; a NaN makes s NaN; +inf makes m infinite.  Both mark the voxel bad at the end (torch.softmax's NaN rows).
// Compiled in the default contraction mode on purpose: both users must round alike.
__device__ __forceinline__ void pp_acc(float x, float& m, float& s, float& sf, float fgc) {
    if (x > m) {
        const float e = expf(m - x);
        s = s * e + 1.f;
        sf = sf * e + fgc;
        m = x;
    } else if (x != -INFINITY) {
        const float e = expf(x - m);
        s += e;
        sf += fgc * e;
    }
}

template <int VEC> __device__ __forceinline__ void ldv(const float* __restrict__ p, int64_t i, float (&x)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = *(const float4*)(p + i);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = p[i];
    }
}
template <int VEC> __device__ __forceinline__ void stv(float* __restrict__ p, int64_t i, const float (&x)[VEC]) {
    if constexpr (VEC == 4) *(float4*)(p + i) = make_float4(x[0], x[1], x[2], x[3]);
    else p[i] = x[0];
}

// The softmax / create_mask / argmax of VEC consecutive voxels from v (include/unet_postproc.h), the body of k_pp_softmax
// (kernels_postproc.hip) and of the passes that form each logit on the fly (kernels_mirror.hip).  first(c, x) yields channel c's
// logits, called once per channel in ascending c; again(c, x) yields the same values a second time, for label_prob only.
template <int VEC, typename First, typename Again>
__device__ __forceinline__ void pp_voxels(int C, int64_t S, int64_t v, float thr, float* __restrict__ lp, float* __restrict__ fg,
                                          uint16_t* __restrict__ lab, First first, Again again) {
    float m[VEC], s[VEC], sf[VEC], best[VEC], x[VEC];
    int arg[VEC];
    first(0, x);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        m[j] = -INFINITY; s[j] = 0.f; sf[j] = 0.f; best[j] = 0.f; arg[j] = 1;
        pp_acc(x[j], m[j], s[j], sf[j], 0.f);
    }
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
        first(c, x);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            pp_acc(x[j], m[j], s[j], sf[j], 1.f);
            if (c == 1 || x[j] > best[j]) { best[j] = x[j]; arg[j] = c; }   // torch.argmax: the first index wins a tie
        }
    }
    bool bad[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) bad[j] = !(fabsf(m[j]) < INFINITY) || s[j] != s[j];
    if (fg || lab) {
        float f[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = bad[j] ? NAN : sf[j] / s[j];
        if (fg) stv<VEC>(fg, v, f);
        if (lab) {
            uint16_t l[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) l[j] = f[j] > thr ? (uint16_t)arg[j] : (uint16_t)0;   // NaN > thr is false
            if constexpr (VEC == 4) *(ushort4*)(lab + v) = make_ushort4(l[0], l[1], l[2], l[3]);
            else lab[v] = l[0];
        }
    }
    if (lp) {
#pragma unroll 4
        for (int c = 1; c < C; ++c) {
            again(c, x);
            float p[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) p[j] = bad[j] ? NAN : expf(x[j] - m[j]) / s[j];
            stv<VEC>(lp, (int64_t)(c - 1) * S + v, p);
        }
    }
}

static inline unsigned cdiv64(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace unet
