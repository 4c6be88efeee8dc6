// Test-time mirroring (include/unet_mirror.h): the K members' logits, each computed from a flipped input, are flipped back, their
// lateralised channels swapped back, and averaged.
//
//   k_mirror_combine   mean(c, v) = (sum_m stack[m][sigma_m(c)][FLIP_m(v)]) / K, and / or the agreement map: one gather pass
//   k_mirror_postproc  the softmax / create_mask / argmax pass of kernels_postproc.hip on the mean: the per-voxel body is the shared
//                      pp_voxels (device_util.h), each logit it asks for being the COMBINE of the stack, never stored
//
// A thread owns VEC consecutive output voxels of one row.  VEC = 4 when W % 4 == 0 and every plane is 16-B aligned: a member
// flipped in x then reads the mirrored 16-B word and reverses its four lanes in registers, so a wave still covers whole lines, in
// descending order.  Otherwise VEC = 1.  The y / z flips only move a member's row: K 32-bit offsets per thread, computed once.
// sigma_m only moves the plane: one uniform walk over the pairs in the launch arguments per channel.  The member loop is the inner
// one over a compile-time K, so the K loads of a channel are in flight together.  With AGREE each member's running amax is kept beside
// the mean's (K + 1 value / index pairs per voxel).  No LDS, no atomics, no scratch.
#include "../../include/unet_mirror.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int MR_T = 256;
constexpr int MR_MAXB = 2048;   // 256 CUs x 8 blocks; the threads stride over the rest

struct MirrorArgs {
    int W, H, D, C;
    int masks[8];
    int swap_axis, n_pairs;
    int pairs[2 * UNET_MIRROR_MAX_PAIRS];
};

// sigma(c): uniform (c and the pairs are)
__device__ __forceinline__ int mirror_sigma(const MirrorArgs& a, int c) {
    int r = c;
    for (int i = 0; i < a.n_pairs; ++i) {
        if (a.pairs[2 * i] == c) r = a.pairs[2 * i + 1];
        if (a.pairs[2 * i + 1] == c) r = a.pairs[2 * i];
    }
    return r;
}

template <int VEC, int K> struct Members {   // one thread's VEC voxels in every member
    unsigned off[K];                         // the first voxel read inside a plane (the lowest address of the word)
    // FLIP_m of the VEC voxels from (x, y, z), x a multiple of VEC
    __device__ __forceinline__ void locate(const MirrorArgs& a, int x, int y, int z) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int m = a.masks[k];
            const int xs = (m & 1) ? a.W - VEC - x : x, ys = (m & 2) ? a.H - 1 - y : y, zs = (m & 4) ? a.D - 1 - z : z;
            off[k] = (unsigned)((zs * a.H + ys) * a.W + xs);
        }
    }
    // COMBINE of channel c: member 0's value, then the others in ascending m, every add rounded; the scale 1/K is exact.
    // each(k, q): member k's VEC values, for the agreement
    template <typename Each>
    __device__ __forceinline__ void combine(const float* __restrict__ stack, const MirrorArgs& a, int64_t S, int c, float (&x)[VEC],
                                            Each each) const {
#pragma clang fp contract(off)
        const int sc = a.swap_axis >= 0 && a.n_pairs ? mirror_sigma(a, c) : c;
        float q[K][VEC];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int m = a.masks[k];
            const int ch = a.swap_axis >= 0 && ((m >> a.swap_axis) & 1) ? sc : c;
            float t[VEC];
            ldv<VEC>(stack + ((int64_t)k * a.C + ch) * S, off[k], t);
#pragma unroll
            for (int j = 0; j < VEC; ++j) q[k][j] = (m & 1) ? t[VEC - 1 - j] : t[j];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) x[j] = q[0][j];
#pragma unroll
        for (int k = 1; k < K; ++k)
#pragma unroll
            for (int j = 0; j < VEC; ++j) x[j] += q[k][j];
        if constexpr (K > 1) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) x[j] *= 1.0f / K;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) each(k, q[k]);
    }
};

// the running amax of include/unet_mirror.h: best = 0, then a later channel wins only when greater (a comparison with NaN is false)
template <int VEC, int K> struct Votes {
    float bv[K + 1][VEC];
    int bi[K + 1][VEC];   // [K]: the mean's
    __device__ __forceinline__ void see(int k, int c, const float (&x)[VEC]) {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (c == 0 || x[j] > bv[k][j]) { bv[k][j] = x[j]; bi[k][j] = c; }
    }
    __device__ __forceinline__ void store(uint8_t* __restrict__ agreement, int64_t v) const {
        uint8_t n[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) cnt += bi[k][j] == bi[K][j];
            n[j] = (uint8_t)cnt;
        }
        if constexpr (VEC == 4) *(uchar4*)(agreement + v) = make_uchar4(n[0], n[1], n[2], n[3]);
        else agreement[v] = n[0];
    }
};

// item i of the grid-stride walk -> the first of its VEC voxels
template <int VEC> __device__ __forceinline__ void mirror_voxel(const MirrorArgs& a, int64_t i, int& x, int& y, int& z) {
    const unsigned wv = (unsigned)a.W / VEC, u = (unsigned)i, row = u / wv;
    x = (int)(u - row * wv) * VEC;
    z = (int)(row / (unsigned)a.H);
    y = (int)(row - (unsigned)z * (unsigned)a.H);
}

template <int VEC, int K, bool AGREE>
__global__ void __launch_bounds__(MR_T) k_mirror_combine(const float* __restrict__ stack, MirrorArgs a, int64_t S, float* __restrict__ mean,
                                                         uint8_t* __restrict__ agreement) {
    const int64_t n = S / VEC;   // VEC == 4 only when W % 4 == 0
    for (int64_t i = (int64_t)blockIdx.x * MR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * MR_T) {
        int x, y, z;
        mirror_voxel<VEC>(a, i, x, y, z);
        Members<VEC, K> mem;
        mem.locate(a, x, y, z);
        Votes<VEC, AGREE ? K : 0> votes;
        const int64_t v = i * VEC;
        for (int c = 0; c < a.C; ++c) {
            float xc[VEC];
            mem.combine(stack, a, S, c, xc, [&](int k, const float (&q)[VEC]) { if constexpr (AGREE) votes.see(k, c, q); });
            if constexpr (AGREE) votes.see(K, c, xc);
            if (mean) stv<VEC>(mean, (int64_t)c * S + v, xc);
        }
        if constexpr (AGREE) votes.store(agreement, v);
    }
}

template <int VEC, int K, bool AGREE>
__global__ void __launch_bounds__(MR_T) k_mirror_postproc(const float* __restrict__ stack, MirrorArgs a, int64_t S, float thr,
                                                          float* __restrict__ lp, float* __restrict__ fg, uint16_t* __restrict__ lab,
                                                          uint8_t* __restrict__ agreement) {
    const int64_t n = S / VEC;
    for (int64_t i = (int64_t)blockIdx.x * MR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * MR_T) {
        int x, y, z;
        mirror_voxel<VEC>(a, i, x, y, z);
        Members<VEC, K> mem;
        mem.locate(a, x, y, z);
        Votes<VEC, AGREE ? K : 0> votes;
        const int64_t v = i * VEC;
        const auto first = [&](int c, float (&xc)[VEC]) {
            mem.combine(stack, a, S, c, xc, [&](int k, const float (&q)[VEC]) { if constexpr (AGREE) votes.see(k, c, q); });
            if constexpr (AGREE) votes.see(K, c, xc);
        };
        const auto again = [&](int c, float (&xc)[VEC]) { mem.combine(stack, a, S, c, xc, [](int, const float (&)[VEC]) {}); };
        if (lp || fg || lab) {
            pp_voxels<VEC>(a.C, S, v, thr, lp, fg, lab, first, again);
        } else {                 // the agreement alone
            float xc[VEC];
            for (int c = 0; c < a.C; ++c) first(c, xc);
        }
        if constexpr (AGREE) votes.store(agreement, v);
    }
}

MirrorArgs mirror_args(int C, int W, int H, int D, int n_members, const int* masks, int swap_axis, const int* pairs, int n_pairs) {
    MirrorArgs a = {};
    a.W = W; a.H = H; a.D = D; a.C = C;
    for (int k = 0; k < n_members; ++k) a.masks[k] = masks[k];
    a.swap_axis = n_pairs ? swap_axis : -1;
    a.n_pairs = n_pairs;
    for (int i = 0; i < 2 * n_pairs; ++i) a.pairs[i] = pairs[i];
    return a;
}

int mirror_blocks(int64_t items) {
    const int64_t nb = (items + MR_T - 1) / MR_T;
    return (int)(nb > MR_MAXB ? MR_MAXB : nb < 1 ? 1 : nb);
}

template <int VEC, int K>
void combine_vk(const float* stack, const MirrorArgs& a, int64_t S, float* mean, uint8_t* agreement, hipStream_t s) {
    const int nb = mirror_blocks(S / VEC);
    if (agreement) k_mirror_combine<VEC, K, true><<<nb, MR_T, 0, s>>>(stack, a, S, mean, agreement);
    else k_mirror_combine<VEC, K, false><<<nb, MR_T, 0, s>>>(stack, a, S, mean, agreement);
}
template <int VEC, int K>
void postproc_vk(const float* stack, const MirrorArgs& a, int64_t S, float thr, float* lp, float* fg, uint16_t* lab, uint8_t* agreement,
                 hipStream_t s) {
    const int nb = mirror_blocks(S / VEC);
    if (agreement) k_mirror_postproc<VEC, K, true><<<nb, MR_T, 0, s>>>(stack, a, S, thr, lp, fg, lab, agreement);
    else k_mirror_postproc<VEC, K, false><<<nb, MR_T, 0, s>>>(stack, a, S, thr, lp, fg, lab, agreement);
}

#define MIRROR_DISPATCH(K, VEC4, CALL)                               \
    do {                                                             \
        if (VEC4) {                                                  \
            if ((K) == 1) { CALL(4, 1); } else if ((K) == 2) { CALL(4, 2); } else if ((K) == 4) { CALL(4, 4); } else { CALL(4, 8); } \
        } else {                                                     \
            if ((K) == 1) { CALL(1, 1); } else if ((K) == 2) { CALL(1, 2); } else if ((K) == 4) { CALL(1, 4); } else { CALL(1, 8); } \
        }                                                            \
    } while (0)

}  // namespace

// n_members is 1, 2, 4 or 8 and every argument is checked (engine.cpp)
void launch_mirror_combine(const float* stack, int C, int W, int H, int D, int n_members, const int* masks, int swap_axis, const int* pairs,
                           int n_pairs, float* mean, uint8_t* agreement, hipStream_t s) {
    const MirrorArgs a = mirror_args(C, W, H, D, n_members, masks, swap_axis, pairs, n_pairs);
    const int64_t S = (int64_t)W * H * D;
    // 16-B words need W % 4 == 0 (a word never straddles a row, and every plane starts a multiple of 16 B after its base)
    const bool v4 = W % 4 == 0 && ((uintptr_t)stack | (uintptr_t)mean) % 16 == 0 && (uintptr_t)agreement % 4 == 0;
#define CALL(V, KK) combine_vk<V, KK>(stack, a, S, mean, agreement, s)
    MIRROR_DISPATCH(n_members, v4, CALL);
#undef CALL
}

void launch_mirror_postproc(const float* stack, int C, int W, int H, int D, int n_members, const int* masks, int swap_axis,
                            const int* pairs, int n_pairs, float thr, float* lp, float* fg, uint16_t* lab, uint8_t* agreement,
                            hipStream_t s) {
    const MirrorArgs a = mirror_args(C, W, H, D, n_members, masks, swap_axis, pairs, n_pairs);
    const int64_t S = (int64_t)W * H * D;
    const bool v4 = W % 4 == 0 && ((uintptr_t)stack | (uintptr_t)lp | (uintptr_t)fg) % 16 == 0 && (uintptr_t)lab % 8 == 0 &&
                    (uintptr_t)agreement % 4 == 0;
#define CALL(V, KK) postproc_vk<V, KK>(stack, a, S, thr, lp, fg, lab, agreement, s)
    MIRROR_DISPATCH(n_members, v4, CALL);
#undef CALL
}

}  // namespace unet
