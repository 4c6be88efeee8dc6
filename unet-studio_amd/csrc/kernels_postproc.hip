// The inference post-processing chain (include/unet_postproc.h; evaluate.cpp:274,303-376) on the level-0 logits.
//
//   k_pp_softmax    softmax + create_mask + argmax in one streaming pass: per voxel an online max m with the sums of
//                   exp(x - m) over all channels and over the foreground rescaled whenever m grows, and the argmax of x over c >= 1.
//                   label and fg_prob need that one read; label_prob reads the foreground planes a second time (same thread)
//   k_cc_*          defragment: 6-connected components by union-find label equivalence (hooking by compare-and-swap of roots,
//                   the larger root onto the smaller, with path halving; then a flatten in two passes), so every root is its component's
//                   smallest linear index whatever the schedule.  Sizes are uint32 counts at the root: each thread folds its run of
//                   CC_RUN consecutive voxels, the lanes of a wave with the same root add once.  Largest count by block partials and
//                   a fold; then the zeroing pass.  Nothing depends on the order of the atomics: the result is bitwise reproducible
//   k_pp_elem       the per-plane element-wise ops, keyed by op; normalize_each's plane maxima by block partials and a fold
//   k_pp_smooth     gaussian_smoothing through binomial3 (device_util.h), the body simulate_modality's smoothing uses
//
// Scratch: UNET_POSTPROC_CHUNK slots per call at most (one for defragment), each {parent int32[S], count uint32[S],
// partial[PP_MAXB], max}: defragment_each, normalize_each and smoothing go over the planes that many at a time.
#include "cc_union_find.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int PP_T = 256;          // threads per block
constexpr int PP_MAXB = 2048;      // grid cap of the streaming kernels (256 CUs x 8 blocks); they stride over the rest

__host__ __device__ inline size_t pp_align(size_t b) { return (b + 255) & ~(size_t)255; }
size_t pp_slot_bytes(int64_t S) { return 2 * pp_align((size_t)S * 4) + pp_align((PP_MAXB + 1) * 4); }

struct Slot {
    int* parent;
    unsigned* count;
    unsigned* partial;   // PP_MAXB block partials, then the folded value
};
Slot pp_slot(void* scratch, int64_t S, int k) {
    char* b = (char*)pp_align((size_t)(uintptr_t)scratch) + (size_t)k * pp_slot_bytes(S);   // any scratch alignment: 256 B of slack
    Slot s;
    s.parent = (int*)b;
    s.count = (unsigned*)(b + pp_align((size_t)S * 4));
    s.partial = (unsigned*)(b + 2 * pp_align((size_t)S * 4));
    return s;
}
// slot k's arrays relative to slot 0's, in 4-byte words (the kernels take slot 0 and blockIdx.y as the slot)
size_t pp_slot_words(int64_t S) { return pp_slot_bytes(S) / 4; }

int pp_blocks(int64_t n, int per_block) {
    const int64_t nb = (n + per_block - 1) / per_block;
    return (int)(nb > PP_MAXB ? PP_MAXB : nb < 1 ? 1 : nb);
}

// ---- softmax / create_mask / argmax --------------------------------------------------------------------------------------------
// ldv, stv, pp_acc and pp_voxels, the per-voxel body: device_util.h (shared with kernels_space.hip and kernels_mirror.hip)
template <int VEC>
__global__ void __launch_bounds__(PP_T) k_pp_softmax(const float* __restrict__ lg, int C, int64_t S, float thr,
                                                     float* __restrict__ lp, float* __restrict__ fg, uint16_t* __restrict__ lab) {
    const int64_t step = (int64_t)gridDim.x * PP_T * VEC;
    for (int64_t v = ((int64_t)blockIdx.x * PP_T + threadIdx.x) * VEC; v < S; v += step) {   // VEC == 4 only when S % 4 == 0
        const auto load = [&](int c, float (&x)[VEC]) { ldv<VEC>(lg, (int64_t)c * S + v, x); };
        pp_voxels<VEC>(C, S, v, thr, lp, fg, lab, load, load);
    }
}

// label = fg > thr ? 1 + argmax_c lp_c : 0 from the current planes (argmax after a command that changed them); the first plane wins
// a tie, a NaN fg gives 0
__global__ void __launch_bounds__(PP_T) k_pp_argmax_planes(const float* __restrict__ lp, int np, int64_t S, const float* __restrict__ fg,
                                                           float thr, uint16_t* __restrict__ lab) {
    for (int64_t v = (int64_t)blockIdx.x * PP_T + threadIdx.x; v < S; v += (int64_t)gridDim.x * PP_T) {
        float best = lp[v];
        int arg = 0;
        for (int c = 1; c < np; ++c) {
            const float x = lp[(int64_t)c * S + v];
            if (x > best) { best = x; arg = c; }
        }
        lab[v] = fg[v] > thr ? (uint16_t)(arg + 1) : (uint16_t)0;
    }
}

// ---- connected components --------------------------------------------------------------------------------------------------
// cc_ld, cc_st, cc_find, cc_union, cc_count_runs: cc_union_find.h (shared with kernels_components.hip)

// parent = i in the mask (src > thr), -1 outside; count = 0.  blockIdx.y: the plane / slot of this round
__global__ void __launch_bounds__(PP_T) k_cc_init(const float* __restrict__ src, int64_t S, float thr, int* __restrict__ parent0,
                                                  size_t slot_words) {
    const float* p = src + (int64_t)blockIdx.y * S;
    int* parent = parent0 + blockIdx.y * slot_words;
    unsigned* count = (unsigned*)parent + pp_align((size_t)S * 4) / 4;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) {
        parent[i] = p[i] > thr ? (int)i : -1;
        count[i] = 0u;
    }
}

// every mask voxel joins its -x, -y and -z face neighbours that are in the mask
__global__ void __launch_bounds__(PP_T) k_cc_link(int W, int H, int S, int* __restrict__ parent0, size_t slot_words) {
    int* parent = parent0 + blockIdx.y * slot_words;
    const int WH = W * H;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) {
        if (parent[i] < 0) continue;   // mask membership never changes: hooking only lowers values that are >= 0
        const int v = (int)i, x = v % W, y = (v / W) % H;   // 64-bit loop counter: the last stride may pass 2^31
        if (x > 0 && parent[v - 1] >= 0) cc_union(parent, v, v - 1);
        if (y > 0 && parent[v - W] >= 0) cc_union(parent, v, v - W);
        if (v >= WH && parent[v - WH] >= 0) cc_union(parent, v, v - WH);
    }
}

// parent = root.  HALVE: a first pass that halves the paths (its stores race with other threads' halving, which may leave an
// entry at an ancestor that is not the root); then a pass that only walks and writes each entry's own root, so nothing races
template <bool HALVE>
__global__ void __launch_bounds__(PP_T) k_cc_flatten(int S, int* __restrict__ parent0, size_t slot_words) {
    int* parent = parent0 + blockIdx.y * slot_words;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) {
        const int p = cc_ld(parent + i);
        if (p < 0) continue;
        if constexpr (HALVE) {
            cc_find(parent, (int)i);
        } else {
            int r = p, next;
            while (r > (next = cc_ld(parent + r))) r = next;
            if (r != p) cc_st(parent + i, r);
        }
    }
}

// count[root] += the component's voxels: a thread folds its CC_RUN consecutive voxels into runs of one root (a run that ends
// inside adds at once), and the lanes whose last runs share a root add them with one atomic
__global__ void __launch_bounds__(PP_T) k_cc_count(int S, int* __restrict__ parent0, size_t slot_words) {
    const int* parent = parent0 + blockIdx.y * slot_words;
    unsigned* count = (unsigned*)parent0 + blockIdx.y * slot_words + pp_align((size_t)S * 4) / 4;
    cc_count_runs<PP_T>(S, parent, count);
}

__device__ __forceinline__ unsigned block_max_u(unsigned v) {
    __shared__ unsigned red[PP_T / 64];
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int w = 1; w < PP_T / 64; ++w) v = max(v, red[w]);
    return v;
}
__device__ __forceinline__ float block_max_f(float v) {   // fmaxf: NaN voxels are skipped
    __shared__ float redf[PP_T / 64];
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = v;
    __syncthreads();
    v = redf[0];
    for (int w = 1; w < PP_T / 64; ++w) v = fmaxf(v, redf[w]);
    return v;
}

// per-block max of the counts -> partial[blockIdx.x]
__global__ void __launch_bounds__(PP_T) k_cc_pmax(int S, int* __restrict__ parent0, size_t slot_words) {
    unsigned* slot = (unsigned*)parent0 + blockIdx.y * slot_words;
    const unsigned* count = slot + pp_align((size_t)S * 4) / 4;
    unsigned* partial = slot + 2 * pp_align((size_t)S * 4) / 4;
    unsigned v = 0;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) v = max(v, count[i]);
    v = block_max_u(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// partial[PP_MAXB] = the max of the nb partials; one block per slot (IS_F: float maxima, else uint32)
template <bool IS_F>
__global__ void __launch_bounds__(PP_T) k_pp_fold(int64_t S, int nb, unsigned* __restrict__ slot0, size_t slot_words) {
    unsigned* partial = slot0 + blockIdx.x * slot_words + 2 * pp_align((size_t)S * 4) / 4;
    if constexpr (IS_F) {
        float v = -INFINITY;
        for (int b = threadIdx.x; b < nb; b += PP_T) v = fmaxf(v, __uint_as_float(partial[b]));
        v = block_max_f(v);
        if (threadIdx.x == 0) partial[PP_MAXB] = __float_as_uint(v);
    } else {
        unsigned v = 0;
        for (int b = threadIdx.x; b < nb; b += PP_T) v = max(v, partial[b]);
        v = block_max_u(v);
        if (threadIdx.x == 0) partial[PP_MAXB] = v;
    }
}

// zero the voxels of the mask whose component is not kept: count[root] >= size_ratio * largest, in double.
// each == 0: fg, the np planes of lp and lab (each may be NULL); each != 0: plane blockIdx.y of lp only
__global__ void __launch_bounds__(PP_T) k_cc_zero(int S, double ratio, int* __restrict__ parent0, size_t slot_words, int each,
                                                  float* __restrict__ fg, float* __restrict__ lp, int np, uint16_t* __restrict__ lab) {
    const int* parent = parent0 + blockIdx.y * slot_words;
    const unsigned* count = (const unsigned*)parent + pp_align((size_t)S * 4) / 4;
    const double need = ratio * (double)((const unsigned*)parent + 2 * pp_align((size_t)S * 4) / 4)[PP_MAXB];
    float* plane = each ? lp + (int64_t)blockIdx.y * S : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) {
        const int r = parent[i];
        if (r < 0 || (double)count[r] >= need) continue;
        if (each) {
            plane[i] = 0.f;
        } else {
            if (fg) fg[i] = 0.f;
            if (lab) lab[i] = 0;
            if (lp)
                for (int p = 0; p < np; ++p) lp[(int64_t)p * S + i] = 0.f;
        }
    }
}

// ---- per-plane ops -----------------------------------------------------------------------------------------------------------
enum { PP_COPY = 0 };   // internal: plane = the slot's smoothed copy

__global__ void __launch_bounds__(PP_T) k_pp_pmaxf(const float* __restrict__ lp, int64_t S, unsigned* __restrict__ slot0,
                                                   size_t slot_words) {
    const float* x = lp + (int64_t)blockIdx.y * S;
    unsigned* partial = slot0 + blockIdx.y * slot_words + 2 * pp_align((size_t)S * 4) / 4;
    float v = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) v = fmaxf(v, x[i]);
    v = block_max_f(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = __float_as_uint(v);
}

__global__ void __launch_bounds__(PP_T) k_pp_elem(int op, float t, float* __restrict__ lp, int64_t S, const unsigned* __restrict__ slot0,
                                                  size_t slot_words) {
    float* x = lp + (int64_t)blockIdx.y * S;
    const unsigned* slot = slot0 + blockIdx.y * slot_words;
    float mx = 0.f;
    if (op == UNET_PP_NORMALIZE) mx = __uint_as_float(slot[2 * pp_align((size_t)S * 4) / 4 + PP_MAXB]);
    if (op == UNET_PP_NORMALIZE && !(mx > 0.f)) return;   // block-uniform
    const float* tmp = (const float*)slot;
    for (int64_t i = (int64_t)blockIdx.x * PP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * PP_T) {
        const float v = x[i];
        float r;
        switch (op) {
            case UNET_PP_UPPER_THRESHOLD: r = v > t ? t : v; break;
            case UNET_PP_LOWER_THRESHOLD: r = v < t ? t : v; break;
            case UNET_PP_MINUS: r = v - t; break;
            case UNET_PP_BINARIZE: r = v > t ? 1.f : 0.f; break;
            case UNET_PP_NORMALIZE: r = v / mx; break;
            default: r = tmp[i]; break;   // PP_COPY
        }
        x[i] = r;
    }
}

__global__ void __launch_bounds__(PP_T) k_pp_smooth(int W, int H, int D, const float* __restrict__ src, float* __restrict__ dst) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (x >= W || y >= H) return;
    dst[((int64_t)z * H + y) * W + x] = binomial3(W, H, D, x, y, z, [&](unsigned i) { return src[i]; });
}

}  // namespace

size_t postproc_scratch_bytes(int planes, int64_t S) {
    const int slots = planes < UNET_POSTPROC_CHUNK ? planes : UNET_POSTPROC_CHUNK;
    return 256 + (size_t)(slots < 1 ? 1 : slots) * pp_slot_bytes(S);
}

void launch_postproc_softmax(const float* logits, int C, int64_t S, float thr, float* lp, float* fg, uint16_t* lab, hipStream_t s) {
    // 16-B loads and stores when every plane starts 16-B aligned (8 B for the uint16 label): S % 4 == 0 and aligned bases.
    // Otherwise the whole pass is scalar: with S % 4 != 0 plane c starts at a different offset mod 16 B for every c, so one vector
    // body with a head and a tail per thread would not line up across the channels it reads (cost measured in DESIGN.md §14)
    const bool v4 = S % 4 == 0 && ((uintptr_t)logits | (uintptr_t)lp | (uintptr_t)fg) % 16 == 0 && (uintptr_t)lab % 8 == 0;
    if (v4) k_pp_softmax<4><<<pp_blocks(S, PP_T * 4), PP_T, 0, s>>>(logits, C, S, thr, lp, fg, lab);
    else k_pp_softmax<1><<<pp_blocks(S, PP_T), PP_T, 0, s>>>(logits, C, S, thr, lp, fg, lab);
}

void launch_postproc_argmax_planes(const float* lp, int np, int64_t S, const float* fg, float thr, uint16_t* lab, hipStream_t s) {
    k_pp_argmax_planes<<<pp_blocks(S, PP_T), PP_T, 0, s>>>(lp, np, S, fg, thr, lab);
}

void launch_postproc_defragment(int W, int H, int D, int each, float thr, double ratio, float* fg, float* lp, int np, uint16_t* lab,
                                void* scratch, hipStream_t s) {
    const int S = W * H * D;   // < 2^31 (checked by the caller)
    const size_t sw = pp_slot_words(S);
    int* parent0 = pp_slot(scratch, S, 0).parent;
    const int nb = pp_blocks(S, PP_T), nbc = pp_blocks(S, PP_T * CC_RUN);
    const int rounds = each ? np : 1;
    for (int p0 = 0; p0 < rounds; p0 += UNET_POSTPROC_CHUNK) {
        const unsigned k = (unsigned)(each ? (rounds - p0 < UNET_POSTPROC_CHUNK ? rounds - p0 : UNET_POSTPROC_CHUNK) : 1);
        k_cc_init<<<dim3(nb, k), PP_T, 0, s>>>(each ? lp + (int64_t)p0 * S : fg, S, thr, parent0, sw);
        k_cc_link<<<dim3(nb, k), PP_T, 0, s>>>(W, H, S, parent0, sw);
        k_cc_flatten<true><<<dim3(nb, k), PP_T, 0, s>>>(S, parent0, sw);
        k_cc_flatten<false><<<dim3(nb, k), PP_T, 0, s>>>(S, parent0, sw);
        k_cc_count<<<dim3(nbc, k), PP_T, 0, s>>>(S, parent0, sw);
        k_cc_pmax<<<dim3(nb, k), PP_T, 0, s>>>(S, parent0, sw);
        k_pp_fold<false><<<k, PP_T, 0, s>>>(S, nb, (unsigned*)parent0, sw);
        if (each) k_cc_zero<<<dim3(nb, k), PP_T, 0, s>>>(S, ratio, parent0, sw, 1, nullptr, lp + (int64_t)p0 * S, 0, nullptr);
        else k_cc_zero<<<dim3(nb, 1), PP_T, 0, s>>>(S, ratio, parent0, sw, 0, fg, lp, np, lab);
    }
}

void launch_postproc_plane_op(int op, float t, int W, int H, int D, float* lp, int np, void* scratch, hipStream_t s) {
    const int64_t S = (int64_t)W * H * D;
    const size_t sw = pp_slot_words(S);
    unsigned* slot0 = (unsigned*)pp_slot(scratch, S, 0).parent;
    const int nb = pp_blocks(S, PP_T);
    for (int p0 = 0; p0 < np; p0 += UNET_POSTPROC_CHUNK) {
        const unsigned k = (unsigned)(np - p0 < UNET_POSTPROC_CHUNK ? np - p0 : UNET_POSTPROC_CHUNK);
        float* x = lp + p0 * S;
        if (op == UNET_PP_NORMALIZE) {
            k_pp_pmaxf<<<dim3(nb, k), PP_T, 0, s>>>(x, S, slot0, sw);
            k_pp_fold<true><<<k, PP_T, 0, s>>>(S, nb, slot0, sw);
        }
        if (op == UNET_PP_SMOOTH) {
            const dim3 rows((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)D);
            for (unsigned j = 0; j < k; ++j) k_pp_smooth<<<rows, PP_T, 0, s>>>(W, H, D, x + j * S, (float*)(slot0 + j * sw));
        }
        k_pp_elem<<<dim3(nb, k), PP_T, 0, s>>>(op == UNET_PP_SMOOTH ? (int)PP_COPY : op, t, x, S, slot0, sw);
    }
}

}  // namespace unet
