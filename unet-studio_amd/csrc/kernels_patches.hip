// The patch feed (include/unet_patches.h): the per-class index of a canvas label, the pick of a window around the r-th voxel of a
// class, and the crop of that window out of the canvas, whose origin stays on the device.
//
// Index: k_patches_count, one block per segment of 1024 voxels, counts the classes of its voxels in an LDS table (integer adds: the
// result does not depend on their order) and writes one count per class into the class-major table; k_patches_prefix, one block per
// class, turns that row of counts into an exclusive prefix in place, 1024 segments per round with a running carry, and writes the
// total.  Pick: one wave per pick.  Crop: one thread per 16 bytes of a row (per voxel when the window's width is no multiple of 4
// or the destination is not 16-byte aligned) in 4 consecutive slices, its 4 loads issued before its first store; grid (slice, z / 4,
// plane), so a thread does one division.  The source rows start at any
// 4-byte alignment: the 16-byte load is declared 4-byte aligned (global_load_dwordx4 takes any dword address), the store is aligned.
#include "device_util.h"

namespace unet {

namespace {

constexpr int SEG = UNET_PATCHES_SEGMENT;
constexpr int PATCH_T = 256;
static_assert(SEG == 4 * PATCH_T && UNET_PATCHES_MAX_CLASSES <= PATCH_T, "a block of 256 threads counts a segment, 4 voxels each");

// the class of a voxel (include/unet_patches.h CLASS); -1: none
__device__ __forceinline__ int patch_class(float l, int classes) {
    if (classes == 0) return l > 0.f ? 1 : 0;
    return (l > -1.f && l < (float)classes) ? (int)l : -1;   // NaN fails both comparisons
}

__global__ void __launch_bounds__(PATCH_T) k_patches_count(const float* __restrict__ label, int V, int classes, int K, int S,
                                                           int* __restrict__ index) {
    __shared__ int hist[PATCH_T];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * SEG;
#pragma unroll
    for (int j = 0; j < SEG / PATCH_T; ++j) {
        const int v = base + j * PATCH_T + threadIdx.x;
        if (v < V) {
            const int c = patch_class(label[v], classes);
            if (c >= 0) atomicAdd(&hist[c], 1);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) index[K + (int64_t)threadIdx.x * S + blockIdx.x] = hist[threadIdx.x];
}

// row blockIdx.x of the counts -> its exclusive prefix, in place; the total -> index[blockIdx.x]
__global__ void __launch_bounds__(PATCH_T) k_patches_prefix(int K, int S, int* __restrict__ index) {
    __shared__ int wsum[PATCH_T / 64];
    int* row = index + K + (int64_t)blockIdx.x * S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int s0 = 0; s0 < S; s0 += 4 * PATCH_T) {
        const int s = s0 + 4 * threadIdx.x;
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = s + j < S ? row[s + j] : 0;
        const int mine = c[0] + c[1] + c[2] + c[3];
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < PATCH_T / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        __syncthreads();
        int run = before + incl - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (s + j < S) row[s + j] = run;
            run += c[j];
        }
        carry += all;
    }
    if (threadIdx.x == 0) index[blockIdx.x] = carry;
}

struct PatchPicks { UnetPatchPick p[UNET_PATCHES_MAX_PICKS]; };

__device__ __forceinline__ int pick_jitter(int centre, unsigned u, int T, int C) {
    const int o = centre - (int)(((uint64_t)u * (uint64_t)T) >> 32);
    return min(max(o, 0), C - T);
}
__device__ __forceinline__ int pick_uniform(unsigned u, int T, int C) { return (int)(((uint64_t)u * (uint64_t)(C - T + 1)) >> 32); }

// one wave per pick (include/unet_patches.h PICK)
__global__ void __launch_bounds__(64) k_patches_pick(const float* __restrict__ label, const int* __restrict__ index, int classes, int K,
                                                     int S, int V, int W, int H, int D, int tw, int th, int td, PatchPicks picks,
                                                     int* __restrict__ origins) {
    const UnetPatchPick p = picks.p[blockIdx.x];
    const int lane = threadIdx.x;
    int* out = origins + 4 * blockIdx.x;
    const int n = (p.cls >= 0 && p.cls < K) ? index[p.cls] : 0;
    if (n <= 0) {
        if (lane == 0) {
            out[0] = pick_uniform(p.u_x, tw, W);
            out[1] = pick_uniform(p.u_y, th, H);
            out[2] = pick_uniform(p.u_z, td, D);
            out[3] = 0;
        }
        return;
    }
    const int r = (int)(((uint64_t)p.u_rank * (uint64_t)n) >> 32);
    const int* prefix = index + K + (int64_t)p.cls * S;
    // the last segment whose prefix is <= r: S <= 2^21, so 32 halvings always finish
    int lo = 0, hi = S - 1;
    for (int it = 0; it < 32; ++it) {
        if (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (prefix[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
    }
    const int base = lo * SEG;
    int rem = r - prefix[lo];      // the rank inside the segment; negative only with an index of another label
    int centre = base, flag = 0;
#pragma unroll 4
    for (int j = 0; j < SEG / 64; ++j) {
        const int v = base + j * 64 + lane;
        const bool match = v < V && patch_class(label[v], classes) == p.cls;
        const unsigned long long ball = __ballot(match);
        const int cnt = __popcll(ball);
        if (!flag && rem >= 0) {            // uniform: ball, rem and flag are the same in every lane
            if (rem < cnt) {
                const bool me = match && __popcll(ball & ((1ull << lane) - 1ull)) == rem;
                centre = base + j * 64 + (__ffsll((long long)__ballot(me)) - 1);
                flag = 1;
            } else {
                rem -= cnt;
            }
        }
    }
    if (lane == 0) {
        const int cx = centre % W, cy = (centre / W) % H, cz = centre / (W * H);
        out[0] = pick_jitter(cx, p.u_x, tw, W);
        out[1] = pick_jitter(cy, p.u_y, th, H);
        out[2] = pick_jitter(cz, p.u_z, td, D);
        out[3] = flag;
    }
}

struct __attribute__((packed, aligned(4))) U4 { uint32_t a, b, c, d; };   // 16 bytes at a 4-byte aligned address

constexpr int CROP_Z = 4;   // slices per thread

// grid (ceil(th * tw / VEC / 256), ceil(td / CROP_Z), planes): plane < channels is an image channel, plane == channels the label
template <int VEC>
__global__ void __launch_bounds__(PATCH_T) k_patches_crop(const uint32_t* __restrict__ image, int channels, const uint32_t* __restrict__ label,
                                                          int W, int H, int D, int tw, int th, int td, const int* __restrict__ origin,
                                                          uint32_t* __restrict__ x, uint32_t* __restrict__ lab) {
    // whatever the three words hold, the window lies inside the canvas
    const int ox = min(max(origin[0], 0), W - tw), oy = min(max(origin[1], 0), H - th), oz = min(max(origin[2], 0), D - td);
    const unsigned qw = (unsigned)tw / VEC;                       // VEC == 4: tw is a multiple of 4
    const unsigned e = blockIdx.x * PATCH_T + threadIdx.x;
    const unsigned yy = e / qw, q = e - yy * qw;
    if (yy >= (unsigned)th) return;
    const unsigned z0 = blockIdx.y * CROP_Z, plane = blockIdx.z;
    const int64_t V = (int64_t)W * H * D, n = (int64_t)tw * th * td;
    const uint32_t* src = plane < (unsigned)channels ? image + plane * V : label;
    uint32_t* dst = plane < (unsigned)channels ? x + plane * n : lab;
    const unsigned s = ((z0 + oz) * (unsigned)H + (yy + oy)) * (unsigned)W + ox + q * VEC;      // < V < 2^31
    const unsigned d = (z0 * (unsigned)th + yy) * (unsigned)tw + q * VEC;
    const unsigned ss = (unsigned)H * (unsigned)W, ds = (unsigned)th * (unsigned)tw;            // one slice further
    // the same row of CROP_Z consecutive slices: all loads are issued before the first store
    if constexpr (VEC == 4) {
        U4 v[CROP_Z];
#pragma unroll
        for (int j = 0; j < CROP_Z; ++j)
            if (z0 + j < (unsigned)td) v[j] = *(const U4*)(src + s + j * ss);
#pragma unroll
        for (int j = 0; j < CROP_Z; ++j)
            if (z0 + j < (unsigned)td) *(uint4*)(dst + d + j * ds) = make_uint4(v[j].a, v[j].b, v[j].c, v[j].d);
    } else {
        uint32_t v[CROP_Z];
#pragma unroll
        for (int j = 0; j < CROP_Z; ++j)
            if (z0 + j < (unsigned)td) v[j] = src[s + j * ss];
#pragma unroll
        for (int j = 0; j < CROP_Z; ++j)
            if (z0 + j < (unsigned)td) dst[d + j * ds] = v[j];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int64_t patches_segments(int64_t voxels) { return (voxels + SEG - 1) / SEG; }

size_t patches_index_bytes(int64_t voxels, int K) { return sizeof(int32_t) * (size_t)K * (size_t)(1 + patches_segments(voxels)); }

void launch_patches_index(const float* label, int64_t voxels, int classes, int32_t* index, hipStream_t s) {
    const int K = classes ? classes : 2, S = (int)patches_segments(voxels);
    k_patches_count<<<S, PATCH_T, 0, s>>>(label, (int)voxels, classes, K, S, index);
    k_patches_prefix<<<K, PATCH_T, 0, s>>>(K, S, index);
}

void launch_patches_pick(const float* label, const int32_t* index, int classes, int W, int H, int D, int tw, int th, int td,
                         const UnetPatchPick* picks, int n, int32_t* origins, hipStream_t s) {
    const int64_t V = (int64_t)W * H * D;
    PatchPicks pp = {};
    for (int i = 0; i < n; ++i) pp.p[i] = picks[i];
    k_patches_pick<<<n, 64, 0, s>>>(label, index, classes, classes ? classes : 2, (int)patches_segments(V), (int)V, W, H, D, tw, th, td, pp,
                                    origins);
}

void launch_patches_crop(const float* image, int channels, const float* label, int W, int H, int D, int tw, int th, int td,
                         const int32_t* origin, float* x, float* lab, hipStream_t s) {
    const int planes = channels + (lab ? 1 : 0);
    const bool v4 = tw % 4 == 0 && aligned16(x) && (!lab || aligned16(lab));
    const dim3 grid(cdiv64((int64_t)th * (tw / (v4 ? 4 : 1)), PATCH_T), (td + CROP_Z - 1) / CROP_Z, planes);
    if (v4) k_patches_crop<4><<<grid, PATCH_T, 0, s>>>((const uint32_t*)image, channels, (const uint32_t*)label, W, H, D, tw, th, td, origin,
                                                      (uint32_t*)x, (uint32_t*)lab);
    else k_patches_crop<1><<<grid, PATCH_T, 0, s>>>((const uint32_t*)image, channels, (const uint32_t*)label, W, H, D, tw, th, td, origin,
                                                   (uint32_t*)x, (uint32_t*)lab);
}

}  // namespace unet
