// The exact squared Euclidean distance transform of one label of a label map and the surface lists built on it
// (include/unet_distance.h).  All arithmetic is int32 on values the entry points have bounded: no sum below can wrap.
//
//   k_dist_x<LDS>     the feature predicate from the label map (of = surface: the six neighbours too) and the x pass in one launch:
//                     wx * (distance along x to the nearest feature of the line)^2, or INF for a line without one.
//                     LDS: a block takes DT_LINES or fewer whole lines at a time; a wave takes 64 consecutive voxels of a line, its
//                     ballot is the word of feature flags, and the words of the block's lines sit in LDS; then every thread finds the
//                     nearest set bit to its left and to its right by word scans (clz / ffs): nobody walks voxels.
//                     GLOBAL: one thread per voxel walks outward along x, evaluating the predicate as it goes.
//   k_dist_axis<LDS>  the y and the z pass: out[p] = min_i (w (p - i)^2 + g[i]) along a line, by the search outward from p (dist_search).
//                     LDS: a block loads a slab, TX consecutive x by the whole line, [i][x] so that lanes on consecutive x read
//                     consecutive dwords for the same i; TX is the launcher's (dist_slab_shift).  GLOBAL: one thread per voxel.
//   k_dist_counts     |S(a, l)| and |S(b, l)| per label from one pass over both maps: a block's LDS table for the rows below
//                     UNET_DIST_LDS_ROWS, global atomics for the rest
//   k_dist_gather     dist[v] for every v of S(at, label) appended through an atomic cursor, one atomic per wave
// Every atomic is an integer add: the counts do not depend on the schedule, the gathered list only in its order.
//
// Passes: labels -> out (x), out -> scratch (y), scratch -> out (z).
#include <algorithm>

#include "../../include/unet_distance.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int DT_T = 256;                             // threads per block
constexpr int DT_MAXB = 4096;                         // grid cap of the kernels that stride
constexpr int DT_MASK_WORDS = 1024;                   // 64-bit words of feature flags a block holds: 8 KiB
constexpr int DT_LINES = 32;                          // lines a block takes at once at the most
constexpr int DT_INF = UNET_DIST_INF;
constexpr int DT_ROWS = UNET_DIST_LDS_ROWS;
static_assert(DT_T % 64 == 0, "whole waves: the ballots below need every lane");
static_assert(UNET_DIST_LDS_MAX_LINE * 8 * 4 <= 64 * 1024, "the slab of a block");

typedef unsigned long long u64;

size_t dist_align(size_t b) { return (b + 255) & ~(size_t)255; }

// a label as read: uint8 or uint16 at any alignment; a value above L reads as 0
__device__ __forceinline__ unsigned dist_label(const void* __restrict__ p, int bytes, int64_t i, unsigned L) {
    const unsigned v = bytes == 1 ? (unsigned)((const uint8_t*)p)[i]
                                  : (unsigned)((const uint8_t*)p)[2 * i] | ((unsigned)((const uint8_t*)p)[2 * i + 1] << 8);
    return v > L ? 0u : v;
}

// is (x, y, z), which reads l, on the surface of l: on a face of the volume, or a 6-neighbour does not read l
__device__ __forceinline__ bool dist_on_surface(const void* __restrict__ p, int bytes, int w, int h, int d, int x, int y, int z, int64_t i,
                                                unsigned l, unsigned L) {
    if (x == 0 || y == 0 || z == 0 || x == w - 1 || y == h - 1 || z == d - 1) return true;
    const int64_t sy = w, sz = (int64_t)w * h;
    return dist_label(p, bytes, i - 1, L) != l || dist_label(p, bytes, i + 1, L) != l || dist_label(p, bytes, i - sy, L) != l ||
           dist_label(p, bytes, i + sy, L) != l || dist_label(p, bytes, i - sz, L) != l || dist_label(p, bytes, i + sz, L) != l;
}

// the feature predicate of the transform at an in-grid voxel
__device__ __forceinline__ bool dist_feature(const void* __restrict__ p, int bytes, int w, int h, int d, int x, int y, int z, unsigned label,
                                             bool surface) {
    const int64_t i = ((int64_t)z * h + y) * w + x;
    if (dist_label(p, bytes, i, 65535u) != label) return false;
    return !surface || dist_on_surface(p, bytes, w, h, d, x, y, z, i, label, 65535u);
}

// ---- the x pass ------------------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(DT_T) k_dist_x(const void* __restrict__ labels, int bytes, int w, int h, int d, unsigned label, int surface,
                                                 int wx, int* __restrict__ out, int wpl, int G) {
    if constexpr (LDS) {
        __shared__ u64 mask[DT_MASK_WORDS];               // [line of the chunk][word]: G * wpl <= DT_MASK_WORDS
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int lines = h * d, chunks = (lines + G - 1) / G;
        for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
            const int line0 = c * G, nseg = min(G, lines - line0) * wpl;
            for (int s = wave; s < nseg; s += DT_T / 64) {    // uniform over the wave: every lane reaches the ballot
                const int li = s / wpl, x = (s - li * wpl) * 64 + lane, line = line0 + li;
                const bool f = x < w && dist_feature(labels, bytes, w, h, d, x, line % h, line / h, label, surface != 0);
                const u64 m = __ballot(f);
                if (lane == 0) mask[s] = m;
            }
            __syncthreads();
            for (int s = wave; s < nseg; s += DT_T / 64) {
                const int li = s / wpl, wd = s - li * wpl, x = wd * 64 + lane;
                if (x >= w) continue;
                const u64* row = mask + li * wpl;
                const u64 own = row[wd];
                int dl = -1, dr = -1;                     // the distance to the nearest feature at or left of x, at or right of x
                u64 m = own & (~0ull >> (63 - lane));
                for (int k = wd;;) {
                    if (m) { dl = x - (k * 64 + 63 - __clzll((long long)m)); break; }
                    if (--k < 0) break;
                    m = row[k];
                }
                m = own & (~0ull << lane);
                for (int k = wd;;) {
                    if (m) { dr = k * 64 + __ffsll((long long)m) - 1 - x; break; }
                    if (++k >= wpl) break;
                    m = row[k];
                }
                const int dist = dl < 0 ? dr : dr < 0 ? dl : min(dl, dr);
                out[(int64_t)(line0 + li) * w + x] = dist < 0 ? DT_INF : wx * dist * dist;
            }
            __syncthreads();                              // the words are rewritten by the next chunk
        }
    } else {
        const int64_t v = (int64_t)blockIdx.x * DT_T + threadIdx.x;
        if (v >= (int64_t)w * h * d) return;
        const int x = (int)(v % w), line = (int)(v / w), y = line % h, z = line / h;
        int dist = -1;
        for (int k = 0; k < w; ++k) {                     // outward: the first hit is the nearest
            const bool lo = x - k >= 0, hi = x + k < w;
            if (!lo && !hi) break;
            if ((lo && dist_feature(labels, bytes, w, h, d, x - k, y, z, label, surface != 0)) ||
                (hi && dist_feature(labels, bytes, w, h, d, x + k, y, z, label, surface != 0))) {
                dist = k;
                break;
            }
        }
        out[v] = dist < 0 ? DT_INF : wx * dist * dist;
    }
}

// ---- the y and z passes ----------------------------------------------------------------------------------------------------------
// min_i (wgt (p - i)^2 + g(i)) over a line of n: delta = 0, 1, 2, ... on both sides of p until wgt delta^2 >= the best so far (nothing
// farther can be smaller) or both ends are passed.  An INF entry is skipped; a finite one plus wgt delta^2 stays below INF (the metric
// bound), so the result needs no clamp beyond INF itself.
template <typename Load> __device__ __forceinline__ int dist_search(int p, int n, int wgt, Load g) {
    int best = g(p);
    for (int k = 1; k < n; ++k) {
        const int c = wgt * k * k;                        // <= wgt (n - 1)^2 < INF
        if (c >= best) break;
        const int lo = p - k, hi = p + k;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            const int v = g(lo);
            if (v != DT_INF) best = min(best, c + v);
        }
        if (hi < n) {
            const int v = g(hi);
            if (v != DT_INF) best = min(best, c + v);
        }
    }
    return min(best, DT_INF);
}

// stride: between the entries of a line; `outer`: the extent of the coordinate that is neither x nor the line's, ostride its stride;
// inner: the line's coordinate is the faster of those two (the y pass).
// LDS: block = (slab of x, outer); TX a power of two, n * TX * 4 bytes of dynamic LDS
template <bool LDS>
__global__ void __launch_bounds__(DT_T) k_dist_axis(const int* __restrict__ in, int* __restrict__ out, int w, int n, int64_t stride, int outer,
                                                    int64_t ostride, int wgt, int inner, int tx_shift, int nsx) {
    if constexpr (LDS) {
        extern __shared__ int slab[];                     // [i][x]
        const int TX = 1 << tx_shift, sx = blockIdx.x % nsx, o = blockIdx.x / nsx, x0 = sx * TX;
        const int64_t base = (int64_t)o * ostride + x0;
        const int total = n << tx_shift;                  // <= 16384
        for (int e = threadIdx.x; e < total; e += DT_T) {
            const int i = e >> tx_shift, tx = e & (TX - 1);
            slab[e] = x0 + tx < w ? in[base + (int64_t)i * stride + tx] : DT_INF;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < total; e += DT_T) {
            const int p = e >> tx_shift, tx = e & (TX - 1);
            if (x0 + tx >= w) continue;
            out[base + (int64_t)p * stride + tx] = dist_search(p, n, wgt, [&](int i) { return slab[(i << tx_shift) + tx]; });
        }
    } else {
        const int64_t v = (int64_t)blockIdx.x * DT_T + threadIdx.x;
        if (v >= (int64_t)w * n * outer) return;
        const int r = (int)(v / w), p = inner ? r % n : r / outer;
        const int64_t base = v - (int64_t)p * stride;
        out[v] = dist_search(p, n, wgt, [&](int i) { return in[base + (int64_t)i * stride]; });
    }
}

// ---- the surface counts ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_T) k_dist_zero(u64* __restrict__ rows, int n) {
    const int i = blockIdx.x * DT_T + threadIdx.x;
    if (i < n) rows[i] = 0ull;
}

__global__ void __launch_bounds__(DT_T) k_dist_counts(const void* __restrict__ a, int a_bytes, const void* __restrict__ b, int b_bytes, int w,
                                                      int h, int d, unsigned L, u64* rows) {
    __shared__ unsigned lc[DT_ROWS * 2];
    const int held = min((int)L + 1, DT_ROWS);
    for (int e = threadIdx.x; e < held * 2; e += DT_T) lc[e] = 0u;
    __syncthreads();
    const int64_t voxels = (int64_t)w * h * d;
    for (int64_t v = (int64_t)blockIdx.x * DT_T + threadIdx.x; v < voxels; v += (int64_t)gridDim.x * DT_T) {
        const int x = (int)(v % w), line = (int)(v / w), y = line % h, z = line / h;
        const unsigned la = dist_label(a, a_bytes, v, L), lb = dist_label(b, b_bytes, v, L);
        if (dist_on_surface(a, a_bytes, w, h, d, x, y, z, v, la, L)) {
            if (la < (unsigned)DT_ROWS) atomicAdd(&lc[la * 2u], 1u);
            else atomicAdd(rows + (size_t)la * 2, 1ull);
        }
        if (dist_on_surface(b, b_bytes, w, h, d, x, y, z, v, lb, L)) {
            if (lb < (unsigned)DT_ROWS) atomicAdd(&lc[lb * 2u + 1u], 1u);
            else atomicAdd(rows + (size_t)lb * 2 + 1, 1ull);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < held * 2; e += DT_T)
        if (const unsigned c = lc[e]) atomicAdd(rows + e, (u64)c);
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_T) k_dist_gather(const void* __restrict__ at, int bytes, int w, int h, int d, unsigned label,
                                                      const int* __restrict__ dist, int* __restrict__ values, int64_t capacity, u64* cursor) {
    const int64_t v = (int64_t)blockIdx.x * DT_T + threadIdx.x;
    bool f = false;
    if (v < (int64_t)w * h * d) {
        const int x = (int)(v % w), line = (int)(v / w);
        f = dist_feature(at, bytes, w, h, d, x, line % h, line / h, label, true);
    }
    const u64 m = __ballot(f);                            // every lane of the wave is here: nobody has left
    if (!m) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    unsigned lo = 0u, hi = 0u;
    if (lane == leader) {                                 // one atomic per wave
        const u64 first = atomicAdd(cursor, (u64)__popcll(m));
        lo = (unsigned)first;
        hi = (unsigned)(first >> 32);
    }
    lo = (unsigned)__shfl((int)lo, leader);
    hi = (unsigned)__shfl((int)hi, leader);
    if (!f) return;
    const u64 slot = (((u64)hi << 32) | lo) + (u64)__popcll(m & ((1ull << lane) - 1ull));
    if (slot < (u64)capacity) values[slot] = dist[v];
}

// the slab width of a y or z pass over lines of n, as log2: the widest power of two <= UNET_DIST_SLAB_MAX_X with n * TX * 4 <= 64 KiB,
// not wider than w needs; below 8 (-1) the line is too long for a block's LDS
int dist_slab_shift(int n, int w) {
    int sh = 5;
    static_assert(UNET_DIST_SLAB_MAX_X == 32, "sh above");
    while (sh >= 3 && ((int64_t)n << sh) * 4 > 64 * 1024) --sh;
    if (sh < 3) return -1;
    while (sh > 3 && (1 << (sh - 1)) >= w) --sh;
    return sh;
}

void dist_axis(const int* in, int* out, int w, int n, int64_t stride, int outer, int64_t ostride, int wgt, int inner, bool lds, hipStream_t s) {
    const int sh = lds ? dist_slab_shift(n, w) : -1;
    if (sh >= 0) {
        const int nsx = (w + (1 << sh) - 1) >> sh;        // nsx * outer <= voxels < 2^31
        k_dist_axis<true><<<nsx * outer, DT_T, ((size_t)n << sh) * 4, s>>>(in, out, w, n, stride, outer, ostride, wgt, inner, sh, nsx);
    } else {
        k_dist_axis<false><<<cdiv64((int64_t)w * n * outer, DT_T), DT_T, 0, s>>>(in, out, w, n, stride, outer, ostride, wgt, inner, 0, 0);
    }
}

}  // namespace

size_t dist_scratch_bytes(int64_t voxels) { return 256 + dist_align((size_t)voxels * 4); }

void launch_dist_transform(const void* labels, int label_bytes, int w, int h, int d, int label, int of, int wx, int wy, int wz, int32_t* out,
                           int impl, void* scratch, hipStream_t s) {
    int* tmp = (int*)dist_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    const bool lds = impl != UNET_DIST_IMPL_GLOBAL;            // DEFAULT: LDS
    const int surface = of == UNET_DIST_OF_SURFACE;
    const int64_t voxels = (int64_t)w * h * d;
    const int wpl = (w + 63) / 64;
    if (lds && wpl <= DT_MASK_WORDS) {
        const int G = std::min(DT_LINES, DT_MASK_WORDS / wpl), chunks = (h * d + G - 1) / G;
        k_dist_x<true><<<std::min(chunks, DT_MAXB), DT_T, 0, s>>>(labels, label_bytes, w, h, d, (unsigned)label, surface, wx, out, wpl, G);
    } else {
        k_dist_x<false><<<cdiv64(voxels, DT_T), DT_T, 0, s>>>(labels, label_bytes, w, h, d, (unsigned)label, surface, wx, out, 0, 0);
    }
    dist_axis(out, tmp, w, h, w, d, (int64_t)w * h, wy, 1, lds, s);   // y: the lines of a z-plane
    dist_axis(tmp, out, w, d, (int64_t)w * h, h, w, wz, 0, lds, s);   // z: the lines of a y-plane
}

void launch_dist_surface_counts(const void* a, int a_bytes, const void* b, int b_bytes, int w, int h, int d, int n_labels, int64_t* rows,
                                hipStream_t s) {
    const int n = (n_labels + 1) * 2;
    k_dist_zero<<<(n + DT_T - 1) / DT_T, DT_T, 0, s>>>((u64*)rows, n);
    const unsigned nb = cdiv64((int64_t)w * h * d, DT_T * 8);
    k_dist_counts<<<std::min(nb, (unsigned)DT_MAXB), DT_T, 0, s>>>(a, a_bytes, b, b_bytes, w, h, d, (unsigned)n_labels, (u64*)rows);
}

void launch_dist_gather(const void* at, int at_bytes, int w, int h, int d, int label, const int32_t* dist, int32_t* values, int64_t capacity,
                        unsigned long long* cursor, hipStream_t s) {
    k_dist_gather<<<cdiv64((int64_t)w * h * d, DT_T), DT_T, 0, s>>>(at, at_bytes, w, h, d, (unsigned)label, dist, values, capacity, cursor);
}

}  // namespace unet
