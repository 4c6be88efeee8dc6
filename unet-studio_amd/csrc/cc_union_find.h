// Union-find label equivalence for connected components, shared by kernels_postproc.hip (defragment: one binary mask, 6-connected)
// and kernels_components.hip (equal values of a label map, 6-, 18- or 26-connected).  parent[j] <= j always: a tree's root is the
// smallest index hooked into it so far, and when all hooking is done the component's smallest linear index, whatever the schedule.
// The functions take global or LDS arrays alike (they are inlined; the compiler resolves the address space).
#pragma once
#include <hip/hip_runtime.h>

namespace unet {

constexpr int CC_RUN = 16;         // consecutive voxels per thread in the size count

__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The backward half N-(CONN) of a 6-, 18- or 26-neighbourhood: the offsets (dx, dy, dz) in {-1, 0, 1}^3 with
// 1 <= |dx| + |dy| + |dz| <= 1, 2, 3 whose neighbour has the smaller linear index (dz = -1, or dz = 0 and dy = -1, or dz = dy = 0
// and dx = -1): 3, 9, 13 offsets.  A voxel that hooks to every neighbour of N- is hooked from every neighbour of the other half.
// f(dx, dy, dz) is called once per offset; the loops unroll, so f sees constants
template <int CONN, class F>
__device__ __forceinline__ void cc_for_backward(F&& f) {
    static_assert(CONN == 6 || CONN == 18 || CONN == 26, "connectivity is 6, 18 or 26");
    constexpr int reach = CONN == 6 ? 1 : CONN == 18 ? 2 : 3;
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int n1 = (dx ? 1 : 0) + (dy ? 1 : 0) + (dz ? 1 : 0);
                const bool back = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                if (back && n1 >= 1 && n1 <= reach) f(dx, dy, dz);
            }
}

// root of i, halving the path on the way.  parent[j] <= j always, so every store points j at one of its ancestors.
// Terminates: cur strictly decreases with every step and is bounded below by 0
__device__ __forceinline__ int cc_find(int* parent, int i) {
    int cur = cc_ld(parent + i);
    if (cur != i) {
        int prev = i, next;
        while (cur > (next = cc_ld(parent + cur))) {
            cc_st(parent + prev, next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// hook the two trees together: the larger root onto the smaller, only while it still is a root (compare-and-swap).
// Terminates: a successful compare-and-swap ends the loop (it lowered the larger root strictly); a failed one returns the value
// that replaced the root, which is strictly smaller than it, so max(ra, rb) strictly decreases and is bounded below by 0
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    int ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        if (ra < rb) {
            const int old = atomicCAS(parent + rb, rb, ra);
            if (old == rb) break;
            rb = old;
        } else {
            const int old = atomicCAS(parent + ra, ra, rb);
            if (old == ra) break;
            ra = old;
        }
    }
}

// count[root] += the component's voxels, over a flattened parent (root or -1 per voxel): a thread folds its CC_RUN consecutive
// voxels into runs of one root (a run that ends inside adds at once), and the lanes whose last runs share a root add them with one
// atomic.  T threads per block; the whole block must call it (the ballots span all 64 lanes)
template <int T>
__device__ __forceinline__ void cc_count_runs(int S, const int* __restrict__ parent, unsigned* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    // block-uniform trip count
    for (int64_t base = (int64_t)blockIdx.x * T * CC_RUN; base < S; base += (int64_t)gridDim.x * T * CC_RUN) {
        const int64_t v0 = base + (int64_t)threadIdx.x * CC_RUN;
        int r[CC_RUN];
        if (v0 + CC_RUN <= S) {   // parent is 256-B aligned and v0 a multiple of 16: four 16-B loads
#pragma unroll
            for (int q = 0; q < CC_RUN / 4; ++q) {
                const int4 t = *(const int4*)(parent + v0 + 4 * q);
                r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < CC_RUN; ++k) r[k] = v0 + k < S ? parent[v0 + k] : -1;
        }
        int cur = -1;
        unsigned n = 0;
#pragma unroll
        for (int k = 0; k < CC_RUN; ++k) {
            if (r[k] != cur) {
                if (n) atomicAdd(count + cur, n);
                cur = r[k];
                n = 0;
            }
            n += r[k] >= 0 ? 1u : 0u;
        }
        const int key = n ? cur : -1;
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {   // wave-uniform: one add per distinct root of the wave
            const int leader = __ffsll((long long)todo) - 1;
            const int lk = __shfl(key, leader);
            const unsigned long long same = __ballot(key == lk);
            unsigned t = key == lk ? n : 0u;
            if (__popcll(same) > 1)
                for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == leader) atomicAdd(count + lk, t);
            todo &= ~same;
        }
    }
}

}  // namespace unet
