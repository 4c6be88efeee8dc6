// What the two lattice warps share (kernels_warp.hip: tissue maps, include/unet_warp.h; kernels_cowarp.hip: intensity codes,
// include/unet_cowarp.h): the lattice over a grid, the warped position of a voxel under a 12-float map and a Q8 displacement field,
// and a node's support, admissibility and choice.  Only what a voxel's sample adds to a node's seven sums differs between the two.
// This is the arithmetic, all inlined device code; the kernels of a sweep and the schedule of a fit built on it are lattice_fit.h's,
// and the histogram, row, refine, carry and resample kernels of the two files call it directly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "affine_search.h"

namespace unet {

constexpr int WARP_MAX_DISP = 32767;   // UNET_WARP_MAX_DISP and UNET_COWARP_MAX_DISP (the files that include this assert it)

struct WarpMap {
    float v[12];
};
struct WarpLat {   // a lattice over the subject grid
    int nx, ny, nz, g, lg;
    float scale;   // 2^-(8 + 3 lg)
};

inline int warp_log2(int g) { return g == 4 ? 2 : g == 8 ? 3 : g == 16 ? 4 : 5; }
inline WarpLat warp_lattice(int sw, int sh, int sd, int g) {
    WarpLat L;
    L.g = g;
    L.lg = warp_log2(g);
    L.nx = (sw + g - 1) / g + 1;
    L.ny = (sh + g - 1) / g + 1;
    L.nz = (sd + g - 1) / g + 1;
    L.scale = ldexpf(1.f, -(8 + 3 * L.lg));
    return L;
}
inline size_t warp_nodes(const WarpLat& L) { return (size_t)L.nx * L.ny * L.nz; }
inline size_t warp_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline WarpMap warp_map(const float* map) {
    WarpMap m;
    for (int e = 0; e < 12; ++e) m.v[e] = map[e];
    return m;
}

// n_r of voxel (x, y, z): the cell's 8 corners weighted; a corner of weight 0 is not read
__device__ __forceinline__ void warp_corners(const int32_t* __restrict__ D, const WarpLat& L, int x, int y, int z, int& n0, int& n1, int& n2) {
    const int g = L.g, m = g - 1, cx = x >> L.lg, cy = y >> L.lg, cz = z >> L.lg, fx = x & m, fy = y & m, fz = z & m;
    n0 = n1 = n2 = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int w = ((c & 1) ? fx : g - fx) * ((c & 2) ? fy : g - fy) * ((c & 4) ? fz : g - fz);
        if (w) {
            const int32_t* d = D + (((size_t)(cz + (c >> 2)) * L.ny + (cy + ((c >> 1) & 1))) * L.nx + (cx + (c & 1))) * 3;
            n0 += w * d[0];
            n1 += w * d[1];
            n2 += w * d[2];
        }
    }
}

// the affine position of a voxel, before the displacement and the half: fp32, left to right, no fused multiply-add
__device__ __forceinline__ void warp_affine(const float* m, int xi, int yi, int zi, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    const float x = (float)xi, y = (float)yi, z = (float)zi;
    px = ((m[0] * x + m[1] * y) + m[2] * z) + m[9];
    py = ((m[3] * x + m[4] * y) + m[5] * z) + m[10];
    pz = ((m[6] * x + m[7] * y) + m[8] * z) + m[11];
}
// p' = p + n * 2^-(8 + 3 lg) along one axis; the scaling by a power of two is exact
__device__ __forceinline__ float warp_p(float p, int n, float scale) {
#pragma clang fp contract(off)
    const float d = (float)n * scale;
    return p + d;
}
// q = p' + 0.5
__device__ __forceinline__ float warp_q(float p, int n, float scale) {
#pragma clang fp contract(off)
    const float w = warp_p(p, n, scale);
    return w + 0.5f;
}
__device__ __forceinline__ AffPos warp_pos(float qx, float qy, float qz, int tw, int th, int td) {
    AffPos p;
    p.qx = qx; p.qy = qy; p.qz = qz;
    p.in = qx >= 0.f && qy >= 0.f && qz >= 0.f && qx < (float)tw && qy < (float)th && qz < (float)td;
    return p;
}
__device__ __forceinline__ AffPos warp_locate(const float* m, const int32_t* __restrict__ D, const WarpLat& L, int x, int y, int z, int tw, int th,
                                              int td) {
    float px, py, pz;
    int n0, n1, n2;
    warp_affine(m, x, y, z, px, py, pz);
    warp_corners(D, L, x, y, z, n0, n1, n2);
    return warp_pos(warp_q(px, n0, L.scale), warp_q(py, n1, L.scale), warp_q(pz, n2, L.scale), tw, th, td);
}
// the template index of a position, -1 outside
__device__ __forceinline__ int warp_offset(float qx, float qy, float qz, int tw, int th, int td) {
    const AffPos p = warp_pos(qx, qy, qz, tw, th, td);
    return p.in ? ((int)floorf(qz) * th + (int)floorf(qy)) * tw + (int)floorf(qx) : -1;
}

// The seven values of one voxel: p its affine position, n its corner sums with the node unmoved, ws what one step of the node adds
// to a sum.  read(o) -> the template sample at index o (-1: outside); value(b) -> what a sample b is worth to this voxel.  mask: bit
// c set = candidate c wanted (bit 0 always); the others give 0.  A moved candidate whose nearest template voxel is the unmoved one's
// reuses its sample: no second gather
struct WarpVotes {
    int v[7];
};
template <typename Read, typename Value>
__device__ __forceinline__ WarpVotes warp_seven(float px, float py, float pz, int n0, int n1, int n2, int ws, float scale, int tw, int th, int td,
                                                unsigned mask, Read read, Value value) {
    const float q0 = warp_q(px, n0, scale), q1 = warp_q(py, n1, scale), q2 = warp_q(pz, n2, scale);
    const int ob = warp_offset(q0, q1, q2, tw, th, td);
    const unsigned bb = read(ob);
    WarpVotes r;
    r.v[0] = value(bb);
    auto moved = [&](int c, float qx, float qy, float qz) {
        if (!((mask >> c) & 1u)) return 0;
        const int o = warp_offset(qx, qy, qz, tw, th, td);
        return value(o == ob ? bb : read(o));
    };
    r.v[1] = moved(1, warp_q(px, n0 + ws, scale), q1, q2);
    r.v[2] = moved(2, warp_q(px, n0 - ws, scale), q1, q2);
    r.v[3] = moved(3, q0, warp_q(py, n1 + ws, scale), q2);
    r.v[4] = moved(4, q0, warp_q(py, n1 - ws, scale), q2);
    r.v[5] = moved(5, q0, q1, warp_q(pz, n2 + ws, scale));
    r.v[6] = moved(6, q0, q1, warp_q(pz, n2 - ws, scale));
    return r;
}

// Is moved candidate c (1..6) of a node at (d0, d1, d2) admissible?  nb(n, v0, v1, v2) -> whether lattice neighbour n (-x, +x, -y,
// +y, -z, +z) exists, and its field
template <typename Nb> __device__ __forceinline__ bool warp_admissible(int d0, int d1, int d2, int c, int step, int limit, Nb nb) {
    const int axis = (c - 1) >> 1, delta = (c & 1) ? step : -step;
    const int c0 = d0 + (axis == 0 ? delta : 0), c1 = d1 + (axis == 1 ? delta : 0), c2 = d2 + (axis == 2 ? delta : 0);
    const int moved = axis == 0 ? c0 : axis == 1 ? c1 : c2;
    bool ok = moved <= WARP_MAX_DISP && moved >= -WARP_MAX_DISP;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        int v0, v1, v2;
        if (nb(n, v0, v1, v2)) ok = ok && abs(c0 - v0) <= limit && abs(c1 - v1) <= limit && abs(c2 - v2) <= limit;
    }
    return ok;
}
// the winner of seven local scores under a mask of admissible candidates: the best, the lowest index among equals
__device__ __forceinline__ int warp_best(const int* score, unsigned mask) {
    int best = 0, top = score[0];
#pragma unroll
    for (int c = 1; c < 7; ++c)
        if (((mask >> c) & 1u) && score[c] > top) { best = c; top = score[c]; }
    return best;
}
// the support of a node along one axis of `dim` voxels: [lo, hi], empty when lo > hi
__device__ __forceinline__ void warp_support(int i, int g, int dim, int& lo, int& hi) {
    lo = max(0, (i - 1) * g + 1);
    hi = min(dim - 1, (i + 1) * g - 1);
}
// the node of parity `par` whose support holds coordinate x, -1 for none
__device__ __forceinline__ int warp_owner(int x, int lg, int g, int par) {
    const int cell = x >> lg;
    if ((x & (g - 1)) == 0) return (cell & 1) == par ? cell : -1;
    return (cell & 1) == par ? cell : cell + 1;
}

// IMPL_NODE: thread e < 81 of NT stages component e % 3 of the node's 3x3x3 neighbourhood (x fastest then component; a node that does
// not exist holds 0) into ld; the caller's barrier follows
template <int NT> __device__ __forceinline__ void warp_stage(const int32_t* D, const WarpLat& L, int i, int j, int k, int* ld) {
    for (int e = threadIdx.x; e < 81; e += NT) {
        const int nb = e / 3, ii = i + nb % 3 - 1, jj = j + (nb / 3) % 3 - 1, kk = k + nb / 9 - 1;
        const bool ok = ii >= 0 && ii < L.nx && jj >= 0 && jj < L.ny && kk >= 0 && kk < L.nz;
        ld[e] = ok ? D[(((size_t)kk * L.ny + jj) * L.nx + ii) * 3 + e % 3] : 0;
    }
}
// IMPL_NODE, thread c - 1 < 6: is moved candidate c of the staged node admissible?
__device__ __forceinline__ bool warp_staged_admissible(const int* ld, const WarpLat& L, int i, int j, int k, int c, int step, int limit) {
    auto nb = [&](int n, int& v0, int& v1, int& v2) {
        const int a = n >> 1, s = (n & 1) ? 1 : -1, ii = i + (a == 0 ? s : 0), jj = j + (a == 1 ? s : 0), kk = k + (a == 2 ? s : 0);
        const int* v = ld + (((kk - k + 1) * 3 + (jj - j + 1)) * 3 + (ii - i + 1)) * 3;
        v0 = v[0]; v1 = v[1]; v2 = v[2];
        return ii >= 0 && ii < L.nx && jj >= 0 && jj < L.ny && kk >= 0 && kk < L.nz;
    };
    return warp_admissible(ld[39], ld[40], ld[41], c, step, limit, nb);
}
// IMPL_NODE: the corner sums of support voxel (x, y, z) of the staged node (i, j, k) with the node unmoved, and ws / step
__device__ __forceinline__ int warp_staged_corners(const int* ld, int g, int x, int y, int z, int i, int j, int k, int& n0, int& n1, int& n2) {
    const int dx = x - i * g, dy = y - j * g, dz = z - k * g;
    // the voxel's cell inside the neighbourhood: its lower corner is the node itself (1) or the one before it (0)
    const int bx = dx >= 0 ? 1 : 0, by = dy >= 0 ? 1 : 0, bz = dz >= 0 ? 1 : 0;
    const int fx = dx >= 0 ? dx : g + dx, fy = dy >= 0 ? dy : g + dy, fz = dz >= 0 ? dz : g + dz;
    n0 = n1 = n2 = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int w = ((c & 1) ? fx : g - fx) * ((c & 2) ? fy : g - fy) * ((c & 4) ? fz : g - fz);
        const int* d = ld + (((bz + (c >> 2)) * 3 + (by + ((c >> 1) & 1))) * 3 + (bx + (c & 1))) * 3;
        n0 += w * d[0];
        n1 += w * d[1];
        n2 += w * d[2];
    }
    return (g - abs(dx)) * (g - abs(dy)) * (g - abs(dz));
}
// IMPL_VOXEL's pick: the mask of admissible candidates of node (i, j, k) at (d0, d1, d2), its neighbours read from D (another
// colour: not written in this pass)
__device__ __forceinline__ unsigned warp_pick_mask(const int32_t* D, const WarpLat& L, int i, int j, int k, int d0, int d1, int d2, int step,
                                                   int limit) {
    auto nb = [&](int n, int& v0, int& v1, int& v2) {
        const int a = n >> 1, s = (n & 1) ? 1 : -1, ii = i + (a == 0 ? s : 0), jj = j + (a == 1 ? s : 0), kk = k + (a == 2 ? s : 0);
        const bool ok = ii >= 0 && ii < L.nx && jj >= 0 && jj < L.ny && kk >= 0 && kk < L.nz;
        v0 = v1 = v2 = 0;
        if (ok) {
            const int32_t* v = D + (((size_t)kk * L.ny + jj) * L.nx + ii) * 3;
            v0 = v[0]; v1 = v[1]; v2 = v[2];
        }
        return ok;
    };
    unsigned mask = 1u;
#pragma unroll
    for (int c = 1; c < 7; ++c)
        if (warp_admissible(d0, d1, d2, c, step, limit, nb)) mask |= 1u << c;
    return mask;
}

}  // namespace unet
