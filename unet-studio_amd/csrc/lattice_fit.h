// The fit of a lattice warp, once for the two of them (kernels_warp.hip, kernels_cowarp.hip): the colour passes of a sweep under
// both implementations, the scratch, a sweep's launches and the schedule of a fit, over lattice_field.h's arithmetic.  A file
// states what differs in a metric M, a plain struct handed to the kernels by value:
//   G                       the two grids: sw, sh, sd the one the lattice lies over, tw, th, td the one that is sampled
//   M(G, scratch)           what of the scratch the kernels read (cowarp: W)
//   COUNTERS                7: the seven sums, every voxel counts and a node with a support is visited; 8: a voxel can be "none",
//                           the eighth sum counts the voxels that are not, and a node without one is not visited
//   stage<NT>()             a block's own table in LDS (cowarp: W; warp: nothing), before the caller's barrier
//   fixed(v, a)             whether voxel v of the lattice's grid counts, and its class or code a
//   seven(a, ..., tab, mask)  warp_seven with the metric's read and value
//   NAME, HIST_BYTES, EXTRA_BYTES   the prefix of an error, and the histogram's and the metric's own part of the scratch
//   before_sweep(...)       what a sweep enqueues in front of its colour passes (cowarp: the histogram and W)
//   row(...)                the histogram after the sweeps of a (level, step) and its report row (lat_row is the row's tail)
//
//   k_lattice_node    IMPL_NODE, one colour pass: a block of NT threads (64 = one wave for g = 4, 256 for g = 8, 1024 above) per node
//                     of the colour.  The node's 3x3x3 neighbourhood of D is staged in LDS (81 ints, read at addresses that differ
//                     only with the voxel's octant: mostly broadcasts) beside the metric's table, the six moved candidates'
//                     admissibility is a block-uniform mask, every thread strides over the support with COUNTERS int32 sums in
//                     registers (a candidate whose nearest sample is the unmoved one's reuses it: no second gather), the sums are
//                     reduced by lane shuffles, then across waves through LDS, and thread 0 chooses and writes the node
//   k_lattice_vox     IMPL_VOXEL, one colour pass: a thread per voxel finds the one node of the colour whose support holds it and adds
//                     its contributions into that node's COUNTERS counters in the scratch (int atomics)
//   k_lattice_pick    IMPL_VOXEL: a thread per node of the colour: admissibility, the choice, the node, and the counters zeroed again
// Every atomic is an integer add: the results do not depend on the schedule.  In a fit every sweep's kernels return at once when
// `prev`, the count of nodes the preceding sweep of the same (level, step) changed, is zero (stream order makes it final): the host
// reads nothing back.
//
// Scratch, each part 256-B aligned: the sweeps' {changed, visited} slots, a histogram, the metric's own part, the counters of
// IMPL_VOXEL (COUNTERS per node of the finest lattice), the fields of all levels but the last.
#pragma once
#include <stdexcept>
#include <string>

#include "kernels.h"
#include "lattice_field.h"

namespace unet {

constexpr int LAT_T = 256;         // threads per block of the per-voxel and per-node-thread kernels
constexpr int LAT_MAXB = 8192;     // their grid cap; they stride over the rest
constexpr int LAT_IMPL_VOXEL = 2, LAT_MAX_LEVELS = 4, LAT_MAX_SWEEPS = 16, LAT_MAX_ROWS = 32;   // the files that include this assert them
constexpr int LAT_SLOTS = LAT_MAX_ROWS * LAT_MAX_SWEEPS;
typedef unsigned long long u64;

// ---- a colour pass, a block per node ---------------------------------------------------------------------------------------------
template <class M, int NT>
__global__ void __launch_bounds__(NT) k_lattice_node(M m, WarpMap map, int32_t* D, WarpLat L, int colour, int step, int limit, u64* info,
                                                     const u64* prev) {
    constexpr int C = M::COUNTERS;
    __shared__ float lm[12];
    __shared__ int ld[27 * 3];          // the 3x3x3 neighbourhood, x fastest then component; a node that does not exist holds 0
    __shared__ unsigned ladm;
    __shared__ int lsum[(NT / 64) * C];
    if (prev && *prev == 0ull) return;  // uniform: the preceding sweep is complete (stream order) and changed nothing
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u;
    const int i = cx + 2 * (int)(blockIdx.x % mx), j = cy + 2 * (int)((blockIdx.x / mx) % my), k = cz + 2 * (int)(blockIdx.x / (mx * my));
    int x0, x1, y0, y1, z0, z1;
    warp_support(i, L.g, m.G.sw, x0, x1);
    warp_support(j, L.g, m.G.sh, y0, y1);
    warp_support(k, L.g, m.G.sd, z0, z1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return;   // uniform: an empty support, the node stays
    const int tid = threadIdx.x;
    warp_stage<NT>(D, L, i, j, k, ld);
    const auto tab = m.template stage<NT>();
    if (tid < 12) lm[tid] = map.v[tid];
    if (tid == 0) ladm = 1u;
    __syncthreads();
    if (tid < 6 && warp_staged_admissible(ld, L, i, j, k, tid + 1, step, limit)) atomicOr(&ladm, 2u << tid);
    __syncthreads();
    const unsigned mask = ladm;
    const int g = L.g, ex = x1 - x0 + 1, ey = y1 - y0 + 1, n = ex * ey * (z1 - z0 + 1);   // <= (2 g - 1)^3
    int acc[C] = {};   // the seven sums, and under 8 the voxels that count
    for (int v = tid; v < n; v += NT) {
        const int x = x0 + v % ex, y = y0 + (v / ex) % ey, z = z0 + v / (ex * ey);
        const int64_t at = ((int64_t)z * m.G.sh + y) * m.G.sw + x;
        unsigned a;
        if constexpr (C == 8)   // a voxel can be "none": found out before anything is computed for it
            if (!m.fixed(at, a)) continue;
        int n0, n1, n2;
        const int ws = warp_staged_corners(ld, g, x, y, z, i, j, k, n0, n1, n2) * step;   // <= g^3 * 32767
        if constexpr (C == 7) m.fixed(at, a);   // every voxel counts: read beside its use, which costs fewer registers
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        const WarpVotes r = m.seven(a, px, py, pz, n0, n1, n2, ws, L.scale, tab, mask);
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[c] += r.v[c];
        if constexpr (C == 8) ++acc[7];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int s = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) lsum[(tid >> 6) * C + c] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int score[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            score[c] = 0;
            for (int w = 0; w < NT / 64; ++w) score[c] += lsum[w * C + c];
        }
        if constexpr (C == 8)
            if (score[7] == 0) return;   // no voxel that counts: not visited
        const int best = warp_best(score, mask);
        if (best) {
            const int axis = (best - 1) >> 1;
            D[(((size_t)k * L.ny + j) * L.nx + i) * 3 + axis] = ld[39 + axis] + ((best & 1) ? step : -step);
            atomicAdd(info, 1ull);
        }
        atomicAdd(info + 1, 1ull);
    }
}

// ---- a colour pass, a thread per voxel -------------------------------------------------------------------------------------------
template <class M>
__global__ void __launch_bounds__(LAT_T) k_lattice_vox(M m, WarpMap map, const int32_t* __restrict__ D, WarpLat L, int colour, int step,
                                                       int* __restrict__ cnt, const u64* prev) {
    constexpr int C = M::COUNTERS;
    __shared__ float lm[12];
    if (prev && *prev == 0ull) return;
    const auto tab = m.template stage<LAT_T>();
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = m.G.sw * m.G.sh * m.G.sd, g = L.g;
    for (int64_t i64 = (int64_t)blockIdx.x * LAT_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * LAT_T) {
        const int v = (int)i64, x = v % m.G.sw, y = (v / m.G.sw) % m.G.sh, z = v / (m.G.sw * m.G.sh);
        const int i = warp_owner(x, L.lg, g, colour & 1), j = warp_owner(y, L.lg, g, (colour >> 1) & 1), k = warp_owner(z, L.lg, g, colour >> 2);
        if (i < 0 || j < 0 || k < 0) continue;
        unsigned a;
        if constexpr (C == 8)   // as in the node pass
            if (!m.fixed(v, a)) continue;
        int n0, n1, n2;
        warp_corners(D, L, x, y, z, n0, n1, n2);
        const int ws = (g - abs(x - i * g)) * (g - abs(y - j * g)) * (g - abs(z - k * g)) * step;
        if constexpr (C == 7) m.fixed(v, a);
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        // every candidate, admissible or not (the pick kernel knows): |n +- ws| <= 2 g^3 * 32767 < 2^31
        const WarpVotes r = m.seven(a, px, py, pz, n0, n1, n2, ws, L.scale, tab, 0x7Fu);
        int* cn = cnt + (((size_t)k * L.ny + j) * L.nx + i) * C;
#pragma unroll
        for (int c = 0; c < 7; ++c)
            if (r.v[c]) atomicAdd(cn + c, r.v[c]);
        if constexpr (C == 8) atomicAdd(cn + 7, 1);
    }
}

template <class M>
__global__ void __launch_bounds__(LAT_T) k_lattice_pick(int sw, int sh, int sd, int32_t* D, WarpLat L, int colour, int step, int limit,
                                                        int* __restrict__ cnt, u64* info, const u64* prev) {
    constexpr int C = M::COUNTERS;
    if (prev && *prev == 0ull) return;
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u, mz = (unsigned)(L.nz - cz + 1) / 2u;
    const int64_t nodes = (int64_t)mx * my * mz;
    for (int64_t b = (int64_t)blockIdx.x * LAT_T + threadIdx.x; b < nodes; b += (int64_t)gridDim.x * LAT_T) {
        const int i = cx + 2 * (int)(b % mx), j = cy + 2 * (int)((b / mx) % my), k = cz + 2 * (int)(b / ((int64_t)mx * my));
        const size_t node = ((size_t)k * L.ny + j) * L.nx + i;
        // no voxel added anything, the counters are still zero: under 8 no voxel that counts, under 7 an empty support
        if constexpr (C == 8) {
            if (cnt[node * 8 + 7] == 0) continue;
        } else {
            int x0, x1, y0, y1, z0, z1;
            warp_support(i, L.g, sw, x0, x1);
            warp_support(j, L.g, sh, y0, y1);
            warp_support(k, L.g, sd, z0, z1);
            if (x0 > x1 || y0 > y1 || z0 > z1) continue;
        }
        int32_t* d = D + node * 3;
        const int d0 = d[0], d1 = d[1], d2 = d[2];
        const unsigned mask = warp_pick_mask(D, L, i, j, k, d0, d1, d2, step, limit);
        int score[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            score[c] = cnt[node * C + c];
            cnt[node * C + c] = 0;
        }
        if constexpr (C == 8) cnt[node * 8 + 7] = 0;
        const int best = warp_best(score, mask);
        if (best) {
            const int axis = (best - 1) >> 1, delta = (best & 1) ? step : -step;
            d[axis] = (axis == 0 ? d0 : axis == 1 ? d1 : d2) + delta;
            atomicAdd(info, 1ull);
        }
        atomicAdd(info + 1, 1ull);
    }
}

// a report row but its score.  slots: the max_sweeps {changed, visited} pairs of this (level, step); sweep s ran when s == 0 or
// sweep s - 1 changed a node
__device__ __forceinline__ void lat_row(const u64* __restrict__ slots, int max_sweeps, int g, int step, int64_t* __restrict__ row) {
    int ran = 1;
    while (ran < max_sweeps && slots[2 * (ran - 1)]) ++ran;
    row[0] = g;
    row[1] = step;
    row[2] = ran;
    row[3] = (int64_t)slots[2 * (ran - 1)];
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
inline void lat_memset(const char* who, void* p, int value, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, value, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string(who) + ": hipMemsetAsync: " + hipGetErrorString(e));
}
inline int lat_blocks(int64_t items) {
    const int64_t nb = (items + LAT_T - 1) / LAT_T;
    return (int)(nb > LAT_MAXB ? LAT_MAXB : nb < 1 ? 1 : nb);
}

struct LatScratch {
    u64* slots;        // LAT_SLOTS x {changed, visited}
    uint32_t* hist;    // M::HIST_BYTES
    void* extra;       // M::EXTRA_BYTES
    int* cnt;          // M::COUNTERS per node of the finest lattice
    int32_t* field[LAT_MAX_LEVELS];   // the levels but the last
    size_t bytes;      // from the aligned base
};
template <class M> LatScratch lat_scratch(void* scratch, int sw, int sh, int sd, const int* levels, int n_levels) {
    char* b = (char*)warp_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    LatScratch s = {};
    size_t o = 0;
    s.slots = (u64*)(b + o);     o += warp_align((size_t)LAT_SLOTS * 2 * sizeof(u64));
    s.hist = (uint32_t*)(b + o); o += warp_align(M::HIST_BYTES);
    s.extra = b + o;             o += warp_align(M::EXTRA_BYTES);
    s.cnt = (int*)(b + o);       o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[5 * (n_levels - 1)])) * M::COUNTERS * sizeof(int));
    for (int l = 0; l + 1 < n_levels; ++l) {
        s.field[l] = (int32_t*)(b + o);
        o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[5 * l])) * 3 * sizeof(int32_t));
    }
    s.bytes = o;
    return s;
}
template <class M> size_t lat_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels) {
    return 256 + lat_scratch<M>(nullptr, sw, sh, sd, levels, n_levels).bytes;
}
template <class M> void lat_zero_counters(const LatScratch& sc, const WarpLat& finest, hipStream_t s) {
    lat_memset(M::NAME, sc.cnt, 0, warp_nodes(finest) * M::COUNTERS * sizeof(int), s);
}

// one sweep: what the metric puts in front, then the 8 colour passes.  sc.cnt: zero on entry under IMPL_VOXEL, and left zero
template <class M>
void lat_sweep_into(const M& m, const WarpMap& map, int32_t* D, const WarpLat& L, int step, int limit, u64* info, const u64* prev, int impl,
                    const LatScratch& sc, hipStream_t s) {
    m.before_sweep(map, D, L, sc, prev, s);
    for (int c = 0; c < 8; ++c) {
        const int64_t nodes = (int64_t)((L.nx - (c & 1) + 1) / 2) * ((L.ny - ((c >> 1) & 1) + 1) / 2) * ((L.nz - (c >> 2) + 1) / 2);
        if (impl == LAT_IMPL_VOXEL) {
            k_lattice_vox<M><<<lat_blocks((int64_t)m.G.sw * m.G.sh * m.G.sd), LAT_T, 0, s>>>(m, map, D, L, c, step, sc.cnt, prev);
            k_lattice_pick<M><<<lat_blocks(nodes), LAT_T, 0, s>>>(m.G.sw, m.G.sh, m.G.sd, D, L, c, step, limit, sc.cnt, info, prev);
            continue;
        }
        // DEFAULT: NODE
        if (L.g == 4) k_lattice_node<M, 64><<<(unsigned)nodes, 64, 0, s>>>(m, map, D, L, c, step, limit, info, prev);
        else if (L.g == 8) k_lattice_node<M, 256><<<(unsigned)nodes, 256, 0, s>>>(m, map, D, L, c, step, limit, info, prev);
        else k_lattice_node<M, 1024><<<(unsigned)nodes, 1024, 0, s>>>(m, map, D, L, c, step, limit, info, prev);
    }
}

// launch_*_sweep: one sweep of D in place, info = {changed, visited}
template <class M>
void lat_sweep(const typename M::Grids& G, const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch,
               hipStream_t s) {
    const int level[5] = {g, step, step, 1, limit};
    const LatScratch sc = lat_scratch<M>(scratch, G.sw, G.sh, G.sd, level, 1);
    const WarpLat L = warp_lattice(G.sw, G.sh, G.sd, g);
    lat_memset(M::NAME, info, 0, 2 * sizeof(int64_t), s);
    if (impl == LAT_IMPL_VOXEL) lat_zero_counters<M>(sc, L, s);
    lat_sweep_into(M(G, sc), warp_map(map), D, L, step, limit, (u64*)info, nullptr, impl, sc, s);
}

// launch_*_fit: the field from zero through every level, a report row per (level, step)
template <class M>
void lat_fit(const typename M::Grids& G, const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl,
             void* scratch, hipStream_t s) {
    const LatScratch sc = lat_scratch<M>(scratch, G.sw, G.sh, G.sd, levels, n_levels);
    const M m(G, sc);
    const WarpMap mp = warp_map(map);
    lat_memset(M::NAME, report, 0xFF, (size_t)LAT_MAX_ROWS * 5 * sizeof(int64_t), s);   // -1 in every row
    lat_memset(M::NAME, sc.slots, 0, (size_t)LAT_SLOTS * 2 * sizeof(u64), s);
    if (impl == LAT_IMPL_VOXEL) lat_zero_counters<M>(sc, warp_lattice(G.sw, G.sh, G.sd, levels[5 * (n_levels - 1)]), s);
    int row = 0, slot = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* lv = levels + 5 * l;
        const WarpLat L = warp_lattice(G.sw, G.sh, G.sd, lv[0]);
        int32_t* D = l + 1 < n_levels ? sc.field[l] : D_out;
        if (l == 0) lat_memset(M::NAME, D, 0, warp_nodes(L) * 3 * sizeof(int32_t), s);
        for (int step = lv[1]; step >= lv[2]; step >>= 1, ++row) {
            const int first = slot;
            for (int k = 0; k < lv[3]; ++k, ++slot)
                lat_sweep_into(m, mp, D, L, step, lv[4], sc.slots + 2 * slot, k ? sc.slots + 2 * (slot - 1) : nullptr, impl, sc, s);
            m.row(mp, D, L, sc, sc.slots + 2 * first, lv[3], step, report + 5 * row, s);
        }
        if (l + 1 < n_levels) launch_warp_refine(D, G.sw, G.sh, G.sd, lv[0], l + 2 < n_levels ? sc.field[l + 1] : D_out, s);
    }
}

}  // namespace unet
