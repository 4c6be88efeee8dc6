// The non-linear refinement of a parcellation (include/unet_warp.h): a Q8 displacement field on a lattice of spacing g, moved node by
// node towards a better tissue agreement, and the carrying of an atlas through the warped map.
//
//   k_warp_hist    grid-stride over the subject's voxels: the warped position, the nearest template tissue, the block's T*T counters
//                  in LDS, one global add per non-zero counter
//   k_warp_node    IMPL_NODE, one colour pass: a block of NT threads (64 = one wave for g = 4, 256 for g = 8, 1024 above) per node
//                  of the colour.  The node's 3x3x3 neighbourhood of D is staged in LDS (81 ints, read at addresses that differ
//                  only with the voxel's octant: mostly broadcasts), the six moved candidates' admissibility is a block-uniform
//                  mask, every thread strides over the support with seven int32 sums in registers (a candidate whose nearest
//                  template voxel is the unmoved one's reuses its tissue: no second gather), the sums are reduced by lane
//                  shuffles, then across waves through LDS, and thread 0 chooses and writes the node
//   k_warp_vox     IMPL_VOXEL, one colour pass: a thread per voxel finds the one node of the colour whose support holds it and adds
//                  its seven contributions into that node's counters in the scratch (int atomics)
//   k_warp_pick    IMPL_VOXEL: a thread per node of the colour: admissibility, the choice, the node, and the counters zeroed again
//   k_warp_refine  a thread per fine node
//   k_warp_row     one thread: a (level, step)'s report row from the sweeps' counts and the histogram after them
//   k_warp_carry   one thread per subject voxel: kernels_register.hip's carry at the warped position (tissue_carry.h)
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off.  In a fit every sweep's kernels return at once when `prev`, the count of nodes the preceding
// sweep of the same (level, step) changed, is zero (stream order makes it final): the host reads nothing back.  The lattice, the
// positions, a node's support, admissibility and choice are the one copy of lattice_field.h, shared with kernels_cowarp.hip.
//
// Scratch, each part 256-B aligned: the sweeps' {changed, visited} slots, a histogram, the counters of IMPL_VOXEL (7 per node of the
// finest lattice), the fields of all levels but the last.
#include <stdexcept>
#include <string>

#include "../../include/unet_warp.h"
#include "affine_search.h"
#include "device_util.h"
#include "lattice_field.h"
#include "tissue_carry.h"

namespace unet {

namespace {

constexpr int WARP_T = 256;                  // threads per block of the per-voxel and per-node-thread kernels
constexpr int WARP_MAXB = 8192;              // their grid cap; they stride over the rest
constexpr int WARP_MAXT = UNET_WARP_MAX_TISSUES;
constexpr int WARP_SLOTS = UNET_WARP_MAX_ROWS * UNET_WARP_MAX_SWEEPS;
typedef unsigned long long u64;
static_assert(WARP_MAX_DISP == UNET_WARP_MAX_DISP, "lattice_field.h's range is this header's");

struct Scratch {
    u64* slots;        // WARP_SLOTS x {changed, visited}
    uint32_t* hist;    // WARP_MAXT^2
    int* cnt;          // 7 per node of the finest lattice
    int32_t* field[UNET_WARP_MAX_LEVELS];   // the levels but the last
    size_t bytes;      // from the aligned base
};
Scratch warp_scratch(void* scratch, int sw, int sh, int sd, const int* levels, int n_levels) {
    char* b = (char*)warp_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s = {};
    size_t o = 0;
    s.slots = (u64*)(b + o);     o += warp_align((size_t)WARP_SLOTS * 2 * sizeof(u64));
    s.hist = (uint32_t*)(b + o); o += warp_align((size_t)WARP_MAXT * WARP_MAXT * 4);
    s.cnt = (int*)(b + o);       o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[5 * (n_levels - 1)])) * 7 * sizeof(int));
    for (int l = 0; l + 1 < n_levels; ++l) {
        s.field[l] = (int32_t*)(b + o);
        o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[5 * l])) * 3 * sizeof(int32_t));
    }
    s.bytes = o;
    return s;
}

// what a voxel of subject tissue a adds to agree - disagree when its template sample reads b
__device__ __forceinline__ int warp_vote(unsigned a, unsigned b) { return a == b ? (a ? 1 : 0) : -1; }

// The seven votes of one voxel of subject tissue a (lattice_field.h's warp_seven): an outside sample reads tissue 0
__device__ __forceinline__ WarpVotes warp_votes(unsigned a, float px, float py, float pz, int n0, int n1, int n2, int ws, float scale,
                                                const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T, unsigned mask) {
    return warp_seven(px, py, pz, n0, n1, n2, ws, scale, tw, th, td, mask,
                      [&](int o) { return o < 0 ? 0u : reg_tissue(tmpl, tbytes, o, T); }, [&](unsigned b) { return warp_vote(a, b); });
}

// ---- the joint histogram ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WARP_T) k_warp_hist(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                      const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T, WarpMap map,
                                                      const int32_t* __restrict__ D, WarpLat L, uint32_t* __restrict__ hist) {
    __shared__ unsigned lh[WARP_MAXT * WARP_MAXT];
    __shared__ float lm[12];
    for (int e = threadIdx.x; e < T * T; e += WARP_T) lh[e] = 0u;
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = sw * sh * sd;
    for (int64_t i64 = (int64_t)blockIdx.x * WARP_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * WARP_T) {
        const int i = (int)i64, x = i % sw, y = (i / sw) % sh, z = i / (sw * sh);
        const unsigned a = reg_tissue(subject, sbytes, i, T);
        const AffPos p = warp_locate(lm, D, L, x, y, z, tw, th, td);
        unsigned b = 0u;
        if (p.in) b = reg_tissue(tmpl, tbytes, ((int64_t)(int)floorf(p.qz) * th + (int)floorf(p.qy)) * tw + (int)floorf(p.qx), T);
        atomicAdd(&lh[a * (unsigned)T + b], 1u);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * T; e += WARP_T)
        if (const unsigned c = lh[e]) atomicAdd(hist + e, c);
}

// ---- a colour pass, a block per node ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) k_warp_node(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                  const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T, WarpMap map,
                                                  int32_t* D, WarpLat L, int colour, int step, int limit, u64* info, const u64* prev) {
    __shared__ float lm[12];
    __shared__ int ld[27 * 3];          // the 3x3x3 neighbourhood, x fastest then component; a node that does not exist holds 0
    __shared__ unsigned ladm;
    __shared__ int lsum[(NT / 64) * 7];
    if (prev && *prev == 0ull) return;  // uniform: the preceding sweep is complete (stream order) and changed nothing
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u;
    const int i = cx + 2 * (int)(blockIdx.x % mx), j = cy + 2 * (int)((blockIdx.x / mx) % my), k = cz + 2 * (int)(blockIdx.x / (mx * my));
    int x0, x1, y0, y1, z0, z1;
    warp_support(i, L.g, sw, x0, x1);
    warp_support(j, L.g, sh, y0, y1);
    warp_support(k, L.g, sd, z0, z1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return;   // uniform: an empty support, the node stays
    const int tid = threadIdx.x;
    warp_stage<NT>(D, L, i, j, k, ld);
    if (tid < 12) lm[tid] = map.v[tid];
    if (tid == 0) ladm = 1u;
    __syncthreads();
    if (tid < 6 && warp_staged_admissible(ld, L, i, j, k, tid + 1, step, limit)) atomicOr(&ladm, 2u << tid);
    __syncthreads();
    const unsigned mask = ladm;
    const int g = L.g, ex = x1 - x0 + 1, ey = y1 - y0 + 1, n = ex * ey * (z1 - z0 + 1);
    int acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int v = tid; v < n; v += NT) {
        const int x = x0 + v % ex, y = y0 + (v / ex) % ey, z = z0 + v / (ex * ey);
        int n0, n1, n2;
        const int ws = warp_staged_corners(ld, g, x, y, z, i, j, k, n0, n1, n2) * step;   // <= g^3 * 32767
        const unsigned a = reg_tissue(subject, sbytes, ((int64_t)z * sh + y) * sw + x, T);
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        const WarpVotes r = warp_votes(a, px, py, pz, n0, n1, n2, ws, L.scale, tmpl, tbytes, tw, th, td, T, mask);
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[c] += r.v[c];
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        int s = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) lsum[(tid >> 6) * 7 + c] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int score[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            score[c] = 0;
            for (int w = 0; w < NT / 64; ++w) score[c] += lsum[w * 7 + c];
        }
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
__global__ void __launch_bounds__(WARP_T) k_warp_vox(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                     const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T, WarpMap map,
                                                     const int32_t* __restrict__ D, WarpLat L, int colour, int step, int* __restrict__ cnt,
                                                     const u64* prev) {
    __shared__ float lm[12];
    if (prev && *prev == 0ull) return;
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = sw * sh * sd, g = L.g;
    for (int64_t i64 = (int64_t)blockIdx.x * WARP_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * WARP_T) {
        const int v = (int)i64, x = v % sw, y = (v / sw) % sh, z = v / (sw * sh);
        const int i = warp_owner(x, L.lg, g, colour & 1), j = warp_owner(y, L.lg, g, (colour >> 1) & 1), k = warp_owner(z, L.lg, g, colour >> 2);
        if (i < 0 || j < 0 || k < 0) continue;
        int n0, n1, n2;
        warp_corners(D, L, x, y, z, n0, n1, n2);
        const int ws = (g - abs(x - i * g)) * (g - abs(y - j * g)) * (g - abs(z - k * g)) * step;
        const unsigned a = reg_tissue(subject, sbytes, v, T);
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        // every candidate, admissible or not (the pick kernel knows): |n +- ws| <= 2 g^3 * 32767 < 2^31
        const WarpVotes r = warp_votes(a, px, py, pz, n0, n1, n2, ws, L.scale, tmpl, tbytes, tw, th, td, T, 0x7Fu);
        int* c7 = cnt + (((size_t)k * L.ny + j) * L.nx + i) * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c)
            if (r.v[c]) atomicAdd(c7 + c, r.v[c]);
    }
}

__global__ void __launch_bounds__(WARP_T) k_warp_pick(int sw, int sh, int sd, int32_t* D, WarpLat L, int colour, int step, int limit,
                                                      int* __restrict__ cnt, u64* info, const u64* prev) {
    if (prev && *prev == 0ull) return;
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u, mz = (unsigned)(L.nz - cz + 1) / 2u;
    const int64_t nodes = (int64_t)mx * my * mz;
    for (int64_t b = (int64_t)blockIdx.x * WARP_T + threadIdx.x; b < nodes; b += (int64_t)gridDim.x * WARP_T) {
        const int i = cx + 2 * (int)(b % mx), j = cy + 2 * (int)((b / mx) % my), k = cz + 2 * (int)(b / ((int64_t)mx * my));
        int x0, x1, y0, y1, z0, z1;
        warp_support(i, L.g, sw, x0, x1);
        warp_support(j, L.g, sh, y0, y1);
        warp_support(k, L.g, sd, z0, z1);
        if (x0 > x1 || y0 > y1 || z0 > z1) continue;   // no voxel added anything: the counters are still zero
        const size_t node = ((size_t)k * L.ny + j) * L.nx + i;
        int32_t* d = D + node * 3;
        const int d0 = d[0], d1 = d[1], d2 = d[2];
        const unsigned mask = warp_pick_mask(D, L, i, j, k, d0, d1, d2, step, limit);
        int score[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            score[c] = cnt[node * 7 + c];
            cnt[node * 7 + c] = 0;
        }
        const int best = warp_best(score, mask);
        if (best) {
            const int axis = (best - 1) >> 1, delta = (best & 1) ? step : -step;
            d[axis] = (axis == 0 ? d0 : axis == 1 ? d1 : d2) + delta;
            atomicAdd(info, 1ull);
        }
        atomicAdd(info + 1, 1ull);
    }
}

// ---- refine, the report, carry ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WARP_T) k_warp_refine(const int32_t* __restrict__ coarse, WarpLat C, WarpLat F, int32_t* __restrict__ fine) {
    const int64_t nodes = (int64_t)F.nx * F.ny * F.nz;
    for (int64_t e = (int64_t)blockIdx.x * WARP_T + threadIdx.x; e < nodes; e += (int64_t)gridDim.x * WARP_T) {
        const int i = (int)(e % F.nx), j = (int)((e / F.nx) % F.ny), k = (int)(e / ((int64_t)F.nx * F.ny));
        const int ia[2] = {i >> 1, min((i >> 1) + (i & 1), C.nx - 1)}, ja[2] = {j >> 1, min((j >> 1) + (j & 1), C.ny - 1)},
                  ka[2] = {k >> 1, min((k >> 1) + (k & 1), C.nz - 1)};
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int32_t* d = coarse + (((size_t)ka[c >> 2] * C.ny + ja[(c >> 1) & 1]) * C.nx + ia[c & 1]) * 3;
            s0 += d[0];
            s1 += d[1];
            s2 += d[2];
        }
        fine[e * 3 + 0] = (s0 + 4) >> 3;
        fine[e * 3 + 1] = (s1 + 4) >> 3;
        fine[e * 3 + 2] = (s2 + 4) >> 3;
    }
}

// slots: the max_sweeps {changed, visited} pairs of this (level, step); sweep s ran when s == 0 or sweep s - 1 changed a node
__global__ void k_warp_row(const uint32_t* __restrict__ hist, int T, const u64* __restrict__ slots, int max_sweeps, int g, int step,
                           int64_t* __restrict__ row) {
    if (threadIdx.x) return;
    long long sc = 0;
    for (int a = 0; a < T; ++a)
        for (int b = 0; b < T; ++b) {
            const long long n = (long long)hist[a * T + b];
            sc += a == b ? (a ? n : 0) : -n;
        }
    int ran = 1;
    while (ran < max_sweeps && slots[2 * (ran - 1)]) ++ran;
    row[0] = g;
    row[1] = step;
    row[2] = ran;
    row[3] = (int64_t)slots[2 * (ran - 1)];
    row[4] = sc;
}

__global__ void __launch_bounds__(WARP_T) k_warp_carry(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                       const void* __restrict__ tmpl, int tbytes, int tw, int th, int td,
                                                       const uint16_t* __restrict__ atlas, int T, WarpMap map, const int32_t* __restrict__ D,
                                                       WarpLat L, uint16_t* __restrict__ out, uint32_t* __restrict__ counts) {
    __shared__ unsigned lc[3 * WARP_MAXT];
    __shared__ float lm[12];
    if (threadIdx.x < 3 * WARP_MAXT) lc[threadIdx.x] = 0u;
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = sw * sh * sd;
    for (int64_t i64 = (int64_t)blockIdx.x * WARP_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * WARP_T) {
        const int i = (int)i64;
        const unsigned a = reg_tissue(subject, sbytes, i, T);
        if (a == 0u) {
            out[i] = 0;
            continue;
        }
        const int x = i % sw, y = (i / sw) % sh, z = i / (sw * sh);
        const AffPos p = warp_locate(lm, D, L, x, y, z, tw, th, td);
        unsigned result;
        const unsigned kind = reg_carry_at(p, a, tmpl, tbytes, tw, th, td, atlas, T, result);
        out[i] = (uint16_t)result;
        if (counts) atomicAdd(&lc[kind * (unsigned)T + a], 1u);
    }
    if (counts) {
        __syncthreads();
        if ((int)threadIdx.x < 3 * T && lc[threadIdx.x]) atomicAdd(counts + threadIdx.x, lc[threadIdx.x]);
    }
}

void warp_memset(void* p, int value, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, value, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_warp: hipMemsetAsync: ") + hipGetErrorString(e));
}
int warp_blocks(int64_t items) {
    const int64_t nb = (items + WARP_T - 1) / WARP_T;
    return (int)(nb > WARP_MAXB ? WARP_MAXB : nb < 1 ? 1 : nb);
}
struct Grids {   // what every kernel over the two tissue maps takes
    const void* subject; int sbytes, sw, sh, sd;
    const void* tmpl;    int tbytes, tw, th, td;
    int T;
};

void warp_hist_into(const Grids& G, const WarpMap& m, const int32_t* D, const WarpLat& L, uint32_t* hist, hipStream_t s) {
    warp_memset(hist, 0, (size_t)G.T * G.T * 4, s);
    k_warp_hist<<<warp_blocks((int64_t)G.sw * G.sh * G.sd), WARP_T, 0, s>>>(G.subject, G.sbytes, G.sw, G.sh, G.sd, G.tmpl, G.tbytes, G.tw, G.th,
                                                                         G.td, G.T, m, D, L, hist);
}

// one sweep: the 8 colour passes.  cnt: zero on entry under IMPL_VOXEL, and left zero
void warp_sweep_into(const Grids& G, const WarpMap& m, int32_t* D, const WarpLat& L, int step, int limit, u64* info, const u64* prev, int impl,
                     int* cnt, hipStream_t s) {
    for (int c = 0; c < 8; ++c) {
        const int64_t nodes = (int64_t)((L.nx - (c & 1) + 1) / 2) * ((L.ny - ((c >> 1) & 1) + 1) / 2) * ((L.nz - (c >> 2) + 1) / 2);
        if (impl == UNET_WARP_IMPL_VOXEL) {
            k_warp_vox<<<warp_blocks((int64_t)G.sw * G.sh * G.sd), WARP_T, 0, s>>>(G.subject, G.sbytes, G.sw, G.sh, G.sd, G.tmpl, G.tbytes, G.tw,
                                                                                G.th, G.td, G.T, m, D, L, c, step, cnt, prev);
            k_warp_pick<<<warp_blocks(nodes), WARP_T, 0, s>>>(G.sw, G.sh, G.sd, D, L, c, step, limit, cnt, info, prev);
            continue;
        }
        // DEFAULT: NODE
#define UNET_WARP_NODE(NT)                                                                                                              \
    k_warp_node<NT><<<(unsigned)nodes, NT, 0, s>>>(G.subject, G.sbytes, G.sw, G.sh, G.sd, G.tmpl, G.tbytes, G.tw, G.th, G.td, G.T, m, D, L, c, \
                                                   step, limit, info, prev)
        if (L.g == 4) UNET_WARP_NODE(64);
        else if (L.g == 8) UNET_WARP_NODE(256);
        else UNET_WARP_NODE(1024);
#undef UNET_WARP_NODE
    }
}

}  // namespace

size_t warp_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels) {
    return 256 + warp_scratch(nullptr, sw, sh, sd, levels, n_levels).bytes;
}

void launch_warp_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                      const float* map, const int32_t* D, int g, uint32_t* hist, hipStream_t s) {
    const Grids G = {subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T};
    warp_hist_into(G, warp_map(map), D, warp_lattice(sw, sh, sd, g), hist, s);
}

void launch_warp_sweep(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                       const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch, hipStream_t s) {
    const Grids G = {subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T};
    const int level[5] = {g, step, step, 1, limit};
    const Scratch sc = warp_scratch(scratch, sw, sh, sd, level, 1);
    const WarpLat L = warp_lattice(sw, sh, sd, g);
    warp_memset(info, 0, 2 * sizeof(int64_t), s);
    if (impl == UNET_WARP_IMPL_VOXEL) warp_memset(sc.cnt, 0, warp_nodes(L) * 7 * sizeof(int), s);
    warp_sweep_into(G, warp_map(map), D, L, step, limit, (u64*)info, nullptr, impl, sc.cnt, s);
}

void launch_warp_refine(const int32_t* coarse, int sw, int sh, int sd, int g, int32_t* fine, hipStream_t s) {
    const WarpLat C = warp_lattice(sw, sh, sd, g), F = warp_lattice(sw, sh, sd, g / 2);
    k_warp_refine<<<warp_blocks((int64_t)warp_nodes(F)), WARP_T, 0, s>>>(coarse, C, F, fine);
}

void launch_warp_fit(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                     const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                     hipStream_t s) {
    const Grids G = {subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T};
    const Scratch sc = warp_scratch(scratch, sw, sh, sd, levels, n_levels);
    const WarpMap m = warp_map(map);
    warp_memset(report, 0xFF, (size_t)UNET_WARP_MAX_ROWS * 5 * sizeof(int64_t), s);   // -1 in every row
    warp_memset(sc.slots, 0, (size_t)WARP_SLOTS * 2 * sizeof(u64), s);
    if (impl == UNET_WARP_IMPL_VOXEL)
        warp_memset(sc.cnt, 0, warp_nodes(warp_lattice(sw, sh, sd, levels[5 * (n_levels - 1)])) * 7 * sizeof(int), s);
    int row = 0, slot = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* lv = levels + 5 * l;
        const WarpLat L = warp_lattice(sw, sh, sd, lv[0]);
        int32_t* D = l + 1 < n_levels ? sc.field[l] : D_out;
        if (l == 0) warp_memset(D, 0, warp_nodes(L) * 3 * sizeof(int32_t), s);
        for (int step = lv[1]; step >= lv[2]; step >>= 1, ++row) {
            const int first = slot;
            for (int k = 0; k < lv[3]; ++k, ++slot)
                warp_sweep_into(G, m, D, L, step, lv[4], sc.slots + 2 * slot, k ? sc.slots + 2 * (slot - 1) : nullptr, impl, sc.cnt, s);
            warp_hist_into(G, m, D, L, sc.hist, s);
            k_warp_row<<<1, 64, 0, s>>>(sc.hist, T, sc.slots + 2 * first, lv[3], lv[0], step, report + 5 * row);
        }
        if (l + 1 < n_levels) launch_warp_refine(D, sw, sh, sd, lv[0], l + 2 < n_levels ? sc.field[l + 1] : D_out, s);
    }
}

void launch_warp_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                       const uint16_t* atlas, int T, const float* map, const int32_t* D, int g, uint16_t* out, uint32_t* counts, hipStream_t s) {
    if (counts) warp_memset(counts, 0, (size_t)3 * T * 4, s);
    const int64_t S = (int64_t)sw * sh * sd;
    k_warp_carry<<<warp_blocks(S), WARP_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, atlas, T, warp_map(map), D,
                                                  warp_lattice(sw, sh, sd, g), out, counts);
}

}  // namespace unet
