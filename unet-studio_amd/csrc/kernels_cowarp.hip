// The non-linear refinement of a co-registration (include/unet_cowarp.h): a Q8 displacement field on a lattice of spacing g, moved
// node by node towards a larger sum of point-wise mutual-information weights, and the resampling of the moving image through it.
// The lattice, the positions, admissibility and the choice are lattice_field.h's (shared with kernels_warp.hip, whose kernels these
// follow shape for shape); the read of a code, the integer logarithm and the score are mi_score.h's (shared with kernels_coreg.hip).
//
//   k_cowarp_hist      grid-stride over row segments of CW_SEG voxels along x: the warped position, the nearest moving code, runs of
//                      equal (a, b) merged in registers, the block's bins * (bins + 1) counters in LDS, one global add per non-zero
//                      counter
//   k_cowarp_weights   one block: the histogram staged in LDS, a thread per row and per column sums it, N by lane shuffles of the row
//                      sums, a thread per cell runs the 16-squarings L, then a thread per row sets the outside column
//   k_cowarp_node      IMPL_NODE, one colour pass: a block of NT threads (64 = one wave for g = 4, 256 for g = 8, 1024 for g = 16)
//                      per node of the colour.  W (2112 B at 32 bins) and the node's 3x3x3 neighbourhood of D are staged in LDS;
//                      every thread strides over the support with seven int32 sums and the count of voxels with a code in registers
//                      (a candidate whose nearest moving voxel is the unmoved one's reuses its code: no second gather); the sums are
//                      reduced by lane shuffles, then across waves through LDS, and thread 0 chooses and writes the node.  The
//                      table reads are data-dependent 2-byte LDS reads
//   k_cowarp_vox       IMPL_VOXEL, one colour pass: a thread per voxel finds the one node of the colour whose support holds it and
//                      adds its seven weights and a 1 into that node's 8 counters in the scratch (int atomics); W staged in LDS
//   k_cowarp_pick      IMPL_VOXEL: a thread per node of the colour: admissibility, the choice, the node, and the counters zeroed again
//   k_cowarp_row       one block: a (level, step)'s report row from the sweeps' counts and the score of the histogram after them
//   k_cowarp_resample  a thread per fixed voxel in kernels_space.hip's bricks: p', the trilinear footprint, 8 gathers
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off.  In a fit every sweep's kernels return at once when `prev`, the count of nodes the preceding
// sweep of the same (level, step) changed, is zero (stream order makes it final): the host reads nothing back.
//
// Scratch, each part 256-B aligned: the sweeps' {changed, visited} slots, a histogram, W, the counters of IMPL_VOXEL (8 per node of
// the finest lattice), the fields of all levels but the last.
#include <stdexcept>
#include <string>

#include "../../include/unet_cowarp.h"
#include "affine_search.h"
#include "device_util.h"
#include "kernels.h"
#include "lattice_field.h"
#include "mi_score.h"

namespace unet {

namespace {

constexpr int CW_T = 256;                    // threads per block of the per-voxel and per-node-thread kernels
constexpr int CW_MAXB = 8192;                // their grid cap; they stride over the rest
constexpr int CW_SEG = 8;                    // voxels along x a thread of k_cowarp_hist takes at once
constexpr int CW_CELLS = UNET_COWARP_MAX_BINS * (UNET_COWARP_MAX_BINS + 1);
constexpr int CW_SLOTS = UNET_COWARP_MAX_ROWS * UNET_COWARP_MAX_SWEEPS;
typedef unsigned long long u64;
static_assert(WARP_MAX_DISP == UNET_COWARP_MAX_DISP, "lattice_field.h's range is this header's");
static_assert(UNET_COWARP_MAX_BINS == CO_MAXBINS && CW_T == CO_T, "mi_score.h scores with this file's block");
static_assert(31 * 31 * 31 == UNET_COWARP_MAX_SUPPORT && (long long)UNET_COWARP_MAX_SUPPORT * UNET_COWARP_MAX_WEIGHT < (1ll << 29),
              "seven int32 sums per node suffice");

struct Scratch {
    u64* slots;        // CW_SLOTS x {changed, visited}
    uint32_t* hist;    // CW_CELLS
    int16_t* w;        // CW_CELLS
    int* cnt;          // 8 per node of the finest lattice
    int32_t* field[UNET_COWARP_MAX_LEVELS];   // the levels but the last
    size_t bytes;      // from the aligned base
};
Scratch cw_scratch(void* scratch, int fw, int fh, int fd, const int* levels, int n_levels) {
    char* b = (char*)warp_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s = {};
    size_t o = 0;
    s.slots = (u64*)(b + o);     o += warp_align((size_t)CW_SLOTS * 2 * sizeof(u64));
    s.hist = (uint32_t*)(b + o); o += warp_align((size_t)CW_CELLS * 4);
    s.w = (int16_t*)(b + o);     o += warp_align((size_t)CW_CELLS * 2);
    s.cnt = (int*)(b + o);       o += warp_align(warp_nodes(warp_lattice(fw, fh, fd, levels[5 * (n_levels - 1)])) * 8 * sizeof(int));
    for (int l = 0; l + 1 < n_levels; ++l) {
        s.field[l] = (int32_t*)(b + o);
        o += warp_align(warp_nodes(warp_lattice(fw, fh, fd, levels[5 * l])) * 3 * sizeof(int32_t));
    }
    s.bytes = o;
    return s;
}

struct Grids {   // what every kernel over the two code images takes
    const uint8_t* fixed;  int fw, fh, fd;
    const uint8_t* moving; int mw, mh, md;
    int bins;
};

// The seven weights of one voxel of fixed code a < bins (lattice_field.h's warp_seven): an outside sample reads `bins`.  lw: W in LDS
__device__ __forceinline__ WarpVotes cw_votes(unsigned a, float px, float py, float pz, int n0, int n1, int n2, int ws, float scale,
                                              const Grids& G, const int16_t* lw, unsigned mask) {
    const unsigned bins = (unsigned)G.bins;
    const int16_t* row = lw + a * (bins + 1u);
    return warp_seven(px, py, pz, n0, n1, n2, ws, scale, G.mw, G.mh, G.md, mask,
                      [&](int o) { return o < 0 ? bins : co_read(G.moving, o, bins); }, [&](unsigned b) { return (int)row[b]; });
}

// ---- the joint histogram ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CW_T) k_cowarp_hist(Grids G, WarpMap map, const int32_t* __restrict__ D, WarpLat L,
                                                      uint32_t* __restrict__ hist, const u64* prev) {
    __shared__ unsigned lh[CW_CELLS];
    __shared__ float lm[12];
    if (prev && *prev == 0ull) return;   // uniform: the preceding sweep is complete (stream order) and changed nothing
    const unsigned bins = (unsigned)G.bins, cols = bins + 1u, cells = bins * cols;
    for (unsigned e = threadIdx.x; e < cells; e += CW_T) lh[e] = 0u;
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int nseg = (G.fw + CW_SEG - 1) / CW_SEG;
    const int64_t units = (int64_t)nseg * G.fh * G.fd;   // <= voxels < 2^31
    auto add = [&](unsigned key, unsigned n) { atomicAdd(&lh[key], n); };
    AffRun run = {0u, 0u};
    for (int64_t u = (int64_t)blockIdx.x * CW_T + threadIdx.x; u < units; u += (int64_t)gridDim.x * CW_T) {
        const unsigned u32 = (unsigned)u;
        const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg), y = r % G.fh, z = r / G.fh;
        const int x0 = seg * CW_SEG, n = min(CW_SEG, G.fw - x0);
        const int64_t row = ((int64_t)z * G.fh + y) * G.fw;
#pragma unroll
        for (int j = 0; j < CW_SEG; ++j) {
            if (j >= n) continue;
            const unsigned a = co_read(G.fixed, row + x0 + j, bins);
            if (a >= bins) continue;   // a fixed "none" voxel is not counted
            const AffPos p = warp_locate(lm, D, L, x0 + j, y, z, G.mw, G.mh, G.md);
            unsigned b = bins;
            if (p.in) b = co_read(G.moving, ((int64_t)(int)floorf(p.qz) * G.mh + (int)floorf(p.qy)) * G.mw + (int)floorf(p.qx), bins);
            run.push(a * cols + b, add);
        }
    }
    run.close(add);
    __syncthreads();
    for (unsigned e = threadIdx.x; e < cells; e += CW_T)
        if (const unsigned c = lh[e]) atomicAdd(hist + e, c);
}

// ---- the weights -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CW_T) k_cowarp_weights(const uint32_t* __restrict__ hist, int bins, int16_t* __restrict__ w, const u64* prev) {
    __shared__ unsigned lh[CW_CELLS];
    __shared__ int lr[UNET_COWARP_MAX_BINS], lc[UNET_COWARP_MAX_BINS], lw[CW_CELLS], ln;
    if (prev && *prev == 0ull) return;
    const int tid = threadIdx.x, cols = bins + 1, cells = bins * cols;
    for (int e = tid; e < cells; e += CW_T) lh[e] = hist[e];
    __syncthreads();
    if (tid < 64) {   // wave 0: a lane per row (bins <= 32), N by shuffles
        unsigned sum = 0u;
        if (tid < bins)
            for (int b = 0; b < cols; ++b) sum += lh[tid * cols + b];
        if (tid < bins) lr[tid] = co_ilog(sum);
        unsigned total = sum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
        if (tid == 0) ln = co_ilog(total);
    } else if (tid < 64 + bins) {   // wave 1: a lane per column b < bins
        const int b = tid - 64;
        unsigned sum = 0u;
        for (int a = 0; a < bins; ++a) sum += lh[a * cols + b];
        lc[b] = co_ilog(sum);
    }
    __syncthreads();
    for (int e = tid; e < bins * bins; e += CW_T) {
        const int a = e / bins, b = e - a * bins;
        lw[a * cols + b] = (co_ilog(lh[a * cols + b]) + ln - lr[a] - lc[b]) >> 8;   // arithmetic
    }
    __syncthreads();
    if (tid < bins) {
        int low = 0;
        for (int b = 0; b < bins; ++b) low = min(low, lw[tid * cols + b]);
        lw[tid * cols + bins] = low;
    }
    __syncthreads();
    for (int e = tid; e < cells; e += CW_T) w[e] = (int16_t)lw[e];
}

// ---- a colour pass, a block per node ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) k_cowarp_node(Grids G, WarpMap map, int32_t* D, WarpLat L, const int16_t* __restrict__ w, int colour,
                                                    int step, int limit, u64* info, const u64* prev) {
    __shared__ float lm[12];
    __shared__ int ld[27 * 3];          // the 3x3x3 neighbourhood, x fastest then component; a node that does not exist holds 0
    __shared__ int16_t lw[CW_CELLS];
    __shared__ unsigned ladm;
    __shared__ int lsum[(NT / 64) * 8];
    if (prev && *prev == 0ull) return;  // uniform
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u;
    const int i = cx + 2 * (int)(blockIdx.x % mx), j = cy + 2 * (int)((blockIdx.x / mx) % my), k = cz + 2 * (int)(blockIdx.x / (mx * my));
    int x0, x1, y0, y1, z0, z1;
    warp_support(i, L.g, G.fw, x0, x1);
    warp_support(j, L.g, G.fh, y0, y1);
    warp_support(k, L.g, G.fd, z0, z1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return;   // uniform: no voxel at all, the node stays
    const int tid = threadIdx.x;
    const unsigned bins = (unsigned)G.bins;
    warp_stage<NT>(D, L, i, j, k, ld);
    for (unsigned e = tid; e < bins * (bins + 1u); e += NT) lw[e] = w[e];
    if (tid < 12) lm[tid] = map.v[tid];
    if (tid == 0) ladm = 1u;
    __syncthreads();
    if (tid < 6 && warp_staged_admissible(ld, L, i, j, k, tid + 1, step, limit)) atomicOr(&ladm, 2u << tid);
    __syncthreads();
    const unsigned mask = ladm;
    const int g = L.g, ex = x1 - x0 + 1, ey = y1 - y0 + 1, n = ex * ey * (z1 - z0 + 1);   // <= 31^3
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the seven sums, each below 2^29, and the voxels with a code
    for (int v = tid; v < n; v += NT) {
        const int x = x0 + v % ex, y = y0 + (v / ex) % ey, z = z0 + v / (ex * ey);
        const unsigned a = co_read(G.fixed, ((int64_t)z * G.fh + y) * G.fw + x, bins);
        if (a >= bins) continue;
        int n0, n1, n2;
        const int ws = warp_staged_corners(ld, g, x, y, z, i, j, k, n0, n1, n2) * step;   // <= g^3 * 32767
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        const WarpVotes r = cw_votes(a, px, py, pz, n0, n1, n2, ws, L.scale, G, lw, mask);
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[c] += r.v[c];
        ++acc[7];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int s = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) lsum[(tid >> 6) * 8 + c] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int score[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            score[c] = 0;
            for (int wv = 0; wv < NT / 64; ++wv) score[c] += lsum[wv * 8 + c];
        }
        if (score[7] == 0) return;   // no voxel with a code: not visited
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
__global__ void __launch_bounds__(CW_T) k_cowarp_vox(Grids G, WarpMap map, const int32_t* __restrict__ D, WarpLat L,
                                                     const int16_t* __restrict__ w, int colour, int step, int* __restrict__ cnt,
                                                     const u64* prev) {
    __shared__ float lm[12];
    __shared__ int16_t lw[CW_CELLS];
    if (prev && *prev == 0ull) return;
    const unsigned bins = (unsigned)G.bins;
    for (unsigned e = threadIdx.x; e < bins * (bins + 1u); e += CW_T) lw[e] = w[e];
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = G.fw * G.fh * G.fd, g = L.g;
    for (int64_t i64 = (int64_t)blockIdx.x * CW_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * CW_T) {
        const int v = (int)i64, x = v % G.fw, y = (v / G.fw) % G.fh, z = v / (G.fw * G.fh);
        const int i = warp_owner(x, L.lg, g, colour & 1), j = warp_owner(y, L.lg, g, (colour >> 1) & 1), k = warp_owner(z, L.lg, g, colour >> 2);
        if (i < 0 || j < 0 || k < 0) continue;
        const unsigned a = co_read(G.fixed, v, bins);
        if (a >= bins) continue;
        int n0, n1, n2;
        warp_corners(D, L, x, y, z, n0, n1, n2);
        const int ws = (g - abs(x - i * g)) * (g - abs(y - j * g)) * (g - abs(z - k * g)) * step;
        float px, py, pz;
        warp_affine(lm, x, y, z, px, py, pz);
        // every candidate, admissible or not (the pick kernel knows): |n +- ws| <= 2 g^3 * 32767 < 2^31
        const WarpVotes r = cw_votes(a, px, py, pz, n0, n1, n2, ws, L.scale, G, lw, 0x7Fu);
        int* c8 = cnt + (((size_t)k * L.ny + j) * L.nx + i) * 8;
#pragma unroll
        for (int c = 0; c < 7; ++c)
            if (r.v[c]) atomicAdd(c8 + c, r.v[c]);
        atomicAdd(c8 + 7, 1);
    }
}

__global__ void __launch_bounds__(CW_T) k_cowarp_pick(int fw, int fh, int fd, int32_t* D, WarpLat L, int colour, int step, int limit,
                                                      int* __restrict__ cnt, u64* info, const u64* prev) {
    if (prev && *prev == 0ull) return;
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u, mz = (unsigned)(L.nz - cz + 1) / 2u;
    const int64_t nodes = (int64_t)mx * my * mz;
    for (int64_t b = (int64_t)blockIdx.x * CW_T + threadIdx.x; b < nodes; b += (int64_t)gridDim.x * CW_T) {
        const int i = cx + 2 * (int)(b % mx), j = cy + 2 * (int)((b / mx) % my), k = cz + 2 * (int)(b / ((int64_t)mx * my));
        const size_t node = ((size_t)k * L.ny + j) * L.nx + i;
        if (cnt[node * 8 + 7] == 0) continue;   // no voxel with a code added anything: the counters are still zero
        int32_t* d = D + node * 3;
        const int d0 = d[0], d1 = d[1], d2 = d[2];
        const unsigned mask = warp_pick_mask(D, L, i, j, k, d0, d1, d2, step, limit);
        int score[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            score[c] = cnt[node * 8 + c];
            cnt[node * 8 + c] = 0;
        }
        cnt[node * 8 + 7] = 0;
        const int best = warp_best(score, mask);
        if (best) {
            const int axis = (best - 1) >> 1, delta = (best & 1) ? step : -step;
            d[axis] = (axis == 0 ? d0 : axis == 1 ? d1 : d2) + delta;
            atomicAdd(info, 1ull);
        }
        atomicAdd(info + 1, 1ull);
    }
}

// ---- the report, resample --------------------------------------------------------------------------------------------------------
// slots: the max_sweeps {changed, visited} pairs of this (level, step); sweep s ran when s == 0 or sweep s - 1 changed a node
__global__ void __launch_bounds__(CW_T) k_cowarp_row(const uint32_t* __restrict__ hist, int bins, const u64* __restrict__ slots, int max_sweeps,
                                                     int g, int step, int64_t* __restrict__ row) {
    __shared__ CoScoreLds sh;
    co_scores(hist, 1, bins, sh);   // ends on a barrier
    if (threadIdx.x) return;
    int ran = 1;
    while (ran < max_sweeps && slots[2 * (ran - 1)]) ++ran;
    row[0] = g;
    row[1] = step;
    row[2] = ran;
    row[3] = (int64_t)slots[2 * (ran - 1)];
    row[4] = (int64_t)sh.score[0];
}

__global__ void __launch_bounds__(CW_T) k_cowarp_resample(const float* __restrict__ moving, int mw, int mh, int md, int fw, int fh, int fd,
                                                          int gx, int gy, WarpMap map, const int32_t* __restrict__ D, WarpLat L,
                                                          float* __restrict__ out) {
    int x, y, z;
    if (!brick_walk(fw, fh, fd, gx, gy, x, y, z)) return;
    float px, py, pz;
    int n0, n1, n2;
    warp_affine(map.v, x, y, z, px, py, pz);
    warp_corners(D, L, x, y, z, n0, n1, n2);
    const Tri t = locate(warp_p(px, n0, L.scale), warp_p(py, n1, L.scale), warp_p(pz, n2, L.scale), mw, mh, md);
    out[((int64_t)z * fh + y) * fw + x] = t.ok ? trilinear(t, moving) : 0.f;
}

void cw_memset(void* p, int value, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, value, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_cowarp: hipMemsetAsync: ") + hipGetErrorString(e));
}
int cw_blocks(int64_t items) {
    const int64_t nb = (items + CW_T - 1) / CW_T;
    return (int)(nb > CW_MAXB ? CW_MAXB : nb < 1 ? 1 : nb);
}

void cw_hist_into(const Grids& G, const WarpMap& m, const int32_t* D, const WarpLat& L, uint32_t* hist, const u64* prev, hipStream_t s) {
    cw_memset(hist, 0, (size_t)G.bins * (G.bins + 1) * 4, s);
    const int64_t units = (int64_t)((G.fw + CW_SEG - 1) / CW_SEG) * G.fh * G.fd;
    k_cowarp_hist<<<cw_blocks(units), CW_T, 0, s>>>(G, m, D, L, hist, prev);
}

// one sweep: the hist, the weights, the 8 colour passes.  cnt: zero on entry under IMPL_VOXEL, and left zero
void cw_sweep_into(const Grids& G, const WarpMap& m, int32_t* D, const WarpLat& L, int step, int limit, u64* info, const u64* prev, int impl,
                   const Scratch& sc, hipStream_t s) {
    cw_hist_into(G, m, D, L, sc.hist, prev, s);
    k_cowarp_weights<<<1, CW_T, 0, s>>>(sc.hist, G.bins, sc.w, prev);
    for (int c = 0; c < 8; ++c) {
        const int64_t nodes = (int64_t)((L.nx - (c & 1) + 1) / 2) * ((L.ny - ((c >> 1) & 1) + 1) / 2) * ((L.nz - (c >> 2) + 1) / 2);
        if (impl == UNET_COWARP_IMPL_VOXEL) {
            k_cowarp_vox<<<cw_blocks((int64_t)G.fw * G.fh * G.fd), CW_T, 0, s>>>(G, m, D, L, sc.w, c, step, sc.cnt, prev);
            k_cowarp_pick<<<cw_blocks(nodes), CW_T, 0, s>>>(G.fw, G.fh, G.fd, D, L, c, step, limit, sc.cnt, info, prev);
            continue;
        }
        // DEFAULT: NODE
        if (L.g == 4) k_cowarp_node<64><<<(unsigned)nodes, 64, 0, s>>>(G, m, D, L, sc.w, c, step, limit, info, prev);
        else if (L.g == 8) k_cowarp_node<256><<<(unsigned)nodes, 256, 0, s>>>(G, m, D, L, sc.w, c, step, limit, info, prev);
        else k_cowarp_node<1024><<<(unsigned)nodes, 1024, 0, s>>>(G, m, D, L, sc.w, c, step, limit, info, prev);
    }
}

}  // namespace

size_t cowarp_scratch_bytes(int fw, int fh, int fd, const int* levels, int n_levels) {
    return 256 + cw_scratch(nullptr, fw, fh, fd, levels, n_levels).bytes;
}

void launch_cowarp_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                        const float* map, const int32_t* D, int g, uint32_t* hist, hipStream_t s) {
    const Grids G = {fixed, fw, fh, fd, moving, mw, mh, md, bins};
    cw_hist_into(G, warp_map(map), D, warp_lattice(fw, fh, fd, g), hist, nullptr, s);
}

void launch_cowarp_weights(const uint32_t* hist, int bins, int16_t* weights, hipStream_t s) {
    k_cowarp_weights<<<1, CW_T, 0, s>>>(hist, bins, weights, nullptr);
}

void launch_cowarp_sweep(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                         const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch, hipStream_t s) {
    const Grids G = {fixed, fw, fh, fd, moving, mw, mh, md, bins};
    const int level[5] = {g, step, step, 1, limit};
    const Scratch sc = cw_scratch(scratch, fw, fh, fd, level, 1);
    const WarpLat L = warp_lattice(fw, fh, fd, g);
    cw_memset(info, 0, 2 * sizeof(int64_t), s);
    if (impl == UNET_COWARP_IMPL_VOXEL) cw_memset(sc.cnt, 0, warp_nodes(L) * 8 * sizeof(int), s);
    cw_sweep_into(G, warp_map(map), D, L, step, limit, (u64*)info, nullptr, impl, sc, s);
}

void launch_cowarp_fit(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                       const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                       hipStream_t s) {
    const Grids G = {fixed, fw, fh, fd, moving, mw, mh, md, bins};
    const Scratch sc = cw_scratch(scratch, fw, fh, fd, levels, n_levels);
    const WarpMap m = warp_map(map);
    cw_memset(report, 0xFF, (size_t)UNET_COWARP_MAX_ROWS * 5 * sizeof(int64_t), s);   // -1 in every row
    cw_memset(sc.slots, 0, (size_t)CW_SLOTS * 2 * sizeof(u64), s);
    if (impl == UNET_COWARP_IMPL_VOXEL)
        cw_memset(sc.cnt, 0, warp_nodes(warp_lattice(fw, fh, fd, levels[5 * (n_levels - 1)])) * 8 * sizeof(int), s);
    int row = 0, slot = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* lv = levels + 5 * l;
        const WarpLat L = warp_lattice(fw, fh, fd, lv[0]);
        int32_t* D = l + 1 < n_levels ? sc.field[l] : D_out;
        if (l == 0) cw_memset(D, 0, warp_nodes(L) * 3 * sizeof(int32_t), s);
        for (int step = lv[1]; step >= lv[2]; step >>= 1, ++row) {
            const int first = slot;
            for (int k = 0; k < lv[3]; ++k, ++slot)
                cw_sweep_into(G, m, D, L, step, lv[4], sc.slots + 2 * slot, k ? sc.slots + 2 * (slot - 1) : nullptr, impl, sc, s);
            cw_hist_into(G, m, D, L, sc.hist, nullptr, s);
            k_cowarp_row<<<1, CW_T, 0, s>>>(sc.hist, bins, sc.slots + 2 * first, lv[3], lv[0], step, report + 5 * row);
        }
        // the refine of kernels_warp.hip: the lattices are the same
        if (l + 1 < n_levels) launch_warp_refine(D, fw, fh, fd, lv[0], l + 2 < n_levels ? sc.field[l + 1] : D_out, s);
    }
}

void launch_cowarp_resample(const float* moving, int mw, int mh, int md, int fw, int fh, int fd, const float* map, const int32_t* D, int g,
                            float* out, hipStream_t s) {
    k_cowarp_resample<<<(unsigned)space_bricks(fw, fh, fd), CW_T, 0, s>>>(moving, mw, mh, md, fw, fh, fd, (fw + BRICK_X - 1) / BRICK_X,
                                                                         (fh + BRICK_Y - 1) / BRICK_Y, warp_map(map), D,
                                                                         warp_lattice(fw, fh, fd, g), out);
}

}  // namespace unet
