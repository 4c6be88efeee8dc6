// The non-linear refinement of a co-registration (include/unet_cowarp.h): a Q8 displacement field on a lattice of spacing g, moved
// node by node towards a larger sum of point-wise mutual-information weights, and the resampling of the moving image through it.
// The sweeps under both implementations, the scratch and the schedule of a fit are lattice_fit.h's (shared with kernels_warp.hip)
// under the metric `Codes` below: a voxel is an intensity code or "none", a sample is worth its entry of the table W (2112 B at 32
// bins, staged in LDS and read there at data-dependent 2-byte addresses), and every sweep forms the histogram and W first.  The read
// of a code, the integer logarithm and the score are mi_score.h's (shared with kernels_coreg.hip).
//
//   k_cowarp_hist      grid-stride over row segments of CW_SEG voxels along x: the warped position, the nearest moving code, runs of
//                      equal (a, b) merged in registers, the block's bins * (bins + 1) counters in LDS, one global add per non-zero
//                      counter
//   k_cowarp_weights   one block: the histogram staged in LDS, a thread per row and per column sums it, N by lane shuffles of the row
//                      sums, a thread per cell runs the 16-squarings L, then a thread per row sets the outside column
//   k_cowarp_row       one block: a (level, step)'s report row from the sweeps' counts and the score of the histogram after them
//   k_cowarp_resample  a thread per fixed voxel in kernels_space.hip's bricks: p', the trilinear footprint, 8 gathers
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off (lattice_field.h).
#include "../../include/unet_cowarp.h"
#include "affine_search.h"
#include "device_util.h"
#include "lattice_fit.h"
#include "mi_score.h"

namespace unet {

namespace {

constexpr int CW_T = LAT_T;
constexpr int CW_SEG = 8;                    // voxels along x a thread of k_cowarp_hist takes at once
constexpr int CW_CELLS = UNET_COWARP_MAX_BINS * (UNET_COWARP_MAX_BINS + 1);
static_assert(WARP_MAX_DISP == UNET_COWARP_MAX_DISP, "lattice_field.h's range is this header's");
static_assert(LAT_IMPL_VOXEL == UNET_COWARP_IMPL_VOXEL && LAT_MAX_LEVELS >= UNET_COWARP_MAX_LEVELS &&
              LAT_MAX_SWEEPS == UNET_COWARP_MAX_SWEEPS && LAT_MAX_ROWS == UNET_COWARP_MAX_ROWS, "lattice_fit.h's schedule is this header's");
static_assert(UNET_COWARP_MAX_BINS == CO_MAXBINS && CW_T == CO_T, "mi_score.h scores with this file's block");
static_assert(31 * 31 * 31 == UNET_COWARP_MAX_SUPPORT && (long long)UNET_COWARP_MAX_SUPPORT * UNET_COWARP_MAX_WEIGHT < (1ll << 29),
              "seven int32 sums per node suffice");

struct Grids {   // what every kernel over the two code images takes, in lattice_fit.h's names: s the fixed grid, t the moving one
    const uint8_t* fixed;  int sw, sh, sd;
    const uint8_t* moving; int tw, th, td;
    int bins;
};

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
    const int nseg = (G.sw + CW_SEG - 1) / CW_SEG;
    const int64_t units = (int64_t)nseg * G.sh * G.sd;   // <= voxels < 2^31
    auto add = [&](unsigned key, unsigned n) { atomicAdd(&lh[key], n); };
    AffRun run = {0u, 0u};
    for (int64_t u = (int64_t)blockIdx.x * CW_T + threadIdx.x; u < units; u += (int64_t)gridDim.x * CW_T) {
        const unsigned u32 = (unsigned)u;
        const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg), y = r % G.sh, z = r / G.sh;
        const int x0 = seg * CW_SEG, n = min(CW_SEG, G.sw - x0);
        const int64_t row = ((int64_t)z * G.sh + y) * G.sw;
#pragma unroll
        for (int j = 0; j < CW_SEG; ++j) {
            if (j >= n) continue;
            const unsigned a = co_read(G.fixed, row + x0 + j, bins);
            if (a >= bins) continue;   // a fixed "none" voxel is not counted
            const AffPos p = warp_locate(lm, D, L, x0 + j, y, z, G.tw, G.th, G.td);
            unsigned b = bins;
            if (p.in) b = co_read(G.moving, ((int64_t)(int)floorf(p.qz) * G.th + (int)floorf(p.qy)) * G.tw + (int)floorf(p.qx), bins);
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

// ---- the report, resample --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CW_T) k_cowarp_row(const uint32_t* __restrict__ hist, int bins, const u64* __restrict__ slots, int max_sweeps,
                                                     int g, int step, int64_t* __restrict__ row) {
    __shared__ CoScoreLds sh;
    co_scores(hist, 1, bins, sh);   // ends on a barrier
    if (threadIdx.x) return;
    lat_row(slots, max_sweeps, g, step, row);
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

void cw_hist_into(const Grids& G, const WarpMap& m, const int32_t* D, const WarpLat& L, uint32_t* hist, const u64* prev, hipStream_t s) {
    lat_memset("unet_cowarp", hist, 0, (size_t)G.bins * (G.bins + 1) * 4, s);
    const int64_t units = (int64_t)((G.sw + CW_SEG - 1) / CW_SEG) * G.sh * G.sd;
    k_cowarp_hist<<<lat_blocks(units), CW_T, 0, s>>>(G, m, D, L, hist, prev);
}

// ---- the metric of lattice_fit.h -------------------------------------------------------------------------------------------------
struct Codes {
    typedef unet::Grids Grids;
    typedef const int16_t* Table;   // W in LDS
    static constexpr int COUNTERS = 8;
    static constexpr const char* NAME = "unet_cowarp";
    static constexpr size_t HIST_BYTES = (size_t)CW_CELLS * 4, EXTRA_BYTES = (size_t)CW_CELLS * 2;
    Grids G;
    const int16_t* __restrict__ w;   // W in the scratch
    Codes(const Grids& g, const LatScratch& sc) : G(g), w((const int16_t*)sc.extra) {}

    template <int NT> __device__ __forceinline__ Table stage() const {
        __shared__ int16_t lw[CW_CELLS];
        const unsigned bins = (unsigned)G.bins;
        for (unsigned e = threadIdx.x; e < bins * (bins + 1u); e += NT) lw[e] = w[e];
        return lw;
    }
    __device__ __forceinline__ bool fixed(int64_t v, unsigned& a) const {
        a = co_read(G.fixed, v, (unsigned)G.bins);
        return a < (unsigned)G.bins;
    }
    // an outside sample reads `bins`
    __device__ __forceinline__ WarpVotes seven(unsigned a, float px, float py, float pz, int n0, int n1, int n2, int ws, float scale, Table lw,
                                               unsigned mask) const {
        const unsigned bins = (unsigned)G.bins;
        const int16_t* row = lw + a * (bins + 1u);
        return warp_seven(px, py, pz, n0, n1, n2, ws, scale, G.tw, G.th, G.td, mask,
                          [&](int o) { return o < 0 ? bins : co_read(G.moving, o, bins); }, [&](unsigned b) { return (int)row[b]; });
    }
    void before_sweep(const WarpMap& m, const int32_t* D, const WarpLat& L, const LatScratch& sc, const u64* prev, hipStream_t s) const {
        cw_hist_into(G, m, D, L, sc.hist, prev, s);
        k_cowarp_weights<<<1, CW_T, 0, s>>>(sc.hist, G.bins, (int16_t*)sc.extra, prev);
    }
    void row(const WarpMap& m, const int32_t* D, const WarpLat& L, const LatScratch& sc, const u64* slots, int max_sweeps, int step,
             int64_t* row, hipStream_t s) const {
        cw_hist_into(G, m, D, L, sc.hist, nullptr, s);
        k_cowarp_row<<<1, CW_T, 0, s>>>(sc.hist, G.bins, slots, max_sweeps, L.g, step, row);
    }
};

}  // namespace

size_t cowarp_scratch_bytes(int fw, int fh, int fd, const int* levels, int n_levels) {
    return lat_scratch_bytes<Codes>(fw, fh, fd, levels, n_levels);
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
    lat_sweep<Codes>({fixed, fw, fh, fd, moving, mw, mh, md, bins}, map, D, g, step, limit, info, impl, scratch, s);
}

void launch_cowarp_fit(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                       const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                       hipStream_t s) {
    lat_fit<Codes>({fixed, fw, fh, fd, moving, mw, mh, md, bins}, map, levels, n_levels, D_out, report, impl, scratch, s);
}

void launch_cowarp_resample(const float* moving, int mw, int mh, int md, int fw, int fh, int fd, const float* map, const int32_t* D, int g,
                            float* out, hipStream_t s) {
    k_cowarp_resample<<<(unsigned)space_bricks(fw, fh, fd), CW_T, 0, s>>>(moving, mw, mh, md, fw, fh, fd, (fw + BRICK_X - 1) / BRICK_X,
                                                                         (fh + BRICK_Y - 1) / BRICK_Y, warp_map(map), D,
                                                                         warp_lattice(fw, fh, fd, g), out);
}

}  // namespace unet
