// The non-linear refinement of a parcellation (include/unet_warp.h): a Q8 displacement field on a lattice of spacing g, moved node by
// node towards a better tissue agreement, and the carrying of an atlas through the warped map.  The sweeps under both implementations,
// the scratch and the schedule of a fit are lattice_fit.h's (shared with kernels_cowarp.hip) under the metric `Tissue` below: a voxel
// is a tissue class, every voxel counts, and a sample adds +1 where it agrees in a tissue, -1 where it differs.
//
//   k_warp_hist    grid-stride over the subject's voxels: the warped position, the nearest template tissue, the block's T*T counters
//                  in LDS, one global add per non-zero counter
//   k_warp_refine  a thread per fine node
//   k_warp_row     one thread: a (level, step)'s report row from the sweeps' counts and the histogram after them
//   k_warp_carry   one thread per subject voxel: kernels_register.hip's carry at the warped position (tissue_carry.h)
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off (lattice_field.h).
#include "../../include/unet_warp.h"
#include "affine_search.h"
#include "device_util.h"
#include "lattice_fit.h"
#include "tissue_carry.h"

namespace unet {

namespace {

constexpr int WARP_T = LAT_T, WARP_MAXT = UNET_WARP_MAX_TISSUES;
static_assert(WARP_MAX_DISP == UNET_WARP_MAX_DISP, "lattice_field.h's range is this header's");
static_assert(LAT_IMPL_VOXEL == UNET_WARP_IMPL_VOXEL && LAT_MAX_LEVELS == UNET_WARP_MAX_LEVELS && LAT_MAX_SWEEPS == UNET_WARP_MAX_SWEEPS &&
              LAT_MAX_ROWS == UNET_WARP_MAX_ROWS, "lattice_fit.h's schedule is this header's");

struct Grids {   // what every kernel over the two tissue maps takes
    const void* subject; int sbytes, sw, sh, sd;
    const void* tmpl;    int tbytes, tw, th, td;
    int T;
};

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

__global__ void k_warp_row(const uint32_t* __restrict__ hist, int T, const u64* __restrict__ slots, int max_sweeps, int g, int step,
                           int64_t* __restrict__ row) {
    if (threadIdx.x) return;
    long long sc = 0;
    for (int a = 0; a < T; ++a)
        for (int b = 0; b < T; ++b) {
            const long long n = (long long)hist[a * T + b];
            sc += a == b ? (a ? n : 0) : -n;
        }
    lat_row(slots, max_sweeps, g, step, row);
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

void warp_hist_into(const Grids& G, const WarpMap& m, const int32_t* D, const WarpLat& L, uint32_t* hist, hipStream_t s) {
    lat_memset("unet_warp", hist, 0, (size_t)G.T * G.T * 4, s);
    k_warp_hist<<<lat_blocks((int64_t)G.sw * G.sh * G.sd), WARP_T, 0, s>>>(G.subject, G.sbytes, G.sw, G.sh, G.sd, G.tmpl, G.tbytes, G.tw, G.th,
                                                                          G.td, G.T, m, D, L, hist);
}

// ---- the metric of lattice_fit.h -------------------------------------------------------------------------------------------------
struct Tissue {
    typedef unet::Grids Grids;
    struct Table {};   // nothing staged
    static constexpr int COUNTERS = 7;
    static constexpr const char* NAME = "unet_warp";
    static constexpr size_t HIST_BYTES = (size_t)WARP_MAXT * WARP_MAXT * 4, EXTRA_BYTES = 0;
    Grids G;
    Tissue(const Grids& g, const LatScratch&) : G(g) {}

    template <int NT> __device__ __forceinline__ Table stage() const { return Table(); }
    __device__ __forceinline__ bool fixed(int64_t v, unsigned& a) const {
        a = reg_tissue(G.subject, G.sbytes, v, G.T);
        return true;
    }
    // an outside sample reads tissue 0; a voxel of subject tissue a adds to agree - disagree when its template sample reads b
    __device__ __forceinline__ WarpVotes seven(unsigned a, float px, float py, float pz, int n0, int n1, int n2, int ws, float scale, Table,
                                               unsigned mask) const {
        return warp_seven(px, py, pz, n0, n1, n2, ws, scale, G.tw, G.th, G.td, mask,
                          [&](int o) { return o < 0 ? 0u : reg_tissue(G.tmpl, G.tbytes, o, G.T); },
                          [&](unsigned b) { return a == b ? (a ? 1 : 0) : -1; });
    }
    void before_sweep(const WarpMap&, const int32_t*, const WarpLat&, const LatScratch&, const u64*, hipStream_t) const {}
    void row(const WarpMap& m, const int32_t* D, const WarpLat& L, const LatScratch& sc, const u64* slots, int max_sweeps, int step,
             int64_t* row, hipStream_t s) const {
        warp_hist_into(G, m, D, L, sc.hist, s);
        k_warp_row<<<1, 64, 0, s>>>(sc.hist, G.T, slots, max_sweeps, L.g, step, row);
    }
};

}  // namespace

size_t warp_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels) {
    return lat_scratch_bytes<Tissue>(sw, sh, sd, levels, n_levels);
}

void launch_warp_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                      const float* map, const int32_t* D, int g, uint32_t* hist, hipStream_t s) {
    const Grids G = {subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T};
    warp_hist_into(G, warp_map(map), D, warp_lattice(sw, sh, sd, g), hist, s);
}

void launch_warp_sweep(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                       const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch, hipStream_t s) {
    lat_sweep<Tissue>({subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T}, map, D, g, step, limit, info, impl, scratch, s);
}

void launch_warp_refine(const int32_t* coarse, int sw, int sh, int sd, int g, int32_t* fine, hipStream_t s) {
    const WarpLat C = warp_lattice(sw, sh, sd, g), F = warp_lattice(sw, sh, sd, g / 2);
    k_warp_refine<<<lat_blocks((int64_t)warp_nodes(F)), WARP_T, 0, s>>>(coarse, C, F, fine);
}

void launch_warp_fit(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                     const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                     hipStream_t s) {
    lat_fit<Tissue>({subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T}, map, levels, n_levels, D_out, report, impl, scratch, s);
}

void launch_warp_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                       const uint16_t* atlas, int T, const float* map, const int32_t* D, int g, uint16_t* out, uint32_t* counts, hipStream_t s) {
    if (counts) lat_memset("unet_warp", counts, 0, (size_t)3 * T * 4, s);
    const int64_t S = (int64_t)sw * sh * sd;
    k_warp_carry<<<lat_blocks(S), WARP_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, atlas, T, warp_map(map), D,
                                                 warp_lattice(sw, sh, sd, g), out, counts);
}

}  // namespace unet
