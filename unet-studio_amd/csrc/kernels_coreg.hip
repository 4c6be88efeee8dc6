// The co-registration of two intensity images (include/unet_coreg.h): codes, joint code histograms under K maps, the integer
// mutual-information score, and the pattern search over them.
//
//   k_coreg_code    one thread per voxel: fp32 -> uint8 code
//   k_coreg_hist    grid-stride over row segments of CO_SEG counted voxels along x; a thread reads its segment's fixed codes once and
//                   then, map by map, samples the moving codes at the nearest voxel and merges equal (map, a, b) keys in registers:
//                   one add per run, into the block's LDS table (TABLE counters: whole maps, flushed with one global add per
//                   non-zero counter; when the K maps do not fit, the block walks its voxels once per group of maps) or, TABLE == 0,
//                   into global memory.  The K maps are uniform across the block: they are staged in LDS once (from the launch
//                   arguments, or, DEV, from the search state together with K and the stride) and read from there at
//                   block-uniform addresses.  DEV: returns at once when the state says done
//   k_coreg_score   one block: the scores of K histograms
//   k_coreg_init    one block: the state of `init`, the candidates of iteration 0, zeroed counters, trace = -1
//   k_coreg_step    one block: scores, the winner, level / stage / state, the trace row, info, map_out, the next candidates, and the
//                   counters zeroed again.  Returns at once when the state says done.  Ordered after k_coreg_hist by the stream
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off: no incremental sums, so the numpy restatement rounds identically.  The search is the state
// machine of kernels_register.hip, statement for statement; the position of a voxel, the run merging and the state arithmetic are
// the one copy of affine_search.h, which both files inline (kernels_register.hip's emitted kernels did not change by the move).
// The read of a code, the integer logarithm and the scoring of histograms by one block are mi_score.h's, shared with
// kernels_cowarp.hip.
//
// Scratch of a search, each part 256-B aligned: the state (CoState), counters uint32[CO_MAXK * bins * (bins + 1)].
#include <stdexcept>
#include <string>

#include "../../include/unet_coreg.h"
#include "affine_search.h"
#include "device_util.h"
#include "mi_score.h"

namespace unet {

namespace {

static_assert(CO_MAXK == UNET_COREG_MAX_MAPS && CO_MAXBINS == UNET_COREG_MAX_BINS, "mi_score.h's sizes are this header's");
constexpr int CO_MAXB = 1024;                         // grid cap of k_coreg_hist and k_coreg_code; they stride over the rest
constexpr int CO_SEG = 8;                             // counted voxels along x a thread takes at once
constexpr int CO_TABLE_16 = CO_MAXK * 16 * 17;        // 6800 counters, 26.6 KiB: every map at 8 and 16 bins
constexpr int CO_TABLE_32 = 13 * 32 * 33;             // 13728 counters, 53.6 KiB: 13 of the 25 maps at 32 bins, two groups

struct CoMaps {   // K maps in the launch arguments
    float v[CO_MAXK * 12];
};
struct CoMap {
    float v[12];
};
struct CoPlan {   // what a search was asked for, in the launch arguments of k_coreg_init and k_coreg_step
    float step[12];
    int stages[UNET_COREG_MAX_STAGES][3];
    int n_stages, max_iterations, bins;
    float cx, cy, cz;
};
struct CoState {   // the device state of a search
    float c[12];                  // c0..c8 the matrix, c9..c11 the moving position of the fixed grid's centre voxel
    float cand[CO_MAXK * 12];     // the maps of the candidates of the coming iteration
    int K, stride, stage, level, done, converged;
};

size_t co_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    CoState* state;
    uint32_t* hist;
    size_t bytes;   // from the aligned base
};
Scratch co_scratch(void* scratch, int bins) {
    char* b = (char*)co_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    size_t o = 0;
    s.state = (CoState*)(b + o); o += co_align(sizeof(CoState));
    s.hist = (uint32_t*)(b + o); o += co_align((size_t)CO_MAXK * bins * (bins + 1) * 4);
    s.bytes = o;
    return s;
}

// ---- codes -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CO_T) k_coreg_code(const float* __restrict__ image, int64_t voxels, float lo, float scale, int bins,
                                                     uint8_t* __restrict__ codes) {
    for (int64_t i = (int64_t)blockIdx.x * CO_T + threadIdx.x; i < voxels; i += (int64_t)gridDim.x * CO_T) {
        const float v = image[i];
        const float t = __fmul_rn(__fsub_rn(v, lo), scale);   // one subtraction, one multiplication, never fused
        const int top = bins - 1;
        codes[i] = (uint8_t)(v != v ? bins : t < 0.f ? 0 : t >= (float)top ? top : (int)t);
    }
}

// ---- joint histograms ------------------------------------------------------------------------------------------------------------
// TABLE: the counters of the block's LDS table, 0 for global adds.  hist holds K * cells counters, all zero before the launch
template <int TABLE, bool DEV>
__global__ void __launch_bounds__(CO_T) k_coreg_hist(const uint8_t* __restrict__ fixed, int fw, int fh, int fd,
                                                     const uint8_t* __restrict__ moving, int mw, int mh, int md, int bins_arg, CoMaps maps,
                                                     int K_arg, int stride_arg, const CoState* __restrict__ st, uint32_t* __restrict__ hist) {
    constexpr bool LDS = TABLE > 0;
    __shared__ float lm[CO_MAXK * 12];
    __shared__ unsigned lh[LDS ? TABLE : 1];
    int K = K_arg, s = stride_arg;
    if constexpr (DEV) {
        if (st->done) return;   // uniform: k_coreg_step of the iteration before is complete (stream order)
        K = st->K;
        s = st->stride;
        for (int e = threadIdx.x; e < K * 12; e += CO_T) lm[e] = st->cand[e];
    } else {
        for (int e = threadIdx.x; e < K * 12; e += CO_T) lm[e] = maps.v[e];
    }
    const unsigned bins = (unsigned)bins_arg, cols = bins + 1u, cells = bins * cols;
    // the maps a walk over the voxels takes: all K, or as many whole maps as the table holds (the launcher picks TABLE >= cells)
    const int group = LDS ? min(K, TABLE / (int)cells) : K;
    // the counted voxels form an nx x ny x nz grid; a unit is CO_SEG of them along x
    const int nx = (fw + s - 1) / s, ny = (fh + s - 1) / s, nz = (fd + s - 1) / s, nseg = (nx + CO_SEG - 1) / CO_SEG;
    const int64_t units = (int64_t)nseg * ny * nz;
    for (int k0 = 0; k0 < K; k0 += group) {   // at most CO_MAXK walks
        const int k1 = min(K, k0 + group);
        const unsigned used = (unsigned)(k1 - k0) * cells;
        if constexpr (LDS)
            for (unsigned e = threadIdx.x; e < used; e += CO_T) lh[e] = 0u;
        __syncthreads();   // also: lm is staged
        auto add = [&](unsigned key, unsigned n) {
            if constexpr (LDS) atomicAdd(&lh[key], n);
            else atomicAdd(hist + key, n);
        };
        AffRun run = {0u, 0u};
        for (int64_t u = (int64_t)blockIdx.x * CO_T + threadIdx.x; u < units; u += (int64_t)gridDim.x * CO_T) {
            const unsigned u32 = (unsigned)u;   // units <= voxels < 2^31: 32-bit division
            const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg);
            const int yi = (r % ny) * s, zi = (r / ny) * s, x0 = seg * CO_SEG, n = min(CO_SEG, nx - x0);
            const int64_t row = ((int64_t)zi * fh + yi) * fw;
            unsigned a[CO_SEG];   // the fixed code; bins: not counted (none, or past the row's end)
#pragma unroll
            for (int j = 0; j < CO_SEG; ++j) a[j] = j < n ? co_read(fixed, row + (int64_t)(x0 + j) * s, bins) : bins;
            for (int k = k0; k < k1; ++k) {
                const float* m = lm + k * 12;          // the same address in every lane: an LDS broadcast
                const unsigned kbase = (unsigned)(k - k0) * cells;
#pragma unroll
                for (int j = 0; j < CO_SEG; ++j) {
                    if (a[j] < bins) {
                        const AffPos p = aff_locate(m, (x0 + j) * s, yi, zi, mw, mh, md);
                        unsigned b = bins;
                        if (p.in) b = co_read(moving, ((int64_t)(int)floorf(p.qz) * mh + (int)floorf(p.qy)) * mw + (int)floorf(p.qx), bins);
                        run.push(kbase + a[j] * cols + b, add);
                    }
                }
            }
        }
        run.close(add);
        if constexpr (LDS) {
            __syncthreads();
            uint32_t* out = hist + (size_t)k0 * cells;
            for (unsigned e = threadIdx.x; e < used; e += CO_T)
                if (const unsigned c = lh[e]) atomicAdd(out + e, c);
            // the next walk zeroes lh[e] from the same thread that read it here, then meets the barrier above
        }
    }
}

// ---- the score -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CO_T) k_coreg_score(const uint32_t* __restrict__ hist, int K, int bins, int64_t* __restrict__ scores) {
    __shared__ CoScoreLds sh;
    co_scores(hist, K, bins, sh);
    if ((int)threadIdx.x < K) scores[threadIdx.x] = (int64_t)sh.score[threadIdx.x];
}

// ---- the search ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CO_T) k_coreg_init(CoState* st, uint32_t* __restrict__ hist, CoMap init, CoPlan p,
                                                     int64_t* __restrict__ trace, int64_t* __restrict__ info) {
#pragma clang fp contract(off)
    __shared__ float lc[12];
    if (threadIdx.x < 9) lc[threadIdx.x] = init.v[threadIdx.x];
    if (threadIdx.x < 3) {
        const int r = threadIdx.x;
        lc[9 + r] = ((init.v[3 * r] * p.cx + init.v[3 * r + 1] * p.cy) + init.v[3 * r + 2] * p.cz) + init.v[9 + r];
    }
    __syncthreads();
    if (threadIdx.x < 12) st->c[threadIdx.x] = lc[threadIdx.x];
    if (threadIdx.x == 0) {
        st->stage = 0;
        st->level = p.stages[0][1];
        st->done = 0;
        st->converged = 0;
    }
    if (threadIdx.x < 4) info[threadIdx.x] = 0;   // k_coreg_step of iteration 0 always runs and overwrites them
    aff_candidates(st, lc, p, 0, p.stages[0][1]);
    for (int e = threadIdx.x; e < CO_MAXK * p.bins * (p.bins + 1); e += CO_T) hist[e] = 0u;
    if (trace)
        for (int e = threadIdx.x; e < 4 * p.max_iterations; e += CO_T) trace[e] = -1;
}

__global__ void __launch_bounds__(CO_T) k_coreg_step(CoState* st, uint32_t* __restrict__ hist, CoPlan p, int it, float* __restrict__ map_out,
                                                     int64_t* __restrict__ trace, int64_t* __restrict__ info) {
    __shared__ float lc[12];
    __shared__ CoScoreLds sh;
    __shared__ int lg[3];   // done, stage, level: read by every thread before thread 0 writes the state
    if (threadIdx.x == 0) {
        lg[0] = st->done;
        lg[1] = st->stage;
        lg[2] = st->level;
    }
    if (threadIdx.x < 12) lc[threadIdx.x] = st->c[threadIdx.x];
    const int K = st->K, bins = p.bins;   // st->K is written again only after the barriers below
    __syncthreads();
    if (lg[0]) return;
    co_scores(hist, K, bins, sh);         // ends on a barrier
    if (threadIdx.x == 0) {
        const long long* score = (const long long*)sh.score;
        int best = 0;
        for (int k = 1; k < K; ++k)
            if (score[k] > score[best]) best = k;   // strictly larger: the lowest index stays among equal scores
        int g = lg[1], l = lg[2], done = 0, converged = 0;
        if (trace) {
            trace[4 * it + 0] = g;
            trace[4 * it + 1] = l;
            trace[4 * it + 2] = best;
            trace[4 * it + 3] = score[best];
        }
        info[0] = it + 1;
        info[2] = score[best];
        info[3] = g;
        if (best == 0) {
            if (++l > p.stages[g][2]) {
                if (++g == p.n_stages) { done = 1; converged = 1; g = p.n_stages - 1; }
                else l = p.stages[g][1];
            }
        } else {
            const int i = aff_param(p, (best - 1) >> 1);
            lc[i] = aff_move(lc[i], p.step[i], l, (best & 1) ? 1 : -1);
            st->c[i] = lc[i];
        }
        if (it + 1 == p.max_iterations) done = 1;
        info[1] = converged;
        st->stage = lg[1] = g;
        st->level = lg[2] = l;
        st->done = lg[0] = done;
        st->converged = converged;
        float c[12], map[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) c[e] = lc[e];
        aff_state_map(c, p, map);
#pragma unroll
        for (int e = 0; e < 12; ++e) map_out[e] = map[e];
    }
    __syncthreads();
    if (lg[0]) return;   // nothing reads the candidates or the counters after the last iteration
    aff_candidates(st, lc, p, lg[1], lg[2]);
    for (int e = threadIdx.x; e < K * bins * (bins + 1); e += CO_T) hist[e] = 0u;
}

void co_zero(void* p, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, 0, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_coreg: hipMemsetAsync: ") + hipGetErrorString(e));
}

// blocks of k_coreg_hist for a fixed grid counted at `stride`
int co_blocks(int fw, int fh, int fd, int stride) {
    const int nx = (fw + stride - 1) / stride, ny = (fh + stride - 1) / stride, nz = (fd + stride - 1) / stride;
    const int64_t units = (int64_t)((nx + CO_SEG - 1) / CO_SEG) * ny * nz, nb = (units + CO_T - 1) / CO_T;
    return (int)(nb > CO_MAXB ? CO_MAXB : nb < 1 ? 1 : nb);
}

template <bool DEV>
void co_launch_hist(int nb, const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                    const CoMaps& m, int K, int stride, const CoState* st, uint32_t* hist, int impl, hipStream_t s) {
    if (impl == UNET_COREG_IMPL_GLOBAL)
        k_coreg_hist<0, DEV><<<nb, CO_T, 0, s>>>(fixed, fw, fh, fd, moving, mw, mh, md, bins, m, K, stride, st, hist);
    else if (bins <= 16)   // DEFAULT: LDS
        k_coreg_hist<CO_TABLE_16, DEV><<<nb, CO_T, 0, s>>>(fixed, fw, fh, fd, moving, mw, mh, md, bins, m, K, stride, st, hist);
    else
        k_coreg_hist<CO_TABLE_32, DEV><<<nb, CO_T, 0, s>>>(fixed, fw, fh, fd, moving, mw, mh, md, bins, m, K, stride, st, hist);
}

}  // namespace

size_t coreg_scratch_bytes(int bins) { return 256 + co_scratch(nullptr, bins).bytes; }

void launch_coreg_code(const float* image, int64_t voxels, float lo, float scale, int bins, uint8_t* codes, hipStream_t s) {
    const int64_t nb = (voxels + CO_T - 1) / CO_T;
    k_coreg_code<<<(int)(nb > 4 * CO_MAXB ? 4 * CO_MAXB : nb), CO_T, 0, s>>>(image, voxels, lo, scale, bins, codes);
}

// maps: K x 12 host floats, read before this returns
void launch_coreg_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                       const float* maps, int K, int stride, uint32_t* hist, int impl, hipStream_t s) {
    CoMaps m = {};
    for (int e = 0; e < K * 12; ++e) m.v[e] = maps[e];
    co_zero(hist, (size_t)K * bins * (bins + 1) * 4, s);
    co_launch_hist<false>(co_blocks(fw, fh, fd, stride), fixed, fw, fh, fd, moving, mw, mh, md, bins, m, K, stride, nullptr, hist, impl, s);
}

void launch_coreg_score(const uint32_t* hist, int K, int bins, int64_t* scores, hipStream_t s) {
    k_coreg_score<<<1, CO_T, 0, s>>>(hist, K, bins, scores);
}

// init, step, stages: host arrays, read before this returns
void launch_coreg_search(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                         const float* init, const float* step, const int* stages, int n_stages, int max_iterations, float* map_out,
                         int64_t* trace, int64_t* info, int impl, void* scratch, hipStream_t s) {
    const Scratch sc = co_scratch(scratch, bins);
    CoPlan p = {};
    CoMap m0;
    for (int e = 0; e < 12; ++e) { p.step[e] = step[e]; m0.v[e] = init[e]; }
    int finest = stages[0];
    for (int g = 0; g < n_stages; ++g) {
        for (int e = 0; e < 3; ++e) p.stages[g][e] = stages[3 * g + e];
        finest = stages[3 * g] < finest ? stages[3 * g] : finest;
    }
    p.n_stages = n_stages;
    p.max_iterations = max_iterations;
    p.bins = bins;
    p.cx = (float)(fw / 2); p.cy = (float)(fh / 2); p.cz = (float)(fd / 2);
    const int nb = co_blocks(fw, fh, fd, finest);   // one fixed grid: the stage is known on the device only
    const CoMaps none = {};
    k_coreg_init<<<1, CO_T, 0, s>>>(sc.state, sc.hist, m0, p, trace, info);
    for (int it = 0; it < max_iterations; ++it) {
        co_launch_hist<true>(nb, fixed, fw, fh, fd, moving, mw, mh, md, bins, none, 0, 0, sc.state, sc.hist, impl, s);
        k_coreg_step<<<1, CO_T, 0, s>>>(sc.state, sc.hist, p, it, map_out, trace, info);
    }
}

}  // namespace unet
