// The parcellation of a subject (include/unet_register.h): joint tissue histograms under K maps, the pattern search over them, and
// the carrying of an atlas through the map found.
//
//   k_reg_hist   grid-stride over row segments of REG_SEG counted voxels along x; a thread reads its segment's subject tissues once
//                and then, map by map, samples the template at the nearest voxel and merges equal (map, a, b) keys in registers:
//                one add per run, into the block's LDS table (K*T*T <= 6400 counters, flushed with one global add per non-zero
//                counter) or, LDS == false, into global memory.  The K maps are uniform across the block: they are staged in LDS
//                once (from the launch arguments, or, DEV, from the search state together with K and the stride) and read from
//                there at block-uniform addresses.  DEV: returns at once when the state says done
//   k_reg_init   one block: the state of `init`, the candidates of iteration 0, zeroed counters, trace = -1
//   k_reg_step   one block: scores, the winner, level / stage / state, the trace row, info, map_out, the next candidates, and the
//                counters zeroed again.  Returns at once when the state says done.  Ordered after k_reg_hist by the stream
//   k_reg_carry  one thread per subject voxel: the centre, or the mode of the eligible voxels of the 3x3x3 cube; the three counts
//                per tissue gathered in LDS
// Every atomic is an integer add: the results do not depend on the schedule.  Positions are computed per voxel from its integer
// coordinates with contraction off: no incremental sums, so the numpy restatement rounds identically.
//
// Scratch of a search, each part 256-B aligned: the state (RegState), counters uint32[REG_MAXK * T * T].
#include <stdexcept>
#include <string>

#include "../../include/unet_register.h"
#include "affine_search.h"
#include "device_util.h"
#include "tissue_carry.h"

namespace unet {

namespace {

constexpr int REG_T = 256;                            // threads per block
constexpr int REG_MAXB = 1024;                        // grid cap of k_reg_hist and k_reg_carry; they stride over the rest
constexpr int REG_MAXK = UNET_REG_MAX_MAPS;
constexpr int REG_MAXT = UNET_REG_MAX_TISSUES;
constexpr int REG_SEG = 8;                            // counted voxels along x a thread takes at once
constexpr int REG_LDS = REG_MAXK * REG_MAXT * REG_MAXT;   // 6400 counters, 25 KiB

struct RegMaps {   // K maps in the launch arguments
    float v[REG_MAXK * 12];
};
struct RegMap {
    float v[12];
};
struct RegPlan {   // what a search was asked for, in the launch arguments of k_reg_init and k_reg_step
    float step[12];
    int stages[UNET_REG_MAX_STAGES][3];
    int n_stages, max_iterations, T;
    float cx, cy, cz;
};
struct RegState {   // the device state of a search
    float c[12];                  // c0..c8 the matrix, c9..c11 the template position of the subject's centre voxel
    float cand[REG_MAXK * 12];    // the maps of the candidates of the coming iteration
    int K, stride, stage, level, done, converged;
};

size_t reg_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    RegState* state;
    uint32_t* hist;
    size_t bytes;   // from the aligned base
};
Scratch reg_scratch(void* scratch, int T) {
    char* b = (char*)reg_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    size_t o = 0;
    s.state = (RegState*)(b + o); o += reg_align(sizeof(RegState));
    s.hist = (uint32_t*)(b + o);  o += reg_align((size_t)REG_MAXK * T * T * 4);
    s.bytes = o;
    return s;
}

// ---- joint histograms ------------------------------------------------------------------------------------------------------------
template <bool LDS, bool DEV>
__global__ void __launch_bounds__(REG_T) k_reg_hist(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                    const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T, RegMaps maps,
                                                    int K_arg, int stride_arg, const RegState* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ float lm[REG_MAXK * 12];
    __shared__ unsigned lh[LDS ? REG_LDS : 1];
    int K = K_arg, s = stride_arg;
    if constexpr (DEV) {
        if (st->done) return;   // uniform: k_reg_step of the iteration before is complete (stream order)
        K = st->K;
        s = st->stride;
        for (int e = threadIdx.x; e < K * 12; e += REG_T) lm[e] = st->cand[e];
    } else {
        for (int e = threadIdx.x; e < K * 12; e += REG_T) lm[e] = maps.v[e];
    }
    const unsigned TT = (unsigned)(T * T), cells = (unsigned)K * TT;
    if constexpr (LDS)
        for (unsigned e = threadIdx.x; e < cells; e += REG_T) lh[e] = 0u;
    __syncthreads();
    auto add = [&](unsigned key, unsigned n) {
        if constexpr (LDS) atomicAdd(&lh[key], n);
        else atomicAdd(hist + key, n);
    };
    // the counted voxels form an nx x ny x nz grid; a unit is REG_SEG of them along x
    const int nx = (sw + s - 1) / s, ny = (sh + s - 1) / s, nz = (sd + s - 1) / s, nseg = (nx + REG_SEG - 1) / REG_SEG;
    const int64_t units = (int64_t)nseg * ny * nz;
    AffRun run = {0u, 0u};
    for (int64_t u = (int64_t)blockIdx.x * REG_T + threadIdx.x; u < units; u += (int64_t)gridDim.x * REG_T) {
        const unsigned u32 = (unsigned)u;   // units <= voxels < 2^31: 32-bit division
        const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg);
        const int yi = (r % ny) * s, zi = (r / ny) * s, x0 = seg * REG_SEG, n = min(REG_SEG, nx - x0);
        const int64_t row = ((int64_t)zi * sh + yi) * sw;
        unsigned a[REG_SEG];
#pragma unroll
        for (int j = 0; j < REG_SEG; ++j) a[j] = j < n ? reg_tissue(subject, sbytes, row + (int64_t)(x0 + j) * s, T) * (unsigned)T : 0u;
        for (int k = 0; k < K; ++k) {
            const float* m = lm + k * 12;          // the same address in every lane: an LDS broadcast
            const unsigned kbase = (unsigned)k * TT;
#pragma unroll
            for (int j = 0; j < REG_SEG; ++j) {
                if (j < n) {
                    const AffPos p = aff_locate(m, (x0 + j) * s, yi, zi, tw, th, td);
                    unsigned b = 0u;
                    if (p.in) b = reg_tissue(tmpl, tbytes, ((int64_t)(int)floorf(p.qz) * th + (int)floorf(p.qy)) * tw + (int)floorf(p.qx), T);
                    run.push(kbase + a[j] + b, add);
                }
            }
        }
    }
    run.close(add);
    if constexpr (LDS) {
        __syncthreads();
        for (unsigned e = threadIdx.x; e < cells; e += REG_T)
            if (const unsigned c = lh[e]) atomicAdd(hist + e, c);
    }
}

// ---- the search ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(REG_T) k_reg_init(RegState* st, uint32_t* __restrict__ hist, RegMap init, RegPlan p,
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
    if (threadIdx.x < 4) info[threadIdx.x] = 0;   // k_reg_step of iteration 0 always runs and overwrites them
    aff_candidates(st, lc, p, 0, p.stages[0][1]);
    for (int e = threadIdx.x; e < REG_MAXK * p.T * p.T; e += REG_T) hist[e] = 0u;
    if (trace)
        for (int e = threadIdx.x; e < 4 * p.max_iterations; e += REG_T) trace[e] = -1;
}

__global__ void __launch_bounds__(REG_T) k_reg_step(RegState* st, uint32_t* __restrict__ hist, RegPlan p, int it, float* __restrict__ map_out,
                                                    int64_t* __restrict__ trace, int64_t* __restrict__ info) {
    __shared__ float lc[12];
    __shared__ long long score[REG_MAXK];
    __shared__ int lg[3];   // done, stage, level: read by every thread before thread 0 writes the state
    if (threadIdx.x == 0) {
        lg[0] = st->done;
        lg[1] = st->stage;
        lg[2] = st->level;
    }
    if (threadIdx.x < 12) lc[threadIdx.x] = st->c[threadIdx.x];
    const int K = st->K, T = p.T;   // st->K is written again only after the barriers below
    __syncthreads();
    if (lg[0]) return;
    if ((int)threadIdx.x < K) {     // agree - disagree of candidate k
        const uint32_t* h = hist + (size_t)threadIdx.x * T * T;
        long long sc = 0;
        for (int a = 0; a < T; ++a)
            for (int b = 0; b < T; ++b) {
                const long long n = (long long)h[a * T + b];
                sc += a == b ? (a ? n : 0) : -n;
            }
        score[threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
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
    for (int e = threadIdx.x; e < K * T * T; e += REG_T) hist[e] = 0u;
}

// ---- carry -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(REG_T) k_reg_carry(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                     const void* __restrict__ tmpl, int tbytes, int tw, int th, int td,
                                                     const uint16_t* __restrict__ atlas, int T, RegMap map, uint16_t* __restrict__ out,
                                                     uint32_t* __restrict__ counts) {
    __shared__ unsigned lc[3 * REG_MAXT];
    __shared__ float lm[12];
    if (threadIdx.x < 3 * REG_MAXT) lc[threadIdx.x] = 0u;
    if (threadIdx.x < 12) lm[threadIdx.x] = map.v[threadIdx.x];
    __syncthreads();
    const int S = sw * sh * sd;
    for (int64_t i64 = (int64_t)blockIdx.x * REG_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * REG_T) {
        const int i = (int)i64;
        const unsigned a = reg_tissue(subject, sbytes, i, T);
        if (a == 0u) {
            out[i] = 0;
            continue;
        }
        const int x = i % sw, y = (i / sw) % sh, z = i / (sw * sh);
        const AffPos p = aff_locate(lm, x, y, z, tw, th, td);
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

void reg_zero(void* p, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, 0, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_reg: hipMemsetAsync: ") + hipGetErrorString(e));
}

// blocks of k_reg_hist for a subject counted at `stride`
int reg_blocks(int sw, int sh, int sd, int stride) {
    const int nx = (sw + stride - 1) / stride, ny = (sh + stride - 1) / stride, nz = (sd + stride - 1) / stride;
    const int64_t units = (int64_t)((nx + REG_SEG - 1) / REG_SEG) * ny * nz, nb = (units + REG_T - 1) / REG_T;
    return (int)(nb > REG_MAXB ? REG_MAXB : nb < 1 ? 1 : nb);
}

}  // namespace

size_t reg_scratch_bytes(int T) { return 256 + reg_scratch(nullptr, T).bytes; }

// maps: K x 12 host floats, read before this returns
void launch_reg_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                     const float* maps, int K, int stride, uint32_t* hist, int impl, hipStream_t s) {
    RegMaps m = {};
    for (int e = 0; e < K * 12; ++e) m.v[e] = maps[e];
    reg_zero(hist, (size_t)K * T * T * 4, s);
    const int nb = reg_blocks(sw, sh, sd, stride);
    if (impl != UNET_REG_IMPL_GLOBAL)   // DEFAULT: LDS
        k_reg_hist<true, false><<<nb, REG_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T, m, K, stride, nullptr, hist);
    else
        k_reg_hist<false, false><<<nb, REG_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T, m, K, stride, nullptr, hist);
}

// init, step, stages: host arrays, read before this returns
void launch_reg_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                       const float* init, const float* step, const int* stages, int n_stages, int max_iterations, float* map_out,
                       int64_t* trace, int64_t* info, int impl, void* scratch, hipStream_t s) {
    const Scratch sc = reg_scratch(scratch, T);
    RegPlan p = {};
    RegMap m0;
    for (int e = 0; e < 12; ++e) { p.step[e] = step[e]; m0.v[e] = init[e]; }
    int finest = stages[0];
    for (int g = 0; g < n_stages; ++g) {
        for (int e = 0; e < 3; ++e) p.stages[g][e] = stages[3 * g + e];
        finest = stages[3 * g] < finest ? stages[3 * g] : finest;
    }
    p.n_stages = n_stages;
    p.max_iterations = max_iterations;
    p.T = T;
    p.cx = (float)(sw / 2); p.cy = (float)(sh / 2); p.cz = (float)(sd / 2);
    const int nb = reg_blocks(sw, sh, sd, finest);   // one fixed grid: the stage is known on the device only
    const RegMaps none = {};
    k_reg_init<<<1, REG_T, 0, s>>>(sc.state, sc.hist, m0, p, trace, info);
    for (int it = 0; it < max_iterations; ++it) {
        if (impl != UNET_REG_IMPL_GLOBAL)
            k_reg_hist<true, true><<<nb, REG_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T, none, 0, 0, sc.state, sc.hist);
        else
            k_reg_hist<false, true><<<nb, REG_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T, none, 0, 0, sc.state, sc.hist);
        k_reg_step<<<1, REG_T, 0, s>>>(sc.state, sc.hist, p, it, map_out, trace, info);
    }
}

void launch_reg_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                      const uint16_t* atlas, int T, const float* map, uint16_t* out, uint32_t* counts, hipStream_t s) {
    RegMap m;
    for (int e = 0; e < 12; ++e) m.v[e] = map[e];
    if (counts) reg_zero(counts, (size_t)3 * T * 4, s);
    const int64_t S = (int64_t)sw * sh * sd, nb = (S + REG_T - 1) / REG_T;
    k_reg_carry<<<(int)(nb > 4 * REG_MAXB ? 4 * REG_MAXB : nb), REG_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, atlas, T, m,
                                                                            out, counts);
}

}  // namespace unet
