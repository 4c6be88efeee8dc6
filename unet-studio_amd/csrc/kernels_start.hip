// The starts of a registration (include/unet_start.h): the moments of a foreground, the choice among ranked starts, and up to four
// pattern searches over the same two tissue maps advancing in lock-step.
//
//   k_start_moments  grid-stride over the voxels; a thread keeps its ten 64-bit sums in registers, a wave reduces them by lane
//                    shuffles, the block's waves through LDS, and the block's first ten threads add one 64-bit integer each
//   k_start_pick     one block: thread k scores table k (agree - disagree, int64); thread 0 takes the n best, the lowest index among
//                    equal scores, and puts `always` in the last place when it is missing; then the chosen maps are copied
//   k_start_init     one block per state: the state of inits[s] (read from the DEVICE), the candidates of iteration 0, zeroed
//                    counters, trace = -1: what the register module's init kernel does from its launch arguments
//   k_start_hist     the register module's histogram pass for every live state in turn: a block stages the state's K maps and its
//                    stride, zeroes its LDS table (K*T*T <= 6400 counters), counts its share of the subject at that stride, flushes
//                    one global add per non-zero counter into the state's own counters, and only then turns to the next state.
//                    Only the block's own barriers separate the states; a state that is done is skipped (block-uniform)
//   k_start_step     one block per state: scores, the winner, level / stage / state, the trace row, info, the map, the next
//                    candidates, the state's counters zeroed again.  Returns at once when the state says done
//   k_start_close    one block: best = the greatest (converged, stage, score), the lowest index among equal keys; its map copied
// Every atomic is an integer add: the results do not depend on the schedule.  The arithmetic of a state (affine_search.h) is the
// register module's, inlined here as there, with contraction off.
//
// Scratch, each part 256-B aligned: n states (StartState), n x uint32[START_MAXK * T * T] counters, and, for IMPL_SEQUENTIAL, n
// scratches of the register module's search.
#include <stdexcept>
#include <string>

#include "../../include/unet_start.h"
#include "affine_search.h"
#include "kernels.h"

namespace unet {

namespace {

constexpr int START_T = 256;                          // threads per block
constexpr int START_WAVE = 64;
constexpr int START_MAXB = 1024;                      // grid cap of k_start_moments and k_start_hist; they stride over the rest
constexpr int START_MAXK = 25;                        // candidates of an iteration: 1 + 2 * 12
constexpr int START_MAXT = 16;
constexpr int START_MAXG = 4;                         // stages
constexpr int START_SEG = 8;                          // counted voxels along x a thread takes at once
constexpr int START_LDS = START_MAXK * START_MAXT * START_MAXT;   // 6400 counters, 25 KiB
constexpr int START_SUMS = 10;

struct StartPlan {   // what the searches were asked for, in the launch arguments of k_start_init and k_start_step
    float step[12];
    int stages[START_MAXG][3];
    int n_stages, max_iterations, T;
    float cx, cy, cz;
};
struct alignas(256) StartState {   // the device state of one search
    float c[12];                   // c0..c8 the matrix, c9..c11 the template position of the subject's centre voxel
    float cand[START_MAXK * 12];   // the maps of the candidates of the coming iteration
    int K, stride, stage, level, done, converged;
};

size_t start_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    StartState* state;   // [n]
    uint32_t* hist;      // [n], hist_stride entries apart
    size_t hist_stride;
    char* seq;           // [n], seq_stride bytes apart
    size_t seq_stride;
    size_t bytes;        // from the aligned base
};
Scratch start_scratch(void* scratch, int T, int n) {
    char* b = (char*)start_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    size_t o = 0;
    s.state = (StartState*)(b + o); o += (size_t)n * sizeof(StartState);
    s.hist_stride = start_align((size_t)START_MAXK * T * T * 4) / 4;
    s.hist = (uint32_t*)(b + o);    o += (size_t)n * s.hist_stride * 4;
    s.seq_stride = start_align(reg_scratch_bytes(T));
    s.seq = b + o;                  o += (size_t)n * s.seq_stride;
    s.bytes = o;
    return s;
}

// a value as read: uint8 or uint16 at any alignment
__device__ __forceinline__ unsigned start_value(const void* __restrict__ p, int bytes, int64_t i) {
    return bytes == 1 ? (unsigned)((const uint8_t*)p)[i]
                      : (unsigned)((const uint8_t*)p)[2 * i] | ((unsigned)((const uint8_t*)p)[2 * i + 1] << 8);
}
// a tissue: a value >= T reads as 0
__device__ __forceinline__ unsigned start_tissue(const void* __restrict__ p, int bytes, int64_t i, int T) {
    const unsigned v = start_value(p, bytes, i);
    return v >= (unsigned)T ? 0u : v;
}

// ---- moments ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(START_T) k_start_moments(const void* __restrict__ vol, int vbytes, int w, int h, int d, unsigned lo,
                                                           unsigned hi, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[START_T / START_WAVE][START_SUMS];
    unsigned long long a[START_SUMS];
#pragma unroll
    for (int e = 0; e < START_SUMS; ++e) a[e] = 0ull;
    const unsigned S = (unsigned)(w * h * d);   // < 2^31
    for (int64_t i64 = (int64_t)blockIdx.x * START_T + threadIdx.x; i64 < (int64_t)S; i64 += (int64_t)gridDim.x * START_T) {
        const unsigned i = (unsigned)i64, v = start_value(vol, vbytes, i64);
        if (v < lo || v > hi) continue;
        const unsigned r = i / (unsigned)w, x = i - r * (unsigned)w, z = r / (unsigned)h, y = r - z * (unsigned)h;   // each <= 65535
        a[0] += 1ull; a[1] += x; a[2] += y; a[3] += z;
        a[4] += x * x; a[5] += y * y; a[6] += z * z;             // <= 65535^2 < 2^32
        a[7] += x * y; a[8] += x * z; a[9] += y * z;
    }
#pragma unroll
    for (int e = 0; e < START_SUMS; ++e)
        for (int off = START_WAVE / 2; off > 0; off >>= 1) a[e] += __shfl_down(a[e], off, START_WAVE);
    const int lane = threadIdx.x % START_WAVE, wave = threadIdx.x / START_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < START_SUMS; ++e) part[wave][e] = a[e];
    }
    __syncthreads();
    if (threadIdx.x < START_SUMS) {
        unsigned long long t = 0ull;
        for (int k = 0; k < START_T / START_WAVE; ++k) t += part[k][threadIdx.x];
        if (t) atomicAdd(sums + threadIdx.x, t);
    }
}

// ---- pick ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long start_score(const uint32_t* __restrict__ h, int T) {   // agree - disagree of one table
    long long sc = 0;
    for (int a = 0; a < T; ++a)
        for (int b = 0; b < T; ++b) {
            const long long n = (long long)h[a * T + b];
            sc += a == b ? (a ? n : 0) : -n;
        }
    return sc;
}

__global__ void __launch_bounds__(128) k_start_pick(const uint32_t* __restrict__ hist, int S, int T, const float* __restrict__ maps, int n,
                                                    int always, long long* __restrict__ scores, float* __restrict__ inits,
                                                    int* __restrict__ picked) {
    __shared__ long long sc[UNET_START_MAX_STARTS];
    __shared__ int lp[UNET_START_MAX_STATES];
    if ((int)threadIdx.x < S) scores[threadIdx.x] = sc[threadIdx.x] = start_score(hist + (size_t)threadIdx.x * T * T, T);
    __syncthreads();
    if (threadIdx.x == 0) {
        bool has = always < 0;
        for (int j = 0; j < n; ++j) {
            int best = -1;
            for (int k = 0; k < S; ++k) {
                bool taken = false;
                for (int i = 0; i < j; ++i) taken |= lp[i] == k;
                if (!taken && (best < 0 || sc[k] > sc[best])) best = k;   // strictly larger: the lowest index among equal scores
            }
            lp[j] = best;
            has |= best == always;
        }
        if (!has) lp[n - 1] = always;
        for (int j = 0; j < n; ++j) picked[j] = lp[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < n * 12) inits[threadIdx.x] = maps[lp[threadIdx.x / 12] * 12 + threadIdx.x % 12];
}

// ---- the searches ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(START_T) k_start_init(StartState* states, uint32_t* __restrict__ hists, size_t hist_stride,
                                                        const float* __restrict__ inits, StartPlan p, int64_t* __restrict__ traces,
                                                        int64_t* __restrict__ infos) {
#pragma clang fp contract(off)
    __shared__ float lc[12];
    __shared__ float li[12];
    const int s = blockIdx.x;
    StartState* st = states + s;
    uint32_t* hist = hists + (size_t)s * hist_stride;
    int64_t* info = infos + 4 * s;
    if (threadIdx.x < 12) li[threadIdx.x] = inits[s * 12 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 9) lc[threadIdx.x] = li[threadIdx.x];
    if (threadIdx.x < 3) {
        const int r = threadIdx.x;
        lc[9 + r] = ((li[3 * r] * p.cx + li[3 * r + 1] * p.cy) + li[3 * r + 2] * p.cz) + li[9 + r];
    }
    __syncthreads();
    if (threadIdx.x < 12) st->c[threadIdx.x] = lc[threadIdx.x];
    if (threadIdx.x == 0) {
        st->stage = 0;
        st->level = p.stages[0][1];
        st->done = 0;
        st->converged = 0;
    }
    if (threadIdx.x < 4) info[threadIdx.x] = 0;   // k_start_step of iteration 0 always runs and overwrites them
    aff_candidates(st, lc, p, 0, p.stages[0][1]);
    for (int e = threadIdx.x; e < START_MAXK * p.T * p.T; e += START_T) hist[e] = 0u;
    if (traces) {
        int64_t* trace = traces + (size_t)s * 4 * p.max_iterations;
        for (int e = threadIdx.x; e < 4 * p.max_iterations; e += START_T) trace[e] = -1;
    }
}

__global__ void __launch_bounds__(START_T) k_start_hist(const void* __restrict__ subject, int sbytes, int sw, int sh, int sd,
                                                        const void* __restrict__ tmpl, int tbytes, int tw, int th, int td, int T,
                                                        const StartState* __restrict__ states, int n, uint32_t* __restrict__ hists,
                                                        size_t hist_stride) {
    __shared__ float lm[START_MAXK * 12];
    __shared__ unsigned lh[START_LDS];
    const unsigned TT = (unsigned)(T * T);
    auto add = [&](unsigned key, unsigned cnt) { atomicAdd(&lh[key], cnt); };
    for (int si = 0; si < n; ++si) {
        const StartState* st = states + si;
        if (st->done) continue;   // uniform: k_start_step of the iteration before is complete (stream order)
        const int K = st->K, s = st->stride;
        const unsigned cells = (unsigned)K * TT;
        for (int e = threadIdx.x; e < K * 12; e += START_T) lm[e] = st->cand[e];
        for (unsigned e = threadIdx.x; e < cells; e += START_T) lh[e] = 0u;
        __syncthreads();
        // the counted voxels form an nx x ny x nz grid; a unit is START_SEG of them along x
        const int nx = (sw + s - 1) / s, ny = (sh + s - 1) / s, nz = (sd + s - 1) / s, nseg = (nx + START_SEG - 1) / START_SEG;
        const int64_t units = (int64_t)nseg * ny * nz;
        AffRun run = {0u, 0u};
        for (int64_t u = (int64_t)blockIdx.x * START_T + threadIdx.x; u < units; u += (int64_t)gridDim.x * START_T) {
            const unsigned u32 = (unsigned)u;   // units <= voxels < 2^31: 32-bit division
            const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg);
            const int yi = (r % ny) * s, zi = (r / ny) * s, x0 = seg * START_SEG, cnt = min(START_SEG, nx - x0);
            const int64_t row = ((int64_t)zi * sh + yi) * sw;
            unsigned a[START_SEG];
#pragma unroll
            for (int j = 0; j < START_SEG; ++j)
                a[j] = j < cnt ? start_tissue(subject, sbytes, row + (int64_t)(x0 + j) * s, T) * (unsigned)T : 0u;
            for (int k = 0; k < K; ++k) {
                const float* m = lm + k * 12;          // the same address in every lane: an LDS broadcast
                const unsigned kbase = (unsigned)k * TT;
#pragma unroll
                for (int j = 0; j < START_SEG; ++j) {
                    if (j < cnt) {
                        const AffPos p = aff_locate(m, (x0 + j) * s, yi, zi, tw, th, td);
                        unsigned b = 0u;
                        if (p.in)
                            b = start_tissue(tmpl, tbytes, ((int64_t)(int)floorf(p.qz) * th + (int)floorf(p.qy)) * tw + (int)floorf(p.qx), T);
                        run.push(kbase + a[j] + b, add);
                    }
                }
            }
        }
        run.close(add);
        __syncthreads();
        uint32_t* hist = hists + (size_t)si * hist_stride;
        for (unsigned e = threadIdx.x; e < cells; e += START_T)
            if (const unsigned c = lh[e]) atomicAdd(hist + e, c);
        __syncthreads();   // the table and the maps are the next state's from here on
    }
}

__global__ void __launch_bounds__(START_T) k_start_step(StartState* states, uint32_t* __restrict__ hists, size_t hist_stride, StartPlan p,
                                                        int it, float* __restrict__ maps_out, int64_t* __restrict__ traces,
                                                        int64_t* __restrict__ infos) {
    __shared__ float lc[12];
    __shared__ long long score[START_MAXK];
    __shared__ int lg[3];   // done, stage, level: read by every thread before thread 0 writes the state
    const int s = blockIdx.x;
    StartState* st = states + s;
    uint32_t* hist = hists + (size_t)s * hist_stride;
    int64_t* info = infos + 4 * s;
    int64_t* trace = traces ? traces + (size_t)s * 4 * p.max_iterations : nullptr;
    if (threadIdx.x == 0) {
        lg[0] = st->done;
        lg[1] = st->stage;
        lg[2] = st->level;
    }
    if (threadIdx.x < 12) lc[threadIdx.x] = st->c[threadIdx.x];
    const int K = st->K, T = p.T;   // st->K is written again only after the barriers below
    __syncthreads();
    if (lg[0]) return;
    if ((int)threadIdx.x < K) score[threadIdx.x] = start_score(hist + (size_t)threadIdx.x * T * T, T);
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
        for (int e = 0; e < 12; ++e) maps_out[s * 12 + e] = map[e];
    }
    __syncthreads();
    if (lg[0]) return;   // nothing reads the candidates or the counters after the last iteration
    aff_candidates(st, lc, p, lg[1], lg[2]);
    for (int e = threadIdx.x; e < K * T * T; e += START_T) hist[e] = 0u;
}

__global__ void __launch_bounds__(START_WAVE) k_start_close(const int64_t* __restrict__ infos, const float* __restrict__ maps_out, int n,
                                                            int* __restrict__ best, float* __restrict__ best_map) {
    __shared__ int lb;
    if (threadIdx.x == 0) {
        int b = 0;
        for (int s = 1; s < n; ++s) {   // (converged, stage, score), strictly greater: the lowest index among equal keys
            const int64_t* x = infos + 4 * s;
            const int64_t* y = infos + 4 * b;
            if (x[1] != y[1] ? x[1] > y[1] : x[3] != y[3] ? x[3] > y[3] : x[2] > y[2]) b = s;
        }
        lb = b;
        *best = b;
    }
    __syncthreads();
    if (threadIdx.x < 12) best_map[threadIdx.x] = maps_out[lb * 12 + threadIdx.x];
}

}  // namespace

size_t start_scratch_bytes(int T, int n) { return 256 + start_scratch(nullptr, T, n).bytes; }

void* start_seq_scratch(void* scratch, int T, int n, int s) {
    const Scratch sc = start_scratch(scratch, T, n);
    return sc.seq + (size_t)s * sc.seq_stride;
}
size_t start_seq_scratch_bytes(int T) { return start_align(reg_scratch_bytes(T)); }

void launch_start_moments(const void* vol, int vbytes, int w, int h, int d, int lo, int hi, uint64_t* sums, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(sums, 0, START_SUMS * sizeof(uint64_t), s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_start: hipMemsetAsync: ") + hipGetErrorString(e));
    if (lo > hi) return;   // an empty range
    const int64_t S = (int64_t)w * h * d, nb = (S + START_T - 1) / START_T;
    k_start_moments<<<(int)(nb > START_MAXB ? START_MAXB : nb), START_T, 0, s>>>(vol, vbytes, w, h, d, (unsigned)lo, (unsigned)hi,
                                                                               (unsigned long long*)sums);
}

void launch_start_pick(const uint32_t* hist, int S, int T, const float* maps, int n, int always, int64_t* scores, float* inits,
                       int32_t* picked, hipStream_t s) {
    k_start_pick<<<1, 128, 0, s>>>(hist, S, T, maps, n, always, (long long*)scores, inits, picked);
}

void launch_start_close(const int64_t* info, const float* maps_out, int n, int32_t* best, float* best_map, hipStream_t s) {
    k_start_close<<<1, START_WAVE, 0, s>>>(info, maps_out, n, best, best_map);
}

// step, stages: host arrays, read before this returns; inits: device
void launch_start_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td, int T,
                         const float* inits, int n, const float* step, const int* stages, int n_stages, int max_iterations, float* maps_out,
                         int64_t* trace, int64_t* info, int32_t* best, float* best_map, void* scratch, hipStream_t s) {
    const Scratch sc = start_scratch(scratch, T, n);
    StartPlan p = {};
    for (int e = 0; e < 12; ++e) p.step[e] = step[e];
    int finest = stages[0];
    for (int g = 0; g < n_stages; ++g) {
        for (int e = 0; e < 3; ++e) p.stages[g][e] = stages[3 * g + e];
        finest = stages[3 * g] < finest ? stages[3 * g] : finest;
    }
    p.n_stages = n_stages;
    p.max_iterations = max_iterations;
    p.T = T;
    p.cx = (float)(sw / 2); p.cy = (float)(sh / 2); p.cz = (float)(sd / 2);
    // one fixed grid, that of the finest stride: the stages are known on the device only
    const int nx = (sw + finest - 1) / finest, ny = (sh + finest - 1) / finest, nz = (sd + finest - 1) / finest;
    const int64_t units = (int64_t)((nx + START_SEG - 1) / START_SEG) * ny * nz, nbu = (units + START_T - 1) / START_T;
    const int nb = (int)(nbu > START_MAXB ? START_MAXB : nbu < 1 ? 1 : nbu);
    k_start_init<<<n, START_T, 0, s>>>(sc.state, sc.hist, sc.hist_stride, inits, p, trace, info);
    for (int it = 0; it < max_iterations; ++it) {
        k_start_hist<<<nb, START_T, 0, s>>>(subject, sbytes, sw, sh, sd, tmpl, tbytes, tw, th, td, T, sc.state, n, sc.hist, sc.hist_stride);
        k_start_step<<<n, START_T, 0, s>>>(sc.state, sc.hist, sc.hist_stride, p, it, maps_out, trace, info);
    }
    launch_start_close(info, maps_out, n, best, best_map, s);
}

}  // namespace unet
