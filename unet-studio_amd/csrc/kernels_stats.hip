// The per-region intensity statistics (include/unet_stats.h): per label the counts, the integer moments and the exact extremes of a
// scalar volume from one pass over a label map and the volume, a 256-bin histogram per label from one pass, and up to eight
// quantiles per label from two passes (a two-level radix select: no sort, nothing stored per voxel).
//
//   k_stats_init     the running tables in the scratch: counters 0, the minimum key 0xFFFFFFFF, the maximum key 0
//   k_stats_moments  grid-stride over units of ST_SEG voxels; a thread reads its unit (the image as two 16-byte vectors, the labels as
//                    one vector, where alignment allows), codes each voxel and sums in registers while the label stays the same:
//                    one update per run of equal labels, which merges more than equal (label, code) pairs would.  LDS: a row below
//                    UNET_STATS_LDS_ROWS is updated in the block's LDS table (six 64-bit sums, two 32-bit keys: 56 B a row, 56 KiB),
//                    flushed with one global update per touched row; other rows, and every row with LDS == false, go to the scratch
//   k_stats_widen    the running moments -> int64 rows, every entry stored.  Coding is monotone, so min q and max q are the codes of
//                    the minimum and the maximum key: they are formed here, not gathered
//   k_stats_count    both histogram passes.  An update is (counter row, bin) += n: pass A (FINE == false) row = label, bin = q >> 8;
//                    pass B row = label * Q + j for the j-th distinct chosen coarse bin of the label when q >> 8 equals it, bin =
//                    q & 255.  A thread merges consecutive voxels with the same (row, bin); voxels that send nothing (NaN, no chosen
//                    bin) do not end a run.  LDS: a block keeps UNET_STATS_LDS_SLOTS slots of UNET_STATS_SLOT_BINS consecutive 32-bit
//                    counters of one row behind a (row, bin / UNET_STATS_SLOT_BINS) -> slot cache (open addressing,
//                    UNET_STATS_LDS_PROBES probes, slots claimed with a compare-and-swap and never released): a row costs the
//                    slots its values occupy, one for a mask, sixteen for an image that fills every bin.  An update that finds no
//                    slot goes to the scratch.  One global update per touched (slot, bin) at the end
//   k_stats_select   one thread per label: n and the ranks from the coarse histogram, per quantile the coarse bin holding the rank and
//                    the rank left inside it; the distinct chosen bins of the label (two quantiles in one bin share one fine row)
//   k_stats_pick     one thread per (label, quantile): the fine bin holding the rank left -> the code, -1 for an empty row
//   k_stats_hist_widen  the coarse counters -> int64 rows
// Every atomic is an integer add, minimum or maximum: the results do not depend on the schedule.
//
// Scratch, each part 256-B aligned.  Moments: sums uint64[(L + 1) * 6], keys uint32[(L + 1) * 2].  Histograms, in the same bytes:
// coarse uint32[(L + 1) * 256]; with Q quantiles also fine uint32[(L + 1) * Q * 256] and four int32[(L + 1) * Q]: the distinct bins
// of a label, and per quantile its fine row, the rank left and its coarse bin.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/unet_stats.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int ST_T = 512;                             // threads per block
constexpr int ST_MAXB = 512;                          // grid cap; the kernels stride over the rest
constexpr int ST_SEG = UNET_STATS_UNIT;               // consecutive voxels a thread takes at once: a unit
constexpr int ST_CHUNK = 8;                           // units a lane takes from one stretch of 64 * ST_CHUNK consecutive units
constexpr int ST_ROWS = UNET_STATS_LDS_ROWS;
constexpr int ST_SLOTS = UNET_STATS_LDS_SLOTS;
constexpr int ST_SBINS = UNET_STATS_SLOT_BINS;       // counters a slot holds
constexpr int ST_PROBES = UNET_STATS_LDS_PROBES;
constexpr int ST_BINS = UNET_STATS_HIST_BINS;
constexpr int ST_MAXQ = UNET_STATS_MAX_QUANTILES;
constexpr unsigned ST_NONE = 0xFFFFFFFFu;             // no counter row / an empty slot
static_assert(ST_SEG == 8, "a unit is two float4 and one label vector");
static_assert(ST_T % 64 == 0, "whole waves");
static_assert(ST_CHUNK * 64 == UNET_STATS_WAVE_UNITS, "the header states a wave's stretch");
static_assert(ST_MAXB * (ST_T / 64) * ST_CHUNK * 64 == UNET_STATS_GRID_UNITS, "the header states the grid's stride");
static_assert(ST_ROWS * (6 * 8 + 2 * 4) <= 64 * 1024, "the LDS table of a block");
static_assert(ST_SLOTS * (ST_SBINS * 4 + 4) <= 64 * 1024 && ST_SLOTS == 512, "the slot cache of a block; the hash keeps 9 bits");
static_assert(ST_SBINS == 16 && ST_BINS % ST_SBINS == 0, "a slot's key is (row * 256 + bin) / 16");
static_assert(ST_BINS == 256 && UNET_STATS_CODES == ST_BINS * ST_BINS, "two radix levels of 8 bits");

typedef unsigned long long u64;

size_t st_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    u64* sum;          // moments: (L + 1) x {n, nan, below, above, sum q, sum q^2}
    unsigned* key;     // moments: (L + 1) x {min key, max key}
    unsigned* coarse;  // (L + 1) x 256, in the first part
    unsigned* fine;    // (L + 1) x Q x 256
    int* dbin;         // (L + 1) x Q: the distinct chosen coarse bins of a label, -1 behind them
    int* own;          // (L + 1) x Q: a quantile's fine row among them
    unsigned* rem;     // (L + 1) x Q: the rank left inside the coarse bin
    int* kbin;         // (L + 1) x Q: a quantile's coarse bin, -1 for an empty row
    size_t bytes;      // from the aligned base
};
Scratch st_scratch(void* scratch, int L, int Q) {
    char* b = (char*)st_align((size_t)(uintptr_t)scratch);    // any scratch alignment: 256 B of slack
    const size_t R = (size_t)L + 1, Rh = R < (size_t)UNET_STATS_MAX_QUANTILE_LABELS + 1 ? R : (size_t)UNET_STATS_MAX_QUANTILE_LABELS + 1;
    Scratch s;
    size_t o = 0;
    s.sum = (u64*)(b + o);       o += st_align(R * 6 * 8);
    s.key = (unsigned*)(b + o);  o += st_align(R * 2 * 4);
    const size_t mom = o;
    o = 0;
    s.coarse = (unsigned*)(b + o);  o += st_align(Rh * ST_BINS * 4);
    s.fine = (unsigned*)(b + o);    o += st_align(Rh * Q * ST_BINS * 4);
    s.dbin = (int*)(b + o);         o += st_align(Rh * Q * 4);
    s.own = (int*)(b + o);          o += st_align(Rh * Q * 4);
    s.rem = (unsigned*)(b + o);     o += st_align(Rh * Q * 4);
    s.kbin = (int*)(b + o);         o += st_align(Rh * Q * 4);
    s.bytes = o > mom ? o : mom;
    return s;
}

// ---- a unit as read ----------------------------------------------------------------------------------------------------------------
// the labels of a unit: uint8 or uint16 at any alignment (one vector when `vec`: the base is aligned to a unit and the unit is
// whole); a value above L reads as 0; no map: one region
__device__ __forceinline__ void st_labels(const void* __restrict__ p, int bytes, bool vec, int64_t i0, int n, unsigned L, unsigned (&l)[ST_SEG]) {
    if (!p) {
#pragma unroll
        for (int j = 0; j < ST_SEG; ++j) l[j] = 0u;
        return;
    }
    const uint8_t* b = (const uint8_t*)p;
    if (vec && n == ST_SEG) {
        if (bytes == 1) {
            const uint2 w = *(const uint2*)(b + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                l[j] = (w.x >> (8 * j)) & 255u;
                l[4 + j] = (w.y >> (8 * j)) & 255u;
            }
        } else {
            const uint4 w = *(const uint4*)(b + 2 * i0);
            l[0] = w.x & 0xFFFFu; l[1] = w.x >> 16; l[2] = w.y & 0xFFFFu; l[3] = w.y >> 16;
            l[4] = w.z & 0xFFFFu; l[5] = w.z >> 16; l[6] = w.w & 0xFFFFu; l[7] = w.w >> 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < ST_SEG; ++j) {
            const int64_t i = i0 + j;
            l[j] = j >= n ? 0u : bytes == 1 ? (unsigned)b[i] : (unsigned)b[2 * i] | ((unsigned)b[2 * i + 1] << 8);
        }
    }
#pragma unroll
    for (int j = 0; j < ST_SEG; ++j) l[j] = l[j] > L ? 0u : l[j];
}

__device__ __forceinline__ void st_values(const float* __restrict__ image, bool vec, int64_t i0, int n, float (&v)[ST_SEG]) {
    if (vec && n == ST_SEG) {
        const float4 a = *(const float4*)(image + i0), b = *(const float4*)(image + i0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < ST_SEG; ++j) v[j] = j < n ? image[i0 + j] : 0.f;
    }
}

// the code of a value that is not NaN: one subtraction, one multiplication, each rounded to nearest, never fused
__device__ __forceinline__ unsigned st_code(float v, float lo, float scale) {
    const float t = __fmul_rn(__fsub_rn(v, lo), scale);
    return t < 0.f ? 0u : t >= 65535.0f ? 65535u : (unsigned)(int)t;
}
__device__ __forceinline__ unsigned st_key(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float st_unkey(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// min / max into a block's LDS table, sent only when the table does not hold it yet (a volatile read: other threads write it; the
// entry only ever moves towards the extreme, so a stale read costs an update, never a result).  Global entries are always sent
template <bool CHECK> __device__ __forceinline__ void st_min(unsigned* p, unsigned v) {
    if (!CHECK || v < *(volatile unsigned*)p) atomicMin(p, v);
}
template <bool CHECK> __device__ __forceinline__ void st_max(unsigned* p, unsigned v) {
    if (!CHECK || v > *(volatile unsigned*)p) atomicMax(p, v);
}

// words of zeros, then (moments only) the keys' start values
__global__ void __launch_bounds__(ST_T) k_stats_init(unsigned* __restrict__ zero, int64_t words, unsigned* __restrict__ key, int rows) {
    const int64_t step = (int64_t)gridDim.x * ST_T, t = (int64_t)blockIdx.x * ST_T + threadIdx.x;
    for (int64_t i = t; i < words; i += step) zero[i] = 0u;
    if (key)
        for (int64_t i = t; i < (int64_t)rows * 2; i += step) key[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}

// The units of a wave: a wave takes ST_CHUNK * 64 consecutive units at a time and lane i the units i, 64 + i, 128 + i, ... of them, so
// that a wave-instruction reads 64 consecutive units and a lane's successive units lie close together: in a solid map they mostly
// read the same label and stay one open run in the lane's registers.  A block's waves take adjacent stretches.
struct Units {
    int64_t units, chunks, chunk, step;
    int lane;
    __device__ __forceinline__ Units(int64_t n) : units(n) {
        chunks = (n + ST_CHUNK * 64 - 1) / (ST_CHUNK * 64);
        chunk = ((int64_t)blockIdx.x * ST_T + threadIdx.x) / 64;
        step = (int64_t)gridDim.x * (ST_T / 64);
        lane = threadIdx.x & 63;
    }
    __device__ __forceinline__ int64_t unit(int64_t c, int it) const { return (c * ST_CHUNK + it) * 64 + lane; }
};

struct Args {
    const void* labels;
    const float* image;
    int64_t voxels;
    unsigned L;
    int bytes;
    float lo, hi, scale;
    bool lab_vec, img_vec;
};

// ---- moments -------------------------------------------------------------------------------------------------------------------------
// the open run of a thread: the voxels of label l since the label last changed
struct MomentRun {
    unsigned l, n, nan, below, above, kmin, kmax;
    u64 sq, sqq;
};

template <bool LDS>
__global__ void __launch_bounds__(ST_T) k_stats_moments(const Args a, u64* sum, unsigned* key) {
    __shared__ u64 ls[LDS ? ST_ROWS * 6 : 1];
    __shared__ unsigned lk[LDS ? ST_ROWS * 2 : 1];
    const int held = min((int)a.L + 1, ST_ROWS);       // the rows this block's table holds
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < held * 6; e += ST_T) ls[e] = 0ull;
        for (int e = threadIdx.x; e < held * 2; e += ST_T) lk[e] = (e & 1) ? 0u : 0xFFFFFFFFu;
        __syncthreads();
    }
    MomentRun run = {};
    bool open = false;
    auto flush = [&]() {
        auto update = [&](u64* s, unsigned* k, auto lds) {  // inlined once per address space: LDS and global atomics, no flat ones
            constexpr bool C = decltype(lds)::value;
            if (run.n) {
                atomicAdd(s + 0, (u64)run.n);
                if (run.sq) {
                    atomicAdd(s + 4, run.sq);
                    atomicAdd(s + 5, run.sqq);
                }
                st_min<C>(k + 0, run.kmin);
                st_max<C>(k + 1, run.kmax);
            }
            if (run.nan) atomicAdd(s + 1, (u64)run.nan);
            if (run.below) atomicAdd(s + 2, (u64)run.below);
            if (run.above) atomicAdd(s + 3, (u64)run.above);
        };
        if (LDS && run.l < (unsigned)ST_ROWS) update(ls + run.l * 6u, lk + run.l * 2u, std::true_type());
        else update(sum + (size_t)run.l * 6, key + (size_t)run.l * 2, std::false_type());
    };
    const Units un((a.voxels + ST_SEG - 1) / ST_SEG);
    for (int64_t c = un.chunk; c < un.chunks; c += un.step) {
        for (int it = 0; it < ST_CHUNK; ++it) {
            const int64_t u = un.unit(c, it);
            if (u >= un.units) break;
            const int64_t i0 = u * ST_SEG;
            const int n = (int)min((int64_t)ST_SEG, a.voxels - i0);
            unsigned l[ST_SEG];
            float v[ST_SEG];
            st_labels(a.labels, a.bytes, a.lab_vec, i0, n, a.L, l);
            st_values(a.image, a.img_vec, i0, n, v);
#pragma unroll
            for (int j = 0; j < ST_SEG; ++j) {
                if (j >= n) break;
                if (!open || run.l != l[j]) {
                    if (open) flush();
                    run = {l[j], 0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0ull, 0ull};
                    open = true;
                }
                const float x = v[j];
                if (x != x) {
                    ++run.nan;
                } else {
                    const unsigned q = st_code(x, a.lo, a.scale), k = st_key(x);
                    ++run.n;
                    run.below += x < a.lo ? 1u : 0u;
                    run.above += x > a.hi ? 1u : 0u;
                    run.sq += (u64)q;
                    run.sqq += (u64)(q * q);           // 65535^2 < 2^32
                    run.kmin = min(run.kmin, k);
                    run.kmax = max(run.kmax, k);
                }
            }
        }
    }
    if (open) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int l = threadIdx.x; l < held; l += ST_T) {
            const u64 cnt = ls[l * 6], nan = ls[l * 6 + 1];
            if ((cnt | nan) == 0ull) continue;         // not touched by this block
            u64* s = sum + (size_t)l * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                if (const u64 x = ls[l * 6 + c]) atomicAdd(s + c, x);
            if (cnt) {
                st_min<false>(key + (size_t)l * 2, lk[l * 2]);
                st_max<false>(key + (size_t)l * 2 + 1, lk[l * 2 + 1]);
            }
        }
    }
}

// the running moments -> int64 rows; every entry is stored
__global__ void __launch_bounds__(ST_T) k_stats_widen(const u64* __restrict__ sum, const unsigned* __restrict__ key, int rows, float lo,
                                                      float scale, int64_t* __restrict__ out) {
    const int i = blockIdx.x * ST_T + threadIdx.x;
    if (i >= rows * 10) return;
    const int l = i / 10, c = i % 10;
    const bool any = sum[l * 6] != 0ull;
    const unsigned kmin = key[l * 2], kmax = key[l * 2 + 1];
    int64_t r;
    if (c < 6) r = (int64_t)sum[l * 6 + c];
    else if (c == 6) r = any ? (int64_t)st_code(st_unkey(kmin), lo, scale) : (int64_t)UNET_STATS_CODES;
    else if (c == 7) r = any ? (int64_t)st_code(st_unkey(kmax), lo, scale) : (int64_t)-1;
    else if (c == 8) r = any ? (int64_t)kmin : (int64_t)0xFFFFFFFFll;
    else r = any ? (int64_t)kmax : (int64_t)-1;
    out[i] = r;
}

// ---- the histogram passes ------------------------------------------------------------------------------------------------------------
template <bool LDS, bool FINE>
__global__ void __launch_bounds__(ST_T) k_stats_count(const Args a, unsigned* cnt, const int* __restrict__ dbin, int Q) {
    __shared__ unsigned lc[LDS ? ST_SLOTS * ST_SBINS : 1];
    __shared__ unsigned lkey[LDS ? ST_SLOTS : 1];     // the counters a slot holds: those from index key * ST_SBINS of cnt on
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < ST_SLOTS * ST_SBINS; e += ST_T) lc[e] = 0u;
        for (int e = threadIdx.x; e < ST_SLOTS; e += ST_T) lkey[e] = ST_NONE;
        __syncthreads();
    }
    unsigned run_row = ST_NONE, run_bin = 0u, run_n = 0u;   // the open run
    unsigned slot_key = ST_NONE;                            // the key this thread last looked up ...
    int slot = -1;                                          // ... and its slot, -1: none, it goes to global memory
    auto flush = [&]() {
        if constexpr (LDS) {
            const unsigned key = (run_row * ST_BINS + run_bin) / ST_SBINS;   // < 2^19: a row is below 4096 * 8
            if (slot_key != key) {
                slot_key = key;
                slot = -1;
                const unsigned h = (key * 2654435761u) >> 23;
#pragma unroll
                for (int p = 0; p < ST_PROBES; ++p) {
                    const unsigned s = (h + p) & (ST_SLOTS - 1);
                    unsigned cur = *(volatile unsigned*)&lkey[s];
                    if (cur == ST_NONE) cur = atomicCAS(&lkey[s], ST_NONE, key);   // claimed for good, by this thread or another
                    if (cur == ST_NONE || cur == key) {
                        slot = (int)s;
                        break;
                    }
                }
            }
            if (slot >= 0) {
                atomicAdd(&lc[slot * ST_SBINS + run_bin % ST_SBINS], run_n);
                return;
            }
        }
        atomicAdd(cnt + (size_t)run_row * ST_BINS + run_bin, run_n);
    };
    unsigned cur_l = ST_NONE;                               // FINE: the label whose distinct chosen bins are in cb
    int cb[ST_MAXQ];
#pragma unroll
    for (int j = 0; j < ST_MAXQ; ++j) cb[j] = -1;
    const Units un((a.voxels + ST_SEG - 1) / ST_SEG);
    for (int64_t c = un.chunk; c < un.chunks; c += un.step) {
        for (int it = 0; it < ST_CHUNK; ++it) {
            const int64_t u = un.unit(c, it);
            if (u >= un.units) break;
            const int64_t i0 = u * ST_SEG;
            const int n = (int)min((int64_t)ST_SEG, a.voxels - i0);
            unsigned l[ST_SEG];
            float v[ST_SEG];
            st_labels(a.labels, a.bytes, a.lab_vec, i0, n, a.L, l);
            st_values(a.image, a.img_vec, i0, n, v);
#pragma unroll
            for (int j = 0; j < ST_SEG; ++j) {
                if (j >= n) break;
                const float x = v[j];
                if (x != x) continue;
                const unsigned q = st_code(x, a.lo, a.scale);
                unsigned row, bin;
                if constexpr (!FINE) {
                    row = l[j];
                    bin = q >> 8;
                } else {
                    if (l[j] != cur_l) {
                        cur_l = l[j];
#pragma unroll
                        for (int k = 0; k < ST_MAXQ; ++k) cb[k] = k < Q ? dbin[(size_t)cur_l * Q + k] : -1;
                    }
                    row = ST_NONE;
#pragma unroll
                    for (int k = 0; k < ST_MAXQ; ++k)
                        if (cb[k] == (int)(q >> 8)) row = cur_l * (unsigned)Q + k;     // distinct bins: at most one k
                    if (row == ST_NONE) continue;
                    bin = q & 255u;
                }
                if (run_n && run_row == row && run_bin == bin) {
                    ++run_n;
                } else {
                    if (run_n) flush();
                    run_row = row;
                    run_bin = bin;
                    run_n = 1u;
                }
            }
        }
    }
    if (run_n) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < ST_SLOTS * ST_SBINS; e += ST_T)
            if (const unsigned x = lc[e]) atomicAdd(cnt + (size_t)lkey[e / ST_SBINS] * ST_SBINS + (e % ST_SBINS), x);
    }
}

struct Permille {
    int p[ST_MAXQ];
};

// the number of leading bins whose running total stays at or below r, and that total: the bin holding rank r and the rank left in it
// (the caller guarantees r < the total of all bins)
__device__ __forceinline__ void st_find(const unsigned* __restrict__ h, unsigned r, int& bin, unsigned& rem) {
    unsigned cum = 0u, base = 0u;
    int b = 0;
    for (int i = 0; i < ST_BINS / 4; ++i) {
        const uint4 w = ((const uint4*)h)[i];
        const unsigned x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cum += x[j];
            if (cum <= r) {
                b = i * 4 + j + 1;
                base = cum;
            }
        }
    }
    bin = min(b, ST_BINS - 1);
    rem = r - base;
}

__global__ void __launch_bounds__(256) k_stats_select(const unsigned* __restrict__ coarse, int rows, const Permille pm, int Q, int* __restrict__ dbin,
                                                      int* __restrict__ own, unsigned* __restrict__ rem, int* __restrict__ kbin) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= rows) return;
    const unsigned* h = coarse + (size_t)l * ST_BINS;
    unsigned n = 0u;                                   // < 2^31
    for (int i = 0; i < ST_BINS / 4; ++i) {
        const uint4 w = ((const uint4*)h)[i];
        n += w.x + w.y + w.z + w.w;
    }
    int nd = 0;
    for (int k = 0; k < Q; ++k) {
        const size_t e = (size_t)l * Q + k;
        dbin[e] = -1;                                  // behind the distinct bins; entries j < nd are written below, by this thread
        if (n == 0u) {
            own[e] = 0;
            rem[e] = 0u;
            kbin[e] = -1;
            continue;
        }
        const unsigned r = (unsigned)(((int64_t)pm.p[k] * (int64_t)(n - 1u)) / 1000);
        int bin;
        unsigned left;
        st_find(h, r, bin, left);
        int j = 0;
        while (j < nd && dbin[(size_t)l * Q + j] != bin) ++j;
        if (j == nd) dbin[(size_t)l * Q + nd++] = bin;
        own[e] = j;
        rem[e] = left;
        kbin[e] = bin;
    }
}

__global__ void __launch_bounds__(256) k_stats_pick(const unsigned* __restrict__ fine, int rows, int Q, const int* __restrict__ own,
                                                    const unsigned* __restrict__ rem, const int* __restrict__ kbin, int32_t* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * Q) return;
    const int cb = kbin[e];
    if (cb < 0) {
        out[e] = -1;
        return;
    }
    const int l = e / Q;
    int bin;
    unsigned left;
    st_find(fine + ((size_t)l * Q + own[e]) * ST_BINS, rem[e], bin, left);
    out[e] = cb * ST_BINS + bin;
}

__global__ void __launch_bounds__(ST_T) k_stats_hist_widen(const unsigned* __restrict__ coarse, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * ST_T + threadIdx.x;
    if (i < n) out[i] = (int64_t)coarse[i];
}

int st_blocks(int64_t voxels) {
    const int64_t units = (voxels + ST_SEG - 1) / ST_SEG, per = (int64_t)ST_T * ST_CHUNK, nb = (units + per - 1) / per;
    return (int)(nb > ST_MAXB ? ST_MAXB : nb < 1 ? 1 : nb);
}
int st_init_blocks(int64_t words) {
    const int64_t nb = (words + ST_T * 4 - 1) / (ST_T * 4);
    return (int)(nb > 2048 ? 2048 : nb < 1 ? 1 : nb);
}

Args st_args(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi, float scale) {
    Args a;
    a.labels = labels;
    a.image = image;
    a.voxels = voxels;
    a.L = (unsigned)n_labels;
    a.bytes = label_bytes;
    a.lo = lo;
    a.hi = hi;
    a.scale = scale;
    a.lab_vec = labels && ((uintptr_t)labels % (size_t)(ST_SEG * label_bytes)) == 0;
    a.img_vec = ((uintptr_t)image & 15) == 0;
    return a;
}

template <bool FINE> void st_count(const Args& a, int impl, unsigned* cnt, const int* dbin, int Q, hipStream_t s) {
    const int nb = st_blocks(a.voxels);
    if (impl != UNET_STATS_IMPL_GLOBAL)   // DEFAULT: LDS
        k_stats_count<true, FINE><<<nb, ST_T, 0, s>>>(a, cnt, dbin, Q);
    else
        k_stats_count<false, FINE><<<nb, ST_T, 0, s>>>(a, cnt, dbin, Q);
}

}  // namespace

size_t stats_scratch_bytes(int n_labels, int n_quantiles) { return 256 + st_scratch(nullptr, n_labels, n_quantiles).bytes; }

void launch_stats_moments(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi, float scale,
                          int64_t* rows, int impl, void* scratch, hipStream_t s) {
    const Scratch sc = st_scratch(scratch, n_labels, 0);
    const int R = n_labels + 1;
    const Args a = st_args(labels, label_bytes, image, voxels, n_labels, lo, hi, scale);
    k_stats_init<<<st_init_blocks((int64_t)R * 12), ST_T, 0, s>>>((unsigned*)sc.sum, (int64_t)R * 12, sc.key, R);
    const int nb = st_blocks(voxels);
    if (impl != UNET_STATS_IMPL_GLOBAL)   // DEFAULT: LDS
        k_stats_moments<true><<<nb, ST_T, 0, s>>>(a, sc.sum, sc.key);
    else
        k_stats_moments<false><<<nb, ST_T, 0, s>>>(a, sc.sum, sc.key);
    k_stats_widen<<<(R * 10 + ST_T - 1) / ST_T, ST_T, 0, s>>>(sc.sum, sc.key, R, lo, scale, rows);
}

void launch_stats_hist(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi, float scale,
                       int64_t* rows, int impl, void* scratch, hipStream_t s) {
    const Scratch sc = st_scratch(scratch, n_labels, 0);
    const int64_t words = (int64_t)(n_labels + 1) * ST_BINS;
    const Args a = st_args(labels, label_bytes, image, voxels, n_labels, lo, hi, scale);
    k_stats_init<<<st_init_blocks(words), ST_T, 0, s>>>(sc.coarse, words, nullptr, 0);
    st_count<false>(a, impl, sc.coarse, nullptr, 0, s);
    k_stats_hist_widen<<<(unsigned)((words + ST_T - 1) / ST_T), ST_T, 0, s>>>(sc.coarse, words, rows);
}

void launch_stats_quantiles(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                            float scale, const int* permille, int n_quantiles, int32_t* out, int impl, void* scratch, hipStream_t s) {
    const int R = n_labels + 1, Q = n_quantiles;
    const Scratch sc = st_scratch(scratch, n_labels, Q);
    const Args a = st_args(labels, label_bytes, image, voxels, n_labels, lo, hi, scale);
    Permille pm = {};
    for (int k = 0; k < Q; ++k) pm.p[k] = permille[k];
    const int64_t words = (int64_t)R * (1 + Q) * ST_BINS;   // coarse and fine are adjacent: R * 1 KiB is a multiple of 256 B
    k_stats_init<<<st_init_blocks(words), ST_T, 0, s>>>(sc.coarse, words, nullptr, 0);
    st_count<false>(a, impl, sc.coarse, nullptr, 0, s);
    k_stats_select<<<(R + 255) / 256, 256, 0, s>>>(sc.coarse, R, pm, Q, sc.dbin, sc.own, sc.rem, sc.kbin);
    st_count<true>(a, impl, sc.fine, sc.dbin, Q, s);
    k_stats_pick<<<(R * Q + 255) / 256, 256, 0, s>>>(sc.fine, R, Q, sc.own, sc.rem, sc.kbin, out);
}

}  // namespace unet
