// The instances of a label map (include/unet_instances.h): every 6-connected component of the listed classes numbered densely and
// tabulated, the overlap pairs of two instance maps, and the removal of small instances.
//
// label
//   launch_components_label   the labelling stage of kernels_components.hip: parent[v] = the component's smallest linear index (its
//                    root) or -1, count[root] = its voxels
//   k_inst_sums      a block counts the roots (parent[v] == v) among its INST_T * INST_ITEMS consecutive voxels
//   k_inst_scan      ONE block turns the block sums into their exclusive prefixes in place (a thread adds up a contiguous share, the
//                    shares are scanned in LDS) and writes info = {N, min(N, max_instances)}
//   k_inst_assign    a block scans its threads' root counts in LDS and numbers its roots from its prefix: inst[root] = id,
//                    root_of[id] = root for the ids that have a row; inst = 0 for a voxel that is no member
//   k_inst_gather    inst[v] = inst[parent[v]] for the members that are no roots (it reads roots only and writes the others only)
//   k_inst_init      the running table in the scratch: sums 0, minima (w, h, d), maxima -1
//   k_inst_rows      kernels_table.hip's scheme over inst: a thread takes units of INST_SEG consecutive voxels along x and merges
//                    equal consecutive ids into one update per run, the run staying open across the thread's units; LDS == true
//                    gathers the ids below UNET_INST_LDS_ROWS in the block's LDS table and flushes one update per touched row.  Id 0
//                    and the ids above max_instances send nothing.  The voxel counts are not gathered again: count[root] has them
//   k_inst_widen     the running table, count[root], label[root] and root -> int64 rows, every entry stored; row 0 and the rows
//                    above N are the empty row
// The three scan kernels and the gather, table and match kernels take a fixed stretch of voxels per block on an uncapped grid (at
// most 2^31 / 4096 blocks): there is no grid-stride path, and no kernel ever waits for another block.
//
// match
//   k_match_pairs    units of INST_SEG consecutive voxels of both maps, equal consecutive pairs merged into runs as above.  A run
//                    goes into an open-addressing table of 64-bit keys (0 = empty: a pair has ia > 0): the slot is claimed by
//                    compare-and-swap, the count added with an integer add, linear probing bounded by the number of slots, then
//                    the overflow flag is raised instead.  LDS == true: into the block's table of UNET_INST_LDS_SLOTS slots first
//                    (at most MATCH_LDS_PROBES probes, then directly to the global table), flushed with one update per used slot
//   k_match_compact  every used slot takes the next place of keys / counts from a cursor while it is below max_pairs
//   k_match_finish   info = {min(cursor, max_pairs), cursor > max_pairs or the flag}
// The global table has at least 2 * max_pairs slots, so a probe gives up only when more than max_pairs distinct pairs exist.
//
// remove_small
//   k_inst_remove    label = 0 where 1 <= inst <= max_instances and the row's count is below min_voxels; removed[class] as in
//                    kernels_components.hip (a block histogram in LDS for the classes below INST_HIST, global adds above)
// Every atomic is an integer compare-and-swap, add, minimum or maximum: the results do not depend on the schedule.
//
// Scratch of label, each part 256-B aligned: the labelling's (components_scratch_bytes), then block sums uint32[blocks], root_of
// int32[M + 1], sums uint64[(M + 1) * 3], extremes int32[(M + 1) * 6].  Scratch of match: keys uint64[slots], counts
// uint64[slots], {cursor, flag} uint64[2].
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/unet_instances.h"
#include "device_util.h"

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int INST_T = 256;                           // threads per block of the scan, gather and remove kernels
constexpr int INST_ITEMS = 16;                        // consecutive voxels per thread there
constexpr int INST_BLOCK = INST_T * INST_ITEMS;       // voxels per block there
constexpr int SCAN_T = 1024;                          // threads of the one block that scans the block sums
constexpr int TAB_T = 512;                            // threads per block of the table and match kernels
constexpr int INST_SEG = 8;                           // consecutive voxels a thread takes at once: a unit
constexpr int INST_CHUNK = 8;                         // units per thread: lane i of a wave takes units i, 64 + i, ... of its 512
constexpr int TAB_UNITS = TAB_T * INST_CHUNK;         // units per block
constexpr int LROWS = UNET_INST_LDS_ROWS;
constexpr int LSLOTS = UNET_INST_LDS_SLOTS;
constexpr int MATCH_LDS_PROBES = 16;
constexpr int INST_HIST = 2048;                       // classes whose removed counts a block gathers in LDS
constexpr u64 MIN_SLOTS = 64;
static_assert(LROWS * (3 * 8 + 6 * 4) <= 64 * 1024, "the LDS table of a block");
static_assert((LSLOTS & (LSLOTS - 1)) == 0 && LSLOTS * 12 <= 64 * 1024, "the LDS pair table of a block");
static_assert(TAB_T % 64 == 0 && INST_T % 64 == 0, "whole waves");

size_t inst_align(size_t b) { return (b + 255) & ~(size_t)255; }

unsigned inst_blocks(int64_t S) { return (unsigned)((S + INST_BLOCK - 1) / INST_BLOCK); }

void inst_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("unet_inst: ") + what + ": " + hipGetErrorString(e));
}

// ---- the dense numbering ---------------------------------------------------------------------------------------------------------
// the roots among a thread's INST_ITEMS consecutive voxels
__device__ __forceinline__ unsigned inst_thread_roots(int S, const int* __restrict__ parent, int64_t v0) {
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < INST_ITEMS; ++k) {
        const int64_t v = v0 + k;
        if (v < S && parent[v] == (int)v) ++n;
    }
    return n;
}

// exclusive prefix of one value per thread over a block of T threads (whole waves); *total receives the block's sum when given.
// lds: T / 64 + 1 entries.  Every thread of the block must call it
template <int T>
__device__ __forceinline__ unsigned inst_block_scan(unsigned v, unsigned* lds, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        for (int w = 0; w < T / 64; ++w) {
            const unsigned t = lds[w];
            lds[w] = run;
            run += t;
        }
        lds[T / 64] = run;
    }
    __syncthreads();
    const unsigned excl = lds[wave] + inc - v;
    if (total) *total = lds[T / 64];
    __syncthreads();                                  // lds may be reused by the caller's next scan
    return excl;
}

__global__ void __launch_bounds__(INST_T) k_inst_sums(int S, const int* __restrict__ parent, unsigned* __restrict__ bsum) {
    __shared__ unsigned lds[INST_T / 64 + 1];
    const int64_t v0 = (int64_t)blockIdx.x * INST_BLOCK + (int64_t)threadIdx.x * INST_ITEMS;
    unsigned total;
    inst_block_scan<INST_T>(inst_thread_roots(S, parent, v0), lds, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum[b] -> the roots in the blocks before b; N < 2^31 fits 32 bits
__global__ void __launch_bounds__(SCAN_T) k_inst_scan(unsigned nblk, unsigned* __restrict__ bsum, int64_t max_instances,
                                                      int64_t* __restrict__ info) {
    __shared__ unsigned lds[SCAN_T / 64 + 1];
    const unsigned per = (nblk + SCAN_T - 1) / SCAN_T;
    const unsigned b0 = min(threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
    unsigned sum = 0;
    for (unsigned b = b0; b < b1; ++b) sum += bsum[b];
    unsigned total;
    unsigned run = inst_block_scan<SCAN_T>(sum, lds, &total);
    for (unsigned b = b0; b < b1; ++b) {
        const unsigned t = bsum[b];
        bsum[b] = run;
        run += t;
    }
    if (threadIdx.x == 0) {
        info[0] = (int64_t)total;
        info[1] = (int64_t)total < max_instances ? (int64_t)total : max_instances;
    }
}

__global__ void __launch_bounds__(INST_T) k_inst_assign(int S, const int* __restrict__ parent, const unsigned* __restrict__ bsum,
                                                        int64_t max_instances, int* __restrict__ inst, int* __restrict__ root_of) {
    __shared__ unsigned lds[INST_T / 64 + 1];
    const int64_t v0 = (int64_t)blockIdx.x * INST_BLOCK + (int64_t)threadIdx.x * INST_ITEMS;
    unsigned id = bsum[blockIdx.x] + inst_block_scan<INST_T>(inst_thread_roots(S, parent, v0), lds, nullptr);
#pragma unroll
    for (int k = 0; k < INST_ITEMS; ++k) {
        const int64_t v = v0 + k;
        if (v >= S) break;
        const int p = parent[v];
        if (p == (int)v) {
            ++id;                                     // ids start at 1
            inst[v] = (int)id;
            if ((int64_t)id <= max_instances) root_of[id] = (int)v;
        } else if (p < 0) {
            inst[v] = 0;
        }
    }
}

__global__ void __launch_bounds__(INST_T) k_inst_gather(int S, const int* __restrict__ parent, int* inst) {
    const int64_t v0 = (int64_t)blockIdx.x * INST_BLOCK + (int64_t)threadIdx.x * INST_ITEMS;
#pragma unroll
    for (int k = 0; k < INST_ITEMS; ++k) {
        const int64_t v = v0 + k;
        if (v >= S) break;
        const int p = parent[v];
        if (p >= 0 && p != (int)v) inst[v] = inst[p]; // inst[p]: a root's, written by the launch before and by nobody here
    }
}

// ---- the table -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(INST_T) k_inst_init(u64* __restrict__ sum, int* __restrict__ ext, int64_t rows, int w, int h, int d) {
    const int64_t i = (int64_t)blockIdx.x * INST_T + threadIdx.x;
    if (i < rows * 3) sum[i] = 0ull;
    if (i < rows * 6) {
        const int c = (int)(i % 6);
        ext[i] = c == 0 ? w : c == 1 ? h : c == 2 ? d : -1;
    }
}

// min / max into a block's LDS table, sent only when the table does not hold it yet (kernels_table.hip: the entry only ever moves
// towards the extreme, so a stale read costs an update, never a result).  Global entries are always sent
template <bool CHECK> __device__ __forceinline__ void inst_min(int* p, int v) {
    if (!CHECK || v < *(volatile int*)p) atomicMin(p, v);
}
template <bool CHECK> __device__ __forceinline__ void inst_max(int* p, int v) {
    if (!CHECK || v > *(volatile int*)p) atomicMax(p, v);
}

// unit `it` of this thread: a wave owns 64 * INST_CHUNK consecutive units of its block's TAB_UNITS, lane i the units i, 64 + i, ...
__device__ __forceinline__ int64_t inst_unit(int it) {
    return (int64_t)blockIdx.x * TAB_UNITS + (int64_t)(threadIdx.x >> 6) * (64 * INST_CHUNK) + it * 64 + (threadIdx.x & 63);
}

// the n <= INST_SEG ids of a unit from p + i0, 0 behind them; vec: p + i0 is 16-B aligned, so a whole unit is two 16-B loads
__device__ __forceinline__ void inst_load(const int* __restrict__ p, int64_t i0, int n, bool vec, int (&v)[INST_SEG]) {
    static_assert(INST_SEG == 8, "two int4 loads");
    if (vec && n == INST_SEG) {
        const int4 lo = *(const int4*)(p + i0), hi = *(const int4*)(p + i0 + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < INST_SEG; ++j) v[j] = j < n ? p[i0 + j] : 0;
    }
}

struct InstRun {
    unsigned id, n;
    u64 sx, sy, sz;
    int x0, y0, z0, x1, y1, z1;
};

template <bool LDS>
__global__ void __launch_bounds__(TAB_T) k_inst_rows(const int* __restrict__ inst, int w, int h, int d, unsigned M, u64* sum, int* ext,
                                                     bool vec /* inst is 16-B aligned and w a multiple of 4 */) {
    __shared__ u64 ls[LDS ? LROWS * 3 : 1];
    __shared__ int le[LDS ? LROWS * 6 : 1];
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < LROWS * 3; e += TAB_T) ls[e] = 0ull;
        for (int e = threadIdx.x; e < LROWS * 6; e += TAB_T) {
            const int c = e % 6;
            le[e] = c == 0 ? w : c == 1 ? h : c == 2 ? d : -1;
        }
        __syncthreads();
    }
    InstRun run = {};
    auto flush = [&]() {
        auto update = [&](u64* s, int* e, auto lds) {  // inlined once per address space: LDS and global atomics, no flat ones
            constexpr bool C = decltype(lds)::value;
            atomicAdd(s + 0, run.sx);
            atomicAdd(s + 1, run.sy);
            atomicAdd(s + 2, run.sz);
            inst_min<C>(e + 0, run.x0);
            inst_min<C>(e + 1, run.y0);
            inst_min<C>(e + 2, run.z0);
            inst_max<C>(e + 3, run.x1);
            inst_max<C>(e + 4, run.y1);
            inst_max<C>(e + 5, run.z1);
        };
        if (LDS && run.id < (unsigned)LROWS) update(ls + run.id * 3u, le + run.id * 6u, std::true_type());
        else update(sum + (size_t)run.id * 3, ext + (size_t)run.id * 6, std::false_type());
    };
    // n voxels of one id from (x0, y, z) along x: they extend the open run or close it and open the next.  Id 0 and the ids without
    // a row (above M; a negative value reads as one) only close it
    auto push = [&](unsigned id, int x0, int n, int y, int z) {
        if (run.n && run.id == id) {
            const u64 n64 = (u64)n;
            run.n += (unsigned)n;
            run.sx += n64 * (u64)x0 + (n64 * (n64 - 1ull)) / 2ull; run.sy += n64 * (u64)y; run.sz += n64 * (u64)z;
            run.x0 = min(run.x0, x0); run.y0 = min(run.y0, y); run.z0 = min(run.z0, z);
            run.x1 = max(run.x1, x0 + n - 1); run.y1 = max(run.y1, y); run.z1 = max(run.z1, z);
            return;
        }
        if (run.n) flush();
        run.n = 0;
        if (id == 0u || id > M) return;
        const u64 n64 = (u64)n;
        run = {id, (unsigned)n, n64 * (u64)x0 + (n64 * (n64 - 1ull)) / 2ull, n64 * (u64)y, n64 * (u64)z, x0, y, z, x0 + n - 1, y, z};
    };
    const int nseg = (w + INST_SEG - 1) / INST_SEG;
    const int64_t units = (int64_t)nseg * h * d;       // <= voxels < 2^31
    for (int it = 0; it < INST_CHUNK; ++it) {
        const int64_t u = inst_unit(it);
        if (u >= units) break;
        const unsigned u32 = (unsigned)u;
        const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg);
        const int y = r % h, z = r / h, x0 = seg * INST_SEG, n = min(INST_SEG, w - x0);
        const int64_t row = ((int64_t)z * h + y) * w + x0;
        int v[INST_SEG];
        inst_load(inst, row, n, vec, v);
        unsigned key = (unsigned)v[0];
        int start = 0;
#pragma unroll
        for (int j = 1; j < INST_SEG; ++j) {
            if (j < n && (unsigned)v[j] != key) {
                push(key, x0 + start, j - start, y, z);
                key = (unsigned)v[j];
                start = j;
            }
        }
        push(key, x0 + start, n - start, y, z);        // n >= 1: the unit's last stretch
    }
    if (run.n) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int l = threadIdx.x; l < LROWS; l += TAB_T) {
            if (le[l * 6] >= w) continue;              // min x still at its start: not touched by this block
            u64* s = sum + (size_t)l * 3;
            int* e = ext + (size_t)l * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) atomicAdd(s + c, ls[l * 3 + c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) inst_min<false>(e + c, le[l * 6 + c]);
#pragma unroll
            for (int c = 3; c < 6; ++c) inst_max<false>(e + c, le[l * 6 + c]);
        }
    }
}

// every entry of rows is stored; info[0] = N was written by k_inst_scan
__global__ void __launch_bounds__(INST_T) k_inst_widen(const u64* __restrict__ sum, const int* __restrict__ ext, const int* __restrict__ root_of,
                                                       const unsigned* __restrict__ count, const uint16_t* __restrict__ label,
                                                       const int64_t* __restrict__ info, int64_t rows, int w, int h, int d,
                                                       int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * INST_T + threadIdx.x;
    if (i >= rows * UNET_INST_COLUMNS) return;
    const int64_t k = i / UNET_INST_COLUMNS;
    const int c = (int)(i % UNET_INST_COLUMNS);
    int64_t v;
    if (k >= 1 && k <= info[0]) {
        const int r = root_of[k];
        v = c == 0 ? (int64_t)label[r] : c == 1 ? (int64_t)count[r] : c < 5 ? (int64_t)sum[k * 3 + (c - 2)] : c < 11 ? (int64_t)ext[k * 6 + (c - 5)] : (int64_t)r;
    } else {
        v = c < 5 ? 0 : c == 5 ? w : c == 6 ? h : c == 7 ? d : -1;
    }
    out[i] = v;
}

// ---- the pairs -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 match_hash(u64 k) {    // the 64-bit finaliser of MurmurHash3: pairs that share a word spread out
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

// n voxels of pair `key` into the global table.  Terminates: at most `slots` probes, none of which waits for anything
__device__ __forceinline__ void match_global(u64* __restrict__ keys, u64* __restrict__ counts, u64 mask, u64* __restrict__ flag, u64 key, u64 n) {
    u64 h = match_hash(key) & mask;
    for (u64 probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        u64 cur = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {                             // claim it; a failed claim returns the pair that took it first
            cur = atomicCAS(keys + h, 0ull, key);
            if (cur == 0ull) cur = key;
        }
        if (cur == key) {
            atomicAdd(counts + h, n);                  // counts were zeroed before the launch: no order with the claim is needed
            return;
        }
    }
    atomicOr(flag, 1ull);                              // every slot holds another pair: more than max_pairs of them exist
}

template <bool LDS>
__global__ void __launch_bounds__(TAB_T) k_match_pairs(const int* __restrict__ ia, const int* __restrict__ ib, int64_t voxels,
                                                       u64* __restrict__ keys, u64* __restrict__ counts, u64 mask, u64* __restrict__ flag,
                                                       bool vec /* both maps are 16-B aligned */) {
    __shared__ u64 lk[LDS ? LSLOTS : 1];
    __shared__ unsigned lc[LDS ? LSLOTS : 1];
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < LSLOTS; e += TAB_T) {
            lk[e] = 0ull;
            lc[e] = 0u;
        }
        __syncthreads();
    }
    u64 open_key = 0ull;
    unsigned open_n = 0u;
    auto flush = [&]() {
        if constexpr (LDS) {
            unsigned h = (unsigned)match_hash(open_key) & (LSLOTS - 1);
            for (int probe = 0; probe < MATCH_LDS_PROBES; ++probe, h = (h + 1) & (LSLOTS - 1)) {
                u64 cur = *(volatile u64*)(lk + h);
                if (cur == 0ull) {
                    cur = atomicCAS(lk + h, 0ull, open_key);
                    if (cur == 0ull) cur = open_key;
                }
                if (cur == open_key) {
                    atomicAdd(lc + h, open_n);         // a block holds TAB_UNITS * INST_SEG voxels: 32 bits suffice
                    return;
                }
            }
        }
        match_global(keys, counts, mask, flag, open_key, (u64)open_n);
    };
    auto push = [&](u64 key, unsigned n) {             // key 0: a voxel outside one of the maps' instances only closes the run
        if (open_n && open_key == key) {
            open_n += n;
            return;
        }
        if (open_n) flush();
        open_key = key;
        open_n = key ? n : 0u;
    };
    const int64_t units = (voxels + INST_SEG - 1) / INST_SEG;
    for (int it = 0; it < INST_CHUNK; ++it) {
        const int64_t u = inst_unit(it);
        if (u >= units) break;
        const int64_t i0 = u * INST_SEG;
        const int n = (int)min((int64_t)INST_SEG, voxels - i0);
        int a[INST_SEG], b[INST_SEG];
        inst_load(ia, i0, n, vec, a);
        inst_load(ib, i0, n, vec, b);
        u64 key[INST_SEG];
#pragma unroll
        for (int j = 0; j < INST_SEG; ++j) key[j] = a[j] > 0 && b[j] > 0 ? ((u64)(unsigned)a[j] << 32) | (u64)(unsigned)b[j] : 0ull;
        u64 k = key[0];
        int start = 0;
#pragma unroll
        for (int j = 1; j < INST_SEG; ++j) {
            if (j < n && key[j] != k) {
                push(k, (unsigned)(j - start));
                k = key[j];
                start = j;
            }
        }
        push(k, (unsigned)(n - start));
    }
    if (open_n) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < LSLOTS; e += TAB_T)
            if (const u64 key = lk[e]) match_global(keys, counts, mask, flag, key, (u64)lc[e]);
    }
}

__global__ void __launch_bounds__(INST_T) k_match_compact(const u64* __restrict__ keys, const u64* __restrict__ counts, u64 slots,
                                                          u64* __restrict__ cursor, u64 max_pairs, u64* __restrict__ out_keys,
                                                          int64_t* __restrict__ out_counts) {
    const u64 i = (u64)blockIdx.x * INST_T + threadIdx.x;
    if (i >= slots) return;
    const u64 key = keys[i];
    if (key == 0ull) return;
    const u64 at = atomicAdd(cursor, 1ull);
    if (at < max_pairs) {
        out_keys[at] = key;
        out_counts[at] = (int64_t)counts[i];
    }
}

__global__ void k_match_finish(const u64* __restrict__ cursor_flag, u64 max_pairs, int64_t* __restrict__ info) {
    const u64 n = cursor_flag[0];
    info[0] = (int64_t)(n < max_pairs ? n : max_pairs);
    info[1] = n > max_pairs || cursor_flag[1] ? 1 : 0;
}

// ---- remove_small ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(INST_T) k_inst_remove(uint16_t* __restrict__ label, const int* __restrict__ inst, int64_t voxels,
                                                        const int64_t* __restrict__ rows, int64_t max_instances, int64_t min_voxels,
                                                        unsigned* __restrict__ removed, int n_classes) {
    __shared__ unsigned hist[INST_HIST];
    if (removed) {
        for (int c = threadIdx.x; c < INST_HIST; c += INST_T) hist[c] = 0u;
        __syncthreads();
    }
    const int64_t v0 = (int64_t)blockIdx.x * INST_BLOCK + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < INST_ITEMS; ++k) {
        const int64_t v = v0 + (int64_t)k * INST_T;
        if (v >= voxels) break;
        const int id = inst[v];
        if (id < 1 || (int64_t)id > max_instances || rows[(int64_t)id * UNET_INST_COLUMNS + 1] >= min_voxels) continue;
        const int c = (int)label[v];
        label[v] = 0;
        if (removed && c < n_classes) {
            if (c < INST_HIST) atomicAdd(&hist[c], 1u);
            else atomicAdd(removed + c, 1u);
        }
    }
    if (removed) {
        __syncthreads();
        for (int c = threadIdx.x; c < INST_HIST && c < n_classes; c += INST_T)
            if (hist[c]) atomicAdd(removed + c, hist[c]);
    }
}

struct Extras {
    unsigned* bsum;
    int* root_of;
    u64* sum;
    int* ext;
    size_t bytes;
};
Extras inst_extras(char* b, int64_t S, int64_t M) {
    Extras x;
    size_t o = 0;
    x.bsum = (unsigned*)(b + o);     o += inst_align((size_t)inst_blocks(S) * 4);
    x.root_of = (int*)(b + o);       o += inst_align((size_t)(M + 1) * 4);
    x.sum = (u64*)(b + o);           o += inst_align((size_t)(M + 1) * 3 * 8);
    x.ext = (int*)(b + o);           o += inst_align((size_t)(M + 1) * 6 * 4);
    x.bytes = o;
    return x;
}

u64 match_slots(int64_t max_pairs) {
    u64 slots = MIN_SLOTS;
    while (slots < 2 * (u64)max_pairs) slots <<= 1;    // max_pairs <= 2^30: at most 2^31 slots
    return slots;
}

}  // namespace

size_t inst_scratch_bytes(int64_t S, int n_classes, int64_t max_instances) {
    return components_scratch_bytes(S, n_classes) + inst_extras(nullptr, S, max_instances).bytes;
}

// classes: n sorted distinct entries in (0, n_classes), host memory; read before this returns
void launch_inst_label(int W, int H, int D, const uint16_t* label, int n_classes, const uint32_t* classes, int n, int32_t* inst,
                       int64_t* rows, int64_t M, int64_t* info, int impl, int connectivity, void* scratch, hipStream_t s) {
    const int S = W * H * D;   // < 2^31 (checked by the caller)
    const int cmp_impl = impl == UNET_INST_LABEL_GLOBAL ? UNET_COMPONENTS_IMPL_GLOBAL : UNET_COMPONENTS_IMPL_TILED;   // DEFAULT: TILED
    const ComponentsForest f = launch_components_label(W, H, D, label, n_classes, classes, n, cmp_impl, connectivity, scratch, s);
    const Extras x = inst_extras(f.end, S, M);
    const unsigned nblk = inst_blocks(S);
    k_inst_sums<<<nblk, INST_T, 0, s>>>(S, f.parent, x.bsum);
    k_inst_scan<<<1, SCAN_T, 0, s>>>(nblk, x.bsum, M, info);
    k_inst_assign<<<nblk, INST_T, 0, s>>>(S, f.parent, x.bsum, M, inst, x.root_of);
    k_inst_gather<<<nblk, INST_T, 0, s>>>(S, f.parent, inst);
    const int64_t R = M + 1;
    k_inst_init<<<cdiv64(R * 6, INST_T), INST_T, 0, s>>>(x.sum, x.ext, R, W, H, D);
    const int64_t units = (int64_t)((W + INST_SEG - 1) / INST_SEG) * H * D;
    const unsigned M32 = (unsigned)(M > 0x7FFFFFFF ? 0x7FFFFFFF : M);
    const bool vec = ((uintptr_t)inst & 15) == 0 && W % 4 == 0;
    if (impl == UNET_INST_LABEL_GLOBAL)   // the second witness takes the table without a block's LDS too
        k_inst_rows<false><<<cdiv64(units, TAB_UNITS), TAB_T, 0, s>>>(inst, W, H, D, M32, x.sum, x.ext, vec);
    else
        k_inst_rows<true><<<cdiv64(units, TAB_UNITS), TAB_T, 0, s>>>(inst, W, H, D, M32, x.sum, x.ext, vec);
    k_inst_widen<<<cdiv64(R * UNET_INST_COLUMNS, INST_T), INST_T, 0, s>>>(x.sum, x.ext, x.root_of, f.count, label, info, R, W, H, D, rows);
}

size_t inst_match_scratch_bytes(int64_t max_pairs) { return 256 + 2 * inst_align((size_t)match_slots(max_pairs) * 8) + 256; }

void launch_inst_match(const int32_t* ia, const int32_t* ib, int64_t voxels, unsigned long long* out_keys, int64_t* out_counts,
                       int64_t max_pairs, int64_t* info, int impl, void* scratch, hipStream_t s) {
    const u64 slots = match_slots(max_pairs);
    char* b = (char*)inst_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    u64* keys = (u64*)b;
    u64* counts = (u64*)(b + inst_align((size_t)slots * 8));
    u64* cursor = (u64*)(b + 2 * inst_align((size_t)slots * 8));   // {cursor, flag}
    inst_check(hipMemsetAsync(b, 0, 2 * inst_align((size_t)slots * 8) + 16, s), "hipMemsetAsync");
    const unsigned nb = cdiv64((voxels + INST_SEG - 1) / INST_SEG, TAB_UNITS);
    const bool vec = (((uintptr_t)ia | (uintptr_t)ib) & 15) == 0;
    if (impl == UNET_INST_IMPL_GLOBAL)
        k_match_pairs<false><<<nb, TAB_T, 0, s>>>(ia, ib, voxels, keys, counts, slots - 1, cursor + 1, vec);
    else   // DEFAULT: LDS
        k_match_pairs<true><<<nb, TAB_T, 0, s>>>(ia, ib, voxels, keys, counts, slots - 1, cursor + 1, vec);
    k_match_compact<<<cdiv64((int64_t)slots, INST_T), INST_T, 0, s>>>(keys, counts, slots, cursor, (u64)max_pairs, out_keys, out_counts);
    k_match_finish<<<1, 1, 0, s>>>(cursor, (u64)max_pairs, info);
}

void launch_inst_remove_small(uint16_t* label, const int32_t* inst, int64_t voxels, const int64_t* rows, int64_t max_instances,
                              int64_t min_voxels, uint32_t* removed, int n_classes, hipStream_t s) {
    if (removed) inst_check(hipMemsetAsync(removed, 0, (size_t)n_classes * 4, s), "hipMemsetAsync");
    k_inst_remove<<<inst_blocks(voxels), INST_T, 0, s>>>(label, inst, voxels, rows, max_instances, min_voxels, removed, n_classes);
}

}  // namespace unet
