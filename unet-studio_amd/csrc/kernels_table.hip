// The tables of a label map (include/unet_table.h): per label its size, its coordinate sums and its bounding box from one pass over a
// region map, and the three counts a Dice coefficient per label needs from one pass over two maps.
//
//   k_table_init     the running table in the scratch: sums 0, minima (w, h, d), maxima -1 (overlap: counters 0)
//   k_table_regions  grid-stride over units of TAB_SEG voxels along x; a thread reads its unit's labels once and merges equal
//                    consecutive labels in registers, and the run stays open across the thread's units (struct Units: they lie a few
//                    rows apart) until another label ends it: one update per run.  LDS: a row below UNET_TABLE_LDS_ROWS is updated in the
//                    block's LDS table (four 64-bit sums, six 32-bit extremes: 56 B a row, 56 KiB), flushed with one global update
//                    per touched row; a row at or above it, and every row with LDS == false, is updated in the scratch directly
//   k_table_overlap  the same over the flat index of two maps, a run being equal consecutive (a, b) pairs; 32-bit counters
//   k_table_widen    the running table -> int64 rows, every entry stored: the caller's rows need no preparation
// Every atomic is an integer add, minimum or maximum: the results do not depend on the schedule.
//
// Scratch, each part 256-B aligned: sums uint64[(L + 1) * 4], extremes int32[(L + 1) * 6]; overlap: counters uint32[(L + 1) * 3] in
// the first part.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/unet_table.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int TAB_T = 512;                            // threads per block: two blocks of 56 KiB fill a CU's LDS with 16 waves
constexpr int TAB_MAXB = 512;                         // grid cap; the kernels stride over the rest
constexpr int TAB_SEG = 8;                            // consecutive voxels along x a thread takes at once: a unit
constexpr int TAB_CHUNK = 8;                          // units a lane takes from one stretch of 64 * TAB_CHUNK consecutive units
static_assert(TAB_T % 64 == 0, "whole waves");
constexpr int TAB_ROWS = UNET_TABLE_LDS_ROWS;
static_assert(TAB_ROWS * (4 * 8 + 6 * 4) <= 64 * 1024, "the LDS table of a block");

typedef unsigned long long u64;

size_t tab_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    u64* sum;        // regions: (L + 1) x {number, sum x, sum y, sum z}
    int* ext;        // regions: (L + 1) x {min x, y, z, max x, y, z}
    unsigned* cnt;   // overlap: (L + 1) x {a, b, both}, in the first part
    size_t bytes;    // from the aligned base
};
Scratch tab_scratch(void* scratch, int L) {
    char* b = (char*)tab_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    size_t o = 0;
    s.sum = (u64*)(b + o);
    s.cnt = (unsigned*)(b + o);   o += tab_align((size_t)(L + 1) * 4 * 8);
    s.ext = (int*)(b + o);        o += tab_align((size_t)(L + 1) * 6 * 4);
    s.bytes = o;
    return s;
}

// a label as read: uint8 or uint16 at any alignment; a value above L reads as 0
__device__ __forceinline__ unsigned tab_label(const void* __restrict__ p, int bytes, int64_t i, unsigned L) {
    const unsigned v = bytes == 1 ? (unsigned)((const uint8_t*)p)[i]
                                  : (unsigned)((const uint8_t*)p)[2 * i] | ((unsigned)((const uint8_t*)p)[2 * i + 1] << 8);
    return v > L ? 0u : v;
}

// min / max into a block's LDS table, sent only when the table does not hold it yet (a volatile read: other threads write it; the
// entry only ever moves towards the extreme, so a stale read costs an update, never a result).  Global entries are always sent
template <bool CHECK> __device__ __forceinline__ void tab_min(int* p, int v) {
    if (!CHECK || v < *(volatile int*)p) atomicMin(p, v);
}
template <bool CHECK> __device__ __forceinline__ void tab_max(int* p, int v) {
    if (!CHECK || v > *(volatile int*)p) atomicMax(p, v);
}

__global__ void __launch_bounds__(TAB_T) k_table_init(u64* __restrict__ sum, int* __restrict__ ext, unsigned* __restrict__ cnt, int rows,
                                                      int w, int h, int d) {
    const int i = blockIdx.x * TAB_T + threadIdx.x;
    if (cnt) {                                         // overlap
        if (i < rows * 3) cnt[i] = 0u;
        return;
    }
    if (i < rows * 4) sum[i] = 0ull;
    if (i < rows * 6) {
        const int c = i % 6;
        ext[i] = c == 0 ? w : c == 1 ? h : c == 2 ? d : -1;
    }
}

// The units of a wave: a wave takes TAB_CHUNK * 64 consecutive units at a time and lane i the units i, 64 + i, 128 + i, ... of them, so
// that a wave-instruction reads 64 consecutive units and a lane's successive units lie close together (a few rows apart): in a solid
// map they mostly read the same label and stay one open run in the lane's registers.
struct Units {
    int64_t units, chunks, chunk, step;
    int lane;
    __device__ __forceinline__ Units(int64_t n) : units(n) {
        chunks = (n + TAB_CHUNK * 64 - 1) / (TAB_CHUNK * 64);
        chunk = ((int64_t)blockIdx.x * TAB_T + threadIdx.x) / 64;
        step = (int64_t)gridDim.x * (TAB_T / 64);
        lane = threadIdx.x & 63;
    }
    __device__ __forceinline__ int64_t unit(int64_t c, int it) const { return (c * TAB_CHUNK + it) * 64 + lane; }
};

// ---- regions ---------------------------------------------------------------------------------------------------------------------
// the open run of a thread: n voxels of label l, their coordinate sums and extremes
struct RegionRun {
    unsigned l, n;
    u64 sx, sy, sz;
    int x0, y0, z0, x1, y1, z1;
};

template <bool LDS>
__global__ void __launch_bounds__(TAB_T) k_table_regions(const void* __restrict__ labels, int bytes, int w, int h, int d, unsigned L,
                                                         u64* sum, int* ext) {
    __shared__ u64 ls[LDS ? TAB_ROWS * 4 : 1];
    __shared__ int le[LDS ? TAB_ROWS * 6 : 1];
    const int held = min((int)L + 1, TAB_ROWS);        // the rows this block's table holds
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < held * 4; e += TAB_T) ls[e] = 0ull;
        for (int e = threadIdx.x; e < held * 6; e += TAB_T) {
            const int c = e % 6;
            le[e] = c == 0 ? w : c == 1 ? h : c == 2 ? d : -1;
        }
        __syncthreads();
    }
    RegionRun run = {};
    // the open run into the table: one update per column
    auto flush = [&]() {
        auto update = [&](u64* s, int* e, auto lds) {  // inlined once per address space: LDS and global atomics, no flat ones
            constexpr bool C = decltype(lds)::value;
            atomicAdd(s + 0, (u64)run.n);
            atomicAdd(s + 1, run.sx);
            atomicAdd(s + 2, run.sy);
            atomicAdd(s + 3, run.sz);
            tab_min<C>(e + 0, run.x0);
            tab_min<C>(e + 1, run.y0);
            tab_min<C>(e + 2, run.z0);
            tab_max<C>(e + 3, run.x1);
            tab_max<C>(e + 4, run.y1);
            tab_max<C>(e + 5, run.z1);
        };
        if (LDS && run.l < (unsigned)TAB_ROWS) update(ls + run.l * 4u, le + run.l * 6u, std::true_type());
        else update(sum + (size_t)run.l * 4, ext + (size_t)run.l * 6, std::false_type());
    };
    // n voxels of label l from (x0, y, z) along x: they extend the open run or close it and open the next
    auto push = [&](unsigned l, int x0, int n, int y, int z) {
        const u64 n64 = (u64)n, sx = n64 * (u64)x0 + (n64 * (n64 - 1ull)) / 2ull, sy = n64 * (u64)y, sz = n64 * (u64)z;
        const int x1 = x0 + n - 1;
        if (run.n && run.l == l) {
            run.n += (unsigned)n;
            run.sx += sx; run.sy += sy; run.sz += sz;
            run.x0 = min(run.x0, x0); run.y0 = min(run.y0, y); run.z0 = min(run.z0, z);
            run.x1 = max(run.x1, x1); run.y1 = max(run.y1, y); run.z1 = max(run.z1, z);
        } else {
            if (run.n) flush();
            run = {l, (unsigned)n, sx, sy, sz, x0, y, z, x1, y, z};
        }
    };
    const int nseg = (w + TAB_SEG - 1) / TAB_SEG;
    const Units un((int64_t)nseg * h * d);             // <= voxels < 2^31
    for (int64_t c = un.chunk; c < un.chunks; c += un.step) {
        for (int it = 0; it < TAB_CHUNK; ++it) {
            const int64_t u = un.unit(c, it);
            if (u >= un.units) break;
            const unsigned u32 = (unsigned)u;
            const int seg = (int)(u32 % (unsigned)nseg), r = (int)(u32 / (unsigned)nseg);
            const int y = r % h, z = r / h, x0 = seg * TAB_SEG, n = min(TAB_SEG, w - x0);
            const int64_t row = ((int64_t)z * h + y) * w + x0;
            unsigned v[TAB_SEG];
#pragma unroll
            for (int j = 0; j < TAB_SEG; ++j) v[j] = j < n ? tab_label(labels, bytes, row + j, L) : 0u;
            unsigned key = v[0];
            int start = 0;
#pragma unroll
            for (int j = 1; j < TAB_SEG; ++j) {
                if (j < n && v[j] != key) {
                    push(key, x0 + start, j - start, y, z);
                    key = v[j];
                    start = j;
                }
            }
            push(key, x0 + start, n - start, y, z);    // n >= 1: the unit's last stretch
        }
    }
    if (run.n) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int l = threadIdx.x; l < held; l += TAB_T) {
            const u64 cnt = ls[l * 4];
            if (cnt == 0ull) continue;                 // not touched by this block
            u64* s = sum + (size_t)l * 4;
            int* e = ext + (size_t)l * 6;
            atomicAdd(s + 0, cnt);
#pragma unroll
            for (int c = 1; c < 4; ++c) atomicAdd(s + c, ls[l * 4 + c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) tab_min<false>(e + c, le[l * 6 + c]);
#pragma unroll
            for (int c = 3; c < 6; ++c) tab_max<false>(e + c, le[l * 6 + c]);
        }
    }
}

// ---- overlap ---------------------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(TAB_T) k_table_overlap(const void* __restrict__ a, int a_bytes, const void* __restrict__ b, int b_bytes,
                                                         int64_t voxels, unsigned L, unsigned* cnt) {
    __shared__ unsigned lc[LDS ? TAB_ROWS * 3 : 1];
    const int held = min((int)L + 1, TAB_ROWS);
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < held * 3; e += TAB_T) lc[e] = 0u;
        __syncthreads();
    }
    auto add1 = [&](unsigned l, unsigned c, unsigned n) {
        if (LDS && l < (unsigned)TAB_ROWS) atomicAdd(&lc[l * 3u + c], n);
        else atomicAdd(cnt + (size_t)l * 3 + c, n);
    };
    unsigned open_key = 0u, open_n = 0u;               // the open run: n voxels where a reads key >> 16 and b reads key & 0xFFFF
    auto flush = [&]() {
        const unsigned la = open_key >> 16, lb = open_key & 0xFFFFu;
        add1(la, 0u, open_n);
        add1(lb, 1u, open_n);
        if (la == lb) add1(la, 2u, open_n);
    };
    auto push = [&](unsigned key, unsigned n) {
        if (open_n && open_key == key) {
            open_n += n;
        } else {
            if (open_n) flush();
            open_key = key;
            open_n = n;
        }
    };
    const Units un((voxels + TAB_SEG - 1) / TAB_SEG);
    for (int64_t c = un.chunk; c < un.chunks; c += un.step) {
        for (int it = 0; it < TAB_CHUNK; ++it) {
            const int64_t u = un.unit(c, it);
            if (u >= un.units) break;
            const int64_t i0 = u * TAB_SEG;
            const int n = (int)min((int64_t)TAB_SEG, voxels - i0);
            unsigned key[TAB_SEG];                     // (a << 16) | b
#pragma unroll
            for (int j = 0; j < TAB_SEG; ++j)
                key[j] = j < n ? (tab_label(a, a_bytes, i0 + j, L) << 16) | tab_label(b, b_bytes, i0 + j, L) : 0u;
            unsigned k = key[0];
            int start = 0;
#pragma unroll
            for (int j = 1; j < TAB_SEG; ++j) {
                if (j < n && key[j] != k) {
                    push(k, (unsigned)(j - start));
                    k = key[j];
                    start = j;
                }
            }
            push(k, (unsigned)(n - start));
        }
    }
    if (open_n) flush();
    if constexpr (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < held * 3; e += TAB_T)
            if (const unsigned c = lc[e]) atomicAdd(cnt + e, c);
    }
}

// the running table -> int64 rows; every entry is stored
__global__ void __launch_bounds__(TAB_T) k_table_widen(const u64* __restrict__ sum, const int* __restrict__ ext, const unsigned* __restrict__ cnt,
                                                       int rows, int64_t* __restrict__ out) {
    const int i = blockIdx.x * TAB_T + threadIdx.x;
    if (cnt) {                                         // overlap
        if (i < rows * 3) out[i] = (int64_t)cnt[i];
        return;
    }
    if (i >= rows * 10) return;
    const int l = i / 10, c = i % 10;
    out[i] = c < 4 ? (int64_t)sum[l * 4 + c] : (int64_t)ext[l * 6 + (c - 4)];
}

int tab_blocks(int64_t units) {
    const int64_t per = (int64_t)TAB_T * TAB_CHUNK, nb = (units + per - 1) / per;
    return (int)(nb > TAB_MAXB ? TAB_MAXB : nb < 1 ? 1 : nb);
}

}  // namespace

size_t table_scratch_bytes(int n_labels) { return 256 + tab_scratch(nullptr, n_labels).bytes; }

void launch_table_regions(const void* labels, int label_bytes, int w, int h, int d, int n_labels, int64_t* rows, int impl, void* scratch,
                          hipStream_t s) {
    const Scratch sc = tab_scratch(scratch, n_labels);
    const int R = n_labels + 1;
    k_table_init<<<(R * 6 + TAB_T - 1) / TAB_T, TAB_T, 0, s>>>(sc.sum, sc.ext, nullptr, R, w, h, d);
    const int nb = tab_blocks((int64_t)((w + TAB_SEG - 1) / TAB_SEG) * h * d);
    if (impl != UNET_TABLE_IMPL_GLOBAL)   // DEFAULT: LDS
        k_table_regions<true><<<nb, TAB_T, 0, s>>>(labels, label_bytes, w, h, d, (unsigned)n_labels, sc.sum, sc.ext);
    else
        k_table_regions<false><<<nb, TAB_T, 0, s>>>(labels, label_bytes, w, h, d, (unsigned)n_labels, sc.sum, sc.ext);
    k_table_widen<<<(R * 10 + TAB_T - 1) / TAB_T, TAB_T, 0, s>>>(sc.sum, sc.ext, nullptr, R, rows);
}

void launch_table_overlap(const void* a, int a_bytes, const void* b, int b_bytes, int64_t voxels, int n_labels, int64_t* rows, int impl,
                          void* scratch, hipStream_t s) {
    const Scratch sc = tab_scratch(scratch, n_labels);
    const int R = n_labels + 1;
    k_table_init<<<(R * 3 + TAB_T - 1) / TAB_T, TAB_T, 0, s>>>(nullptr, nullptr, sc.cnt, R, 0, 0, 0);
    const int nb = tab_blocks((voxels + TAB_SEG - 1) / TAB_SEG);
    if (impl != UNET_TABLE_IMPL_GLOBAL)
        k_table_overlap<true><<<nb, TAB_T, 0, s>>>(a, a_bytes, b, b_bytes, voxels, (unsigned)n_labels, sc.cnt);
    else
        k_table_overlap<false><<<nb, TAB_T, 0, s>>>(a, a_bytes, b, b_bytes, voxels, (unsigned)n_labels, sc.cnt);
    k_table_widen<<<(R * 3 + TAB_T - 1) / TAB_T, TAB_T, 0, s>>>(nullptr, nullptr, sc.cnt, R, rows);
}

}  // namespace unet
