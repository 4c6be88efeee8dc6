// The atlas preparation of evaluate_unet::load_atlas (include/unet_atlas.h): tissue votes, majority, erase, region growing.
//
//   reclassify
//   k_atl_votes     grid-stride; a thread reads 8 voxels per step (one 16-byte load of the atlas, 8 or 16 bytes of tissue, or 8
//                   single tissue loads when the tissue pointer does not share the atlas's alignment), merges equal (a, t) keys in
//                   registers and issues one add per run: into the block's LDS table for the rows that fit, into votes otherwise.
//                   tissue_total goes through T LDS counters the same way.  The table is flushed with one global add per non-zero
//                   entry.  The elements before and after the 16-byte aligned body are handled one at a time by block 0.
//                   LDS == false: the same run merging, every add global
//   k_atl_majority  one thread per region: the first maximum of its row, and the row added to the T column sums of the block (LDS),
//                   flushed with one global add per non-zero column into covered
//   k_atl_erase     the same 8-voxel walk: a voxel of region a whose tissue differs from majority[a] becomes 0 (and, under PRESERVE,
//                   every voxel whose tissue reads 0); a vector is stored only when one of its voxels changed; erased[a] is gathered
//                   in LDS for a < LDS_ENTRIES, global adds above
//   grow
//   k_atl_mark      active[t] for the T tissues (the host flags travel in the kernel arguments: no host copy to wait for)
//   k_atl_init      word[i] = (round << 16) | label: label > 0 -> round 0; an active voxel with label 0 -> round 0xFFFF; every
//                   other voxel 0.  changed[0] = 1
//   k_atl_fill      round r, in place: returns at once when changed[r - 1] == 0.  An unfilled voxel counts the peers whose label is
//                   non-zero and whose round is below r; a word is one 4-byte store, so a voxel filled in this same round (round
//                   == r) is ignored whether or not its store has landed: the synchronous definition.  A fill sets changed[r]
//   k_atl_smooth    one synchronous smoothing round from one word buffer into the other
//   k_atl_finish    unpacks the labels into the atlas, counts filled[t] (round in 1..0xFFFE), and one block sums changed[1..] into
//                   info
// Every atomic is an integer add: the results do not depend on the schedule.
//
// Scratch, each part 256-B aligned: votes uint32[(R+1)*T], total uint32[256], covered uint32[256], majority uint8[R+1],
// active uint8[256], changed uint32[max_rounds + 1], word uint32[S] twice.
#include <stdexcept>
#include <string>

#include "../../include/unet_atlas.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int ATL_T = 256;                         // threads per block
constexpr int ATL_MAXB = 1024;                     // grid cap of the streaming kernels; they stride over the rest
constexpr int ATL_LDS = UNET_ATLAS_LDS_ENTRIES;    // votes / erased entries a block keeps in LDS
constexpr int ATL_MAXT = 256;                      // the largest n_tissues
constexpr unsigned ATL_UNFILLED = 0xFFFF0000u;     // an active voxel the fill has not reached
static_assert(ATL_T == ATL_MAXT, "k_atl_mark, k_atl_smooth and k_atl_finish give every possible tissue one thread");

size_t atl_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    uint32_t* votes;
    uint32_t* total;
    uint32_t* covered;
    uint8_t* majority;
    uint8_t* active;
    uint32_t* changed;
    uint32_t* word[2];
    size_t bytes;   // from the aligned base
};
Scratch atl_scratch(void* scratch, int64_t S, int R, int T, int max_rounds) {
    char* b = (char*)atl_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    size_t o = 0;
    s.votes = (uint32_t*)(b + o);   o += atl_align((size_t)(R + 1) * T * 4);
    s.total = (uint32_t*)(b + o);   o += atl_align(ATL_MAXT * 4);
    s.covered = (uint32_t*)(b + o); o += atl_align(ATL_MAXT * 4);
    s.majority = (uint8_t*)(b + o); o += atl_align((size_t)R + 1);
    s.active = (uint8_t*)(b + o);   o += atl_align(ATL_MAXT);
    s.changed = (uint32_t*)(b + o); o += atl_align(((size_t)max_rounds + 1) * 4);
    s.word[0] = (uint32_t*)(b + o); o += atl_align((size_t)S * 4);
    s.word[1] = (uint32_t*)(b + o); o += atl_align((size_t)S * 4);
    s.bytes = o;
    return s;
}

int atl_blocks(int64_t n, int per_block) {
    const int64_t nb = (n + per_block - 1) / per_block;
    return (int)(nb > ATL_MAXB ? ATL_MAXB : nb < 1 ? 1 : nb);
}

// the tissue as read: a value >= T reads as 0 under CLAMP
__device__ __forceinline__ unsigned atl_tissue(unsigned raw, int T, int flags) {
    return (flags & UNET_ATLAS_CLAMP) && raw >= (unsigned)T ? 0u : raw;
}
// the atlas as read: 0 where the tissue reads 0 under PRESERVE
__device__ __forceinline__ unsigned atl_label(unsigned raw, unsigned t, int flags) {
    return (flags & UNET_ATLAS_PRESERVE) && t == 0u ? 0u : raw;
}

template <typename TT> __device__ __forceinline__ unsigned atl_ld(const void* tissue, int64_t i) { return ((const TT*)tissue)[i]; }

// 8 consecutive voxels from element `base` on (the atlas is 16-byte aligned there).  TVEC: the tissue is aligned for one vector
// load there as well (8 B for uint8, 16 B for uint16); otherwise it is read one element at a time
template <typename TT, bool TVEC>
__device__ __forceinline__ void atl_load8(const void* __restrict__ tissue, const uint16_t* atlas, int64_t base, unsigned (&a)[8],
                                          unsigned (&t)[8]) {
    const uint4 av = *(const uint4*)(atlas + base);
    const unsigned aw[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (aw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    if constexpr (!TVEC) {
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = atl_ld<TT>(tissue, base + j);
    } else if constexpr (sizeof(TT) == 1) {
        const uint2 tv = *(const uint2*)((const uint8_t*)tissue + base);
        const unsigned tw[2] = {tv.x, tv.y};
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (tw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
    } else {
        const uint4 tv = *(const uint4*)((const uint16_t*)tissue + base);
        const unsigned tw[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (tw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    }
}

// A run of equal keys in registers: push() adds to the open run or hands the closed one to add(key, n)
struct Run {
    unsigned key, n;
    template <typename Add> __device__ __forceinline__ void push(unsigned k, Add add) {
        if (k == key) {
            ++n;
        } else {
            if (n) add(key, n);
            key = k;
            n = 1u;
        }
    }
    template <typename Add> __device__ __forceinline__ void close(Add add) {
        if (n) add(key, n);
        n = 0u;
    }
};

// The walk every streaming reclassify kernel makes: `head` single elements, nvec vectors of 8 from element head on, then the tail.
// Block 0 takes the head and the tail, one element per thread (head, tail < 8)
template <typename TT, bool TVEC, typename One, typename Eight>
__device__ __forceinline__ void atl_walk(int64_t S, int head, const void* __restrict__ tissue, const uint16_t* atlas, One one,
                                         Eight eight) {
    const int64_t nvec = (S - head) >> 3;
    for (int64_t v = (int64_t)blockIdx.x * ATL_T + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * ATL_T) {
        unsigned a[8], t[8];
        const int64_t base = head + (v << 3);
        atl_load8<TT, TVEC>(tissue, atlas, base, a, t);
        eight(base, a, t);
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + (nvec << 3);
        const int n_single = head + (int)(S - tail0);   // < 16
        if ((int)threadIdx.x < n_single) {
            const int64_t i = (int)threadIdx.x < head ? (int64_t)threadIdx.x : tail0 + ((int)threadIdx.x - head);
            one(i, (unsigned)atlas[i], atl_ld<TT>(tissue, i));
        }
    }
}

// ---- reclassify ------------------------------------------------------------------------------------------------------------------
template <typename TT, bool TVEC, bool LDS>
__global__ void __launch_bounds__(ATL_T) k_atl_votes(int64_t S, int head, const void* __restrict__ tissue,
                                                     const uint16_t* __restrict__ atlas, int R, int T, int flags,
                                                     uint32_t* __restrict__ votes, uint32_t* __restrict__ total) {
    __shared__ unsigned lv[LDS ? ATL_LDS : 1];
    __shared__ unsigned lt[LDS ? ATL_MAXT : 1];
    // whole rows only: the entries below fit live in LDS.  fit <= ATL_LDS and fit <= (R + 1) * T
    const unsigned rows = min((unsigned)(ATL_LDS / T), (unsigned)R + 1u), fit = LDS ? rows * (unsigned)T : 0u;
    if constexpr (LDS) {
        for (unsigned e = threadIdx.x; e < fit; e += ATL_T) lv[e] = 0u;
        for (int e = threadIdx.x; e < T; e += ATL_T) lt[e] = 0u;
        __syncthreads();
    }
    auto add_vote = [&](unsigned key, unsigned n) {
        if (LDS && key < fit) atomicAdd(&lv[key], n);
        else atomicAdd(votes + key, n);
    };
    auto add_total = [&](unsigned key, unsigned n) {
        if constexpr (LDS) atomicAdd(&lt[key], n);
        else atomicAdd(total + key, n);
    };
    Run rv = {0u, 0u}, rt = {0u, 0u};
    auto voxel = [&](unsigned a_raw, unsigned t_raw) {
        const unsigned t = atl_tissue(t_raw, T, flags), a = atl_label(a_raw, t, flags);
        if (t < (unsigned)T) {
            rt.push(t, add_total);
            if (a - 1u < (unsigned)R) rv.push(a * (unsigned)T + t, add_vote);   // 1 <= a <= R
        }
    };
    atl_walk<TT, TVEC>(
        S, head, tissue, atlas, [&](int64_t, unsigned a, unsigned t) { voxel(a, t); },
        [&](int64_t, const unsigned(&a)[8], const unsigned(&t)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) voxel(a[j], t[j]);
        });
    rv.close(add_vote);
    rt.close(add_total);
    if constexpr (LDS) {
        __syncthreads();
        for (unsigned e = threadIdx.x; e < fit; e += ATL_T)
            if (const unsigned n = lv[e]) atomicAdd(votes + e, n);
        for (int e = threadIdx.x; e < T; e += ATL_T)
            if (const unsigned n = lt[e]) atomicAdd(total + e, n);
    }
}

__global__ void __launch_bounds__(ATL_T) k_atl_majority(int R, int T, const uint32_t* __restrict__ votes, uint8_t* __restrict__ majority,
                                                        uint32_t* __restrict__ covered) {
    __shared__ unsigned col[ATL_MAXT];
    for (int e = threadIdx.x; e < T; e += ATL_T) col[e] = 0u;
    __syncthreads();
    const int a = blockIdx.x * ATL_T + threadIdx.x;   // the grid covers 0..R exactly once
    if (a <= R) {
        const uint32_t* row = votes + (size_t)a * T;
        unsigned best = 0u, best_n = row[0];
        if (best_n) atomicAdd(&col[0], best_n);
        for (int t = 1; t < T; ++t) {
            const unsigned n = row[t];
            if (n > best_n) { best_n = n; best = (unsigned)t; }   // strictly larger: the first maximum stays
            if (n) atomicAdd(&col[t], n);
        }
        majority[a] = (uint8_t)best;                  // row 0 is all zero: 0
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T; e += ATL_T)
        if (const unsigned n = col[e]) atomicAdd(covered + e, n);
}

template <typename TT, bool TVEC, bool LDS>
__global__ void __launch_bounds__(ATL_T) k_atl_erase(int64_t S, int head, const void* __restrict__ tissue, uint16_t* __restrict__ atlas,
                                                     int R, int T, int flags, const uint8_t* __restrict__ majority,
                                                     uint32_t* __restrict__ erased) {
    __shared__ unsigned le[LDS ? ATL_LDS : 1];
    const unsigned fit = LDS ? min((unsigned)ATL_LDS, (unsigned)R + 1u) : 0u;
    const bool write = !(flags & UNET_ATLAS_COUNT_ONLY);
    if constexpr (LDS) {
        if (erased) {
            for (unsigned e = threadIdx.x; e < fit; e += ATL_T) le[e] = 0u;
            __syncthreads();
        }
    }
    auto add = [&](unsigned key, unsigned n) {
        if (LDS && key < fit) atomicAdd(&le[key], n);
        else atomicAdd(erased + key, n);
    };
    Run re = {0u, 0u};
    unsigned last_a = 0u, last_m = 0u;   // the majority of the region seen last: solid regions repeat it
    // the value the voxel holds afterwards
    auto voxel = [&](unsigned a_raw, unsigned t_raw) -> unsigned {
        const unsigned t = atl_tissue(t_raw, T, flags), a = atl_label(a_raw, t, flags);
        if (a - 1u >= (unsigned)R) return a;          // 0, or above R: never counted; only PRESERVE may have changed it
        if (a != last_a) { last_a = a; last_m = majority[a]; }
        if (t == last_m) return a;
        if (erased) re.push(a, add);
        return 0u;
    };
    atl_walk<TT, TVEC>(
        S, head, tissue, atlas,
        [&](int64_t i, unsigned a, unsigned t) {
            const unsigned b = voxel(a, t);
            if (write && b != a) atlas[i] = (uint16_t)b;
        },
        [&](int64_t base, const unsigned(&a)[8], const unsigned(&t)[8]) {
            unsigned b[8];
            bool any = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                b[j] = voxel(a[j], t[j]);
                any |= b[j] != a[j];
            }
            if (write && any)
                *(uint4*)(atlas + base) = make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
        });
    if (erased) {
        re.close(add);
        if constexpr (LDS) {
            __syncthreads();
            for (unsigned e = threadIdx.x; e < fit; e += ATL_T)
                if (const unsigned n = le[e]) atomicAdd(erased + e, n);
        }
    }
}

// ---- grow ------------------------------------------------------------------------------------------------------------------------
struct GrowFlags {
    uint8_t v[ATL_MAXT];
};

__global__ void __launch_bounds__(ATL_T) k_atl_mark(uint8_t* __restrict__ active, GrowFlags g, int T, int flags) {
    const int t = threadIdx.x;   // ATL_T == ATL_MAXT: one thread per possible tissue
    active[t] = t < T && g.v[t] && !((flags & UNET_ATLAS_PRESERVE) && t == 0) ? 1 : 0;
}

template <typename TT>
__global__ void __launch_bounds__(ATL_T) k_atl_init(int S, const void* __restrict__ tissue, const uint16_t* __restrict__ atlas, int T,
                                                    int flags, const uint8_t* __restrict__ active, uint32_t* __restrict__ word,
                                                    uint32_t* __restrict__ changed) {
    if (blockIdx.x == 0 && threadIdx.x == 0) changed[0] = 1u;
    for (int64_t i = (int64_t)blockIdx.x * ATL_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * ATL_T) {
        const unsigned t = atl_tissue(atl_ld<TT>(tissue, i), T, flags), a = atl_label(atlas[i], t, flags);
        word[i] = a ? a : (t < (unsigned)T && active[t] ? ATL_UNFILLED : 0u);
    }
}

// The face neighbours of voxel i inside the volume whose tissue reads t: f(neighbour index) for each
template <typename TT, typename F>
__device__ __forceinline__ void atl_peers(int W, int H, int D, int i, unsigned t, const void* __restrict__ tissue, int T, int flags, F f) {
    const int x = i % W, y = (i / W) % H, z = i / (W * H), WH = W * H;
    const int nb[6] = {i - 1, i + 1, i - W, i + W, i - WH, i + WH};
    const bool in[6] = {x > 0, x + 1 < W, y > 0, y + 1 < H, z > 0, z + 1 < D};
#pragma unroll
    for (int k = 0; k < 6; ++k)
        f(k, in[k] && atl_tissue(atl_ld<TT>(tissue, in[k] ? nb[k] : i), T, flags) == t, in[k] ? nb[k] : i);
}

// the most frequent non-zero entry of lab[0..N), the smallest among equal counts; 0 when all are 0.  count receives its frequency
template <int N> __device__ __forceinline__ unsigned atl_mode(const unsigned (&lab)[N], unsigned& count) {
    unsigned best = 0u, best_n = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        unsigned n = 0u;
#pragma unroll
        for (int k = 0; k < N; ++k) n += lab[k] == lab[j] ? 1u : 0u;
        if (lab[j] && (n > best_n || (n == best_n && lab[j] < best))) { best_n = n; best = lab[j]; }
    }
    count = best_n;
    return best;
}

template <typename TT>
__global__ void __launch_bounds__(ATL_T) k_atl_fill(int W, int H, int D, const void* __restrict__ tissue, int T, int flags, unsigned r,
                                                    uint32_t* word, uint32_t* __restrict__ changed) {
    if (changed[r - 1] == 0u) return;   // the round before filled nothing: the fill has ended
    const int S = W * H * D;
    for (int64_t i64 = (int64_t)blockIdx.x * ATL_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * ATL_T) {
        const int i = (int)i64;
        if (__hip_atomic_load(word + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ATL_UNFILLED) continue;
        const unsigned t = atl_tissue(atl_ld<TT>(tissue, i), T, flags);
        unsigned lab[6];
        atl_peers<TT>(W, H, D, i, t, tissue, T, flags, [&](int k, bool peer, int n) {
            const unsigned w = peer ? __hip_atomic_load(word + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            lab[k] = (w >> 16) < r ? (w & 0xFFFFu) : 0u;   // labelled before this round; an unfilled word's label is 0 anyway
        });
        unsigned n;
        const unsigned m = atl_mode<6>(lab, n);
        if (m) {
            __hip_atomic_store(word + i, (r << 16) | m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            changed[r] = 1u;
        }
    }
}

template <typename TT>
__global__ void __launch_bounds__(ATL_T) k_atl_smooth(int W, int H, int D, const void* __restrict__ tissue, int T, int flags,
                                                      const uint8_t* __restrict__ active, const uint32_t* __restrict__ src,
                                                      uint32_t* __restrict__ dst, uint32_t* __restrict__ relabelled) {
    __shared__ unsigned lr[ATL_MAXT];
    if (relabelled) {
        lr[threadIdx.x] = 0u;
        __syncthreads();
    }
    const int S = W * H * D;
    for (int64_t i64 = (int64_t)blockIdx.x * ATL_T + threadIdx.x; i64 < S; i64 += (int64_t)gridDim.x * ATL_T) {
        const int i = (int)i64;
        unsigned w = src[i];
        const unsigned L = w & 0xFFFFu;
        if (L) {
            const unsigned t = atl_tissue(atl_ld<TT>(tissue, i), T, flags);
            if (t < (unsigned)T && active[t]) {
                unsigned lab[7];
                lab[6] = L;
                atl_peers<TT>(W, H, D, i, t, tissue, T, flags, [&](int k, bool peer, int n) { lab[k] = peer ? src[n] & 0xFFFFu : 0u; });
                unsigned nm, nl = 0u;
                const unsigned m = atl_mode<7>(lab, nm);
#pragma unroll
                for (int k = 0; k < 7; ++k) nl += lab[k] == L ? 1u : 0u;
                if (nm > nl) {
                    w = (w & 0xFFFF0000u) | m;
                    if (relabelled) atomicAdd(&lr[t], 1u);
                }
            }
        }
        dst[i] = w;
    }
    if (relabelled) {
        __syncthreads();
        if ((int)threadIdx.x < T && lr[threadIdx.x]) atomicAdd(relabelled + threadIdx.x, lr[threadIdx.x]);
    }
}

template <typename TT>
__global__ void __launch_bounds__(ATL_T) k_atl_finish(int S, const void* __restrict__ tissue, int T, int flags,
                                                      const uint32_t* __restrict__ word, uint16_t* __restrict__ atlas,
                                                      const uint32_t* __restrict__ changed, int max_rounds, uint32_t* __restrict__ filled,
                                                      uint32_t* __restrict__ info) {
    __shared__ unsigned lf[ATL_MAXT];
    lf[threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * ATL_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * ATL_T) {
        const unsigned w = word[i], r = w >> 16;
        atlas[i] = (uint16_t)(w & 0xFFFFu);
        if (filled && r - 1u < 0xFFFEu) {   // filled by round r; it was active, so its tissue is below T
            const unsigned t = atl_tissue(atl_ld<TT>(tissue, i), T, flags);
            if (t < (unsigned)T) atomicAdd(&lf[t], 1u);
        }
    }
    __syncthreads();
    if (filled && (int)threadIdx.x < T && lf[threadIdx.x]) atomicAdd(filled + threadIdx.x, lf[threadIdx.x]);
    if (info && blockIdx.x == 0) {   // changed is 1 up to the last round that filled something and 0 from there on
        __syncthreads();
        lf[threadIdx.x] = 0u;
        __syncthreads();
        unsigned n = 0u;
        for (int r = 1 + threadIdx.x; r <= max_rounds; r += ATL_T) n += changed[r];
        if (n) atomicAdd(&lf[0], n);
        __syncthreads();
        if (threadIdx.x == 0) {
            info[0] = lf[0];
            info[1] = changed[max_rounds] == 0u ? 1u : 0u;   // some round up to max_rounds filled nothing (changed[0] is 1)
        }
    }
}

void atl_zero(void* p, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, 0, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_atlas: hipMemsetAsync: ") + hipGetErrorString(e));
}

// the elements before the atlas's first 16-byte boundary
int atl_head(const uint16_t* atlas, int64_t S) {
    const int64_t h = (int64_t)(((16 - ((uintptr_t)atlas & 15)) & 15) >> 1);
    return (int)(h < S ? h : S);
}

template <typename TT, bool TVEC>
void atl_reclassify(int64_t S, int head, const void* tissue, uint16_t* atlas, int R, int T, int flags, uint32_t* votes, uint32_t* total,
                    uint32_t* covered, uint8_t* majority, uint32_t* erased, bool lds, hipStream_t s) {
    const int nb = atl_blocks((S - head) >> 3, ATL_T);
    if (lds) k_atl_votes<TT, TVEC, true><<<nb, ATL_T, 0, s>>>(S, head, tissue, atlas, R, T, flags, votes, total);
    else k_atl_votes<TT, TVEC, false><<<nb, ATL_T, 0, s>>>(S, head, tissue, atlas, R, T, flags, votes, total);
    k_atl_majority<<<R / ATL_T + 1, ATL_T, 0, s>>>(R, T, votes, majority, covered);
    if (R == 0 && !(flags & UNET_ATLAS_PRESERVE)) return;   // no region: nothing to erase and nothing to preserve
    if ((flags & UNET_ATLAS_COUNT_ONLY) && !erased) return;
    if (lds) k_atl_erase<TT, TVEC, true><<<nb, ATL_T, 0, s>>>(S, head, tissue, atlas, R, T, flags, majority, erased);
    else k_atl_erase<TT, TVEC, false><<<nb, ATL_T, 0, s>>>(S, head, tissue, atlas, R, T, flags, majority, erased);
}

template <typename TT>
void atl_grow(int W, int H, int D, const void* tissue, uint16_t* atlas, int T, int flags, int max_rounds, int smooth_rounds,
              uint32_t* filled, uint32_t* relabelled, uint32_t* info, const Scratch& sc, hipStream_t s) {
    const int S = W * H * D, nb = atl_blocks(S, ATL_T);
    k_atl_init<TT><<<nb, ATL_T, 0, s>>>(S, tissue, atlas, T, flags, sc.active, sc.word[0], sc.changed);
    for (int r = 1; r <= max_rounds; ++r) k_atl_fill<TT><<<nb, ATL_T, 0, s>>>(W, H, D, tissue, T, flags, (unsigned)r, sc.word[0], sc.changed);
    int cur = 0;
    for (int k = 0; k < smooth_rounds; ++k, cur ^= 1)
        k_atl_smooth<TT><<<nb, ATL_T, 0, s>>>(W, H, D, tissue, T, flags, sc.active, sc.word[cur], sc.word[cur ^ 1], relabelled);
    k_atl_finish<TT><<<nb, ATL_T, 0, s>>>(S, tissue, T, flags, sc.word[cur], atlas, sc.changed, max_rounds, filled, info);
}

}  // namespace

size_t atlas_scratch_bytes(int64_t S, int R, int T, int max_rounds) { return 256 + atl_scratch(nullptr, S, R, T, max_rounds).bytes; }

void launch_atlas_reclassify(int64_t S, const void* tissue, int tissue_bytes, uint16_t* atlas, int R, int T, int flags, uint32_t* votes,
                             uint32_t* total, uint32_t* covered, uint8_t* majority, uint32_t* erased, int impl, void* scratch,
                             hipStream_t s) {
    const Scratch sc = atl_scratch(scratch, 1, R, T, 0);   // the tables only
    if (!votes) votes = sc.votes;
    if (!total) total = sc.total;
    if (!covered) covered = sc.covered;
    if (!majority) majority = sc.majority;
    atl_zero(votes, (size_t)(R + 1) * T * 4, s);
    atl_zero(total, (size_t)T * 4, s);
    atl_zero(covered, (size_t)T * 4, s);
    if (erased) atl_zero(erased, ((size_t)R + 1) * 4, s);
    const int head = atl_head(atlas, S);
    const bool lds = impl != UNET_ATLAS_IMPL_GLOBAL;   // DEFAULT: LDS
    // one vector load of the tissue per 8 voxels needs the tissue aligned where the atlas is
    const bool tvec = (((uintptr_t)tissue + (size_t)head * tissue_bytes) & (size_t)(8 * tissue_bytes - 1)) == 0;
#define ATL_GO(TT, TVEC) atl_reclassify<TT, TVEC>(S, head, tissue, atlas, R, T, flags, votes, total, covered, majority, erased, lds, s)
    if (tissue_bytes == 1) { if (tvec) ATL_GO(uint8_t, true); else ATL_GO(uint8_t, false); }
    else { if (tvec) ATL_GO(uint16_t, true); else ATL_GO(uint16_t, false); }
#undef ATL_GO
}

// grow: T host flags, read before this returns
void launch_atlas_grow(int W, int H, int D, const void* tissue, int tissue_bytes, uint16_t* atlas, int T, int flags, const uint8_t* grow,
                       int max_rounds, int smooth_rounds, uint32_t* filled, uint32_t* relabelled, uint32_t* info, void* scratch,
                       hipStream_t s) {
    const Scratch sc = atl_scratch(scratch, (int64_t)W * H * D, 0, T, max_rounds);
    GrowFlags g;
    for (int t = 0; t < ATL_MAXT; ++t) g.v[t] = t < T ? grow[t] : 0;
    atl_zero(sc.changed, ((size_t)max_rounds + 1) * 4, s);
    if (filled) atl_zero(filled, (size_t)T * 4, s);
    if (relabelled) atl_zero(relabelled, (size_t)T * 4, s);
    k_atl_mark<<<1, ATL_T, 0, s>>>(sc.active, g, T, flags);
    if (tissue_bytes == 1)
        atl_grow<uint8_t>(W, H, D, tissue, atlas, T, flags, max_rounds, smooth_rounds, filled, relabelled, info, sc, s);
    else
        atl_grow<uint16_t>(W, H, D, tissue, atlas, T, flags, max_rounds, smooth_rounds, filled, relabelled, info, sc, s);
}

}  // namespace unet
