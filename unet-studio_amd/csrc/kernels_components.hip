// A model's single_component_label (include/unet_components.h): every listed class of a uint16 label map keeps its largest
// 6-connected component, all listed classes in one labelling; include/unet_connectivity.h runs the same stages with 18- and
// 26-connectivity (CONN below; N-(CONN) is cc_for_backward's half neighbourhood, the three face neighbours for 6).
//
//   k_cmp_mark      flags[v] = 1 for the listed classes (the host list travels in the kernel arguments: no host copy to wait for)
//   TILED
//   k_cmp_tile      a block owns a TX x TY x TZ tile: it stages the tile's values in LDS (0 for a voxel that is not a member), builds
//                   the tile's union-find in LDS (a member hooks to every neighbour of N-(CONN) inside the tile that holds an
//                   equal value), walks every voxel to its tile-local root, counts the voxels per local root with LDS adds, and writes
//                   parent[i] = the GLOBAL linear index of the local root (-1 for non-members) and count[i] = the piece's voxels
//                   at a local root, 0 elsewhere.  A tile's local order and the global order are both (z, y, x) lexicographic, so
//                   the local root is the piece's smallest global index and parent[j] <= j holds for cc_find / cc_union
//   k_cmp_border    <6>: only the voxels on a low face of a tile: each hooks across the face to an equal-valued member with a
//                   global union.  It reads the label map at those voxels.  <18>, <26>: a backward neighbour can also lie across a
//                   HIGH x or y face (dx or dy = +1 with dz = -1, or dx = +1 with dy = -1) and across two or three faces at once,
//                   so the voxels on both sides of every interior x and y face and on the low side of every interior z face
//                   (x % TX in {0, TX-1}, y % TY in {0, TY-1}, z % TZ == 0) each hook every pair (v, v + o), o in N-(CONN), whose
//                   two voxels lie in different tiles.  A pair that crosses a tile boundary crosses one along some axis, where v
//                   is on the plane next to it: no pair is missed; a voxel on two planes is visited twice, which is harmless
//   GLOBAL
//   k_cmp_init      parent = i for members, -1 otherwise; count = 0
//   k_cmp_link      every member hooks to every neighbour of N-(CONN) of equal value with a global union (defragment's scheme)
//   both
//   k_cmp_flatten   <false> halves the paths; <true> walks every voxel to its root and writes it.  TILED adds a local root's
//                   piece count to its global root in that same pass (only global roots are added to, only non-roots add: no entry
//                   is read by one thread while another writes it); GLOBAL counts with cc_count_runs (k_cmp_count) afterwards
//   k_cmp_best      every root: best[class] = max over (count << 32) | (0xFFFFFFFF - root), a 64-bit integer maximum, so the largest
//                   count wins and among equal counts the smallest root, whatever the order of arrival
//   k_cmp_zero      a member whose root is not its class's best becomes 0; removed[class] counts them (block histogram in LDS for
//                   the classes below CMP_HIST, global adds above)
// Every atomic is an integer compare-and-swap, add or maximum: the result does not depend on the schedule.
// Everything up to and including the flatten passes is launch_components_label, which kernels_instances.hip shares.
//
// Scratch: parent int32[S], count uint32[S], best uint64[n_classes], flags uint8[n_classes], each 256-B aligned.
#include <stdexcept>
#include <string>

#include "../../include/unet_components.h"
#include "cc_union_find.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int CMP_T = 256;         // threads per block
constexpr int CMP_MAXB = 2048;     // grid cap of the streaming kernels; they stride over the rest
constexpr int TX = UNET_COMPONENTS_TILE_X, TY = UNET_COMPONENTS_TILE_Y, TZ = UNET_COMPONENTS_TILE_Z;
constexpr int TV = TX * TY * TZ;   // voxels per tile
constexpr int CMP_HIST = 2048;     // classes whose removed counts a block gathers in LDS
constexpr int CMP_CHUNK = 512;     // list entries per k_cmp_mark launch (2 KB of kernel arguments)
static_assert(TX * TY == CMP_T, "a thread owns one (x, y) column of the tile");

size_t cmp_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
    int* parent;
    unsigned* count;
    unsigned long long* best;
    uint8_t* flags;
    size_t table_bytes;   // best and flags, contiguous: zeroed by one memset
};
Scratch cmp_scratch(void* scratch, int64_t S, int n_classes) {
    char* b = (char*)cmp_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    s.parent = (int*)b;
    s.count = (unsigned*)(b + cmp_align((size_t)S * 4));
    s.best = (unsigned long long*)(b + 2 * cmp_align((size_t)S * 4));
    s.flags = (uint8_t*)s.best + cmp_align((size_t)n_classes * 8);
    s.table_bytes = cmp_align((size_t)n_classes * 8) + cmp_align((size_t)n_classes);
    return s;
}

int cmp_blocks(int64_t n, int per_block) {
    const int64_t nb = (n + per_block - 1) / per_block;
    return (int)(nb > CMP_MAXB ? CMP_MAXB : nb < 1 ? 1 : nb);
}

struct ListChunk {
    uint32_t v[CMP_CHUNK];
};

__global__ void __launch_bounds__(CMP_T) k_cmp_mark(uint8_t* __restrict__ flags, ListChunk chunk, int n) {
    for (int i = threadIdx.x; i < n; i += CMP_T) flags[chunk.v[i]] = 1;   // entries are checked on the host: 0 < v < n_classes
}

// ---- TILED ---------------------------------------------------------------------------------------------------------------------
template <int CONN>
__global__ void __launch_bounds__(CMP_T) k_cmp_tile(int W, int H, int D, int ntx, int nty, const uint16_t* __restrict__ label,
                                                    int n_classes, const uint8_t* __restrict__ flags, int* __restrict__ parent,
                                                    unsigned* __restrict__ count) {
    __shared__ uint16_t val[TV];     // the value of a member, 0 for everything else (class 0 is never listed)
    __shared__ int lpar[TV];         // the tile's forest over local indices l = (lz * TY + ly) * TX + lx
    __shared__ unsigned lcnt[TV];    // voxels per local root
    const int b = blockIdx.x;
    const int x0 = (b % ntx) * TX, y0 = ((b / ntx) % nty) * TY, z0 = (b / (ntx * nty)) * TZ;
    const int t = threadIdx.x, lx = t % TX, ly = t / TX;
    const int x = x0 + lx, y = y0 + ly;
    const bool inxy = x < W && y < H;
#pragma unroll
    for (int k = 0; k < TZ; ++k) {
        const int l = t + CMP_T * k;
        uint16_t v = 0;
        if (inxy && z0 + k < D) {
            const uint16_t u = label[((int64_t)(z0 + k) * H + y) * W + x];
            if ((int)u < n_classes && flags[u]) v = u;
        }
        val[l] = v;
        lpar[l] = v ? l : -1;
        lcnt[l] = 0u;
    }
    __syncthreads();
    // The LDS union-find.  cc_find: the index strictly decreases along a path (lpar[j] <= j), so the walk ends at a root.  cc_union:
    // a successful compare-and-swap ends its loop, having hooked the larger root onto the smaller; a failed one returns what
    // replaced the root, which is strictly smaller, so max(ra, rb) strictly decreases, bounded below by 0: every loop terminates
    // whatever the other threads do
    if constexpr (CONN == 6) {
#pragma unroll
        for (int k = 0; k < TZ; ++k) {
            const int l = t + CMP_T * k;
            const uint16_t v = val[l];
            if (!v) continue;
            if (lx > 0 && val[l - 1] == v) cc_union(lpar, l, l - 1);
            if (ly > 0 && val[l - TX] == v) cc_union(lpar, l, l - TX);
            if (k > 0 && val[l - CMP_T] == v) cc_union(lpar, l, l - CMP_T);
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < TZ; ++k) {   // not unrolled: 9 or 13 inlined unions per step
            const int l = t + CMP_T * k;
            const uint16_t v = val[l];
            if (!v) continue;
            cc_for_backward<CONN>([&](int dx, int dy, int dz) {
                // a neighbour outside the tile is k_cmp_border's; one outside the grid holds 0
                if (lx + dx < 0 || lx + dx >= TX || ly + dy < 0 || ly + dy >= TY || k + dz < 0) return;
                const int m = l + dx + dy * TX + dz * CMP_T;
                if (val[m] == v) cc_union(lpar, l, m);
            });
        }
    }
    __syncthreads();
    // nothing writes lpar from here on: a plain walk down to the root (r strictly decreases)
    int root[TZ];
    int cur = -1;
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < TZ; ++k) {
        const int l = t + CMP_T * k;
        int r = -1;
        if (val[l]) {
            int next;
            r = l;
            while (r > (next = lpar[r])) r = next;
        }
        root[k] = r;
        if (r != cur) {   // the column's runs of one root add once
            if (n) atomicAdd(&lcnt[cur], n);
            cur = r;
            n = 0;
        }
        n += r >= 0 ? 1u : 0u;
    }
    if (n) atomicAdd(&lcnt[cur], n);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TZ; ++k) {
        if (!(inxy && z0 + k < D)) continue;
        const int l = t + CMP_T * k, r = root[k];
        const int64_t g = ((int64_t)(z0 + k) * H + y) * W + x;
        int gr = -1;
        if (r >= 0) gr = (int)(((int64_t)(z0 + r / CMP_T) * H + (y0 + (r / TX) % TY)) * W + (x0 + r % TX));
        parent[g] = gr;
        count[g] = lcnt[l];
    }
}

// the voxels k_cmp_border<CONN> visits: per interior face the plane on its high side, and for 18 and 26 also the plane on the low
// side of an x or y face
template <int CONN>
int64_t border_voxels(int W, int H, int D, int nfx, int nfy, int nfz) {
    constexpr int sides = CONN == 6 ? 1 : 2;
    return sides * ((int64_t)nfx * H * D + (int64_t)W * nfy * D) + (int64_t)W * H * nfz;
}

// nfx, nfy, nfz: the interior tile faces per axis; the voxels of all of them, one section per axis, enumerated in closed form from
// the launch index
template <int CONN>
__global__ void __launch_bounds__(CMP_T) k_cmp_border(int W, int H, int D, int nfx, int nfy, int nfz, const uint16_t* __restrict__ label,
                                                      int* __restrict__ parent) {
    if constexpr (CONN != 6) {
        const int64_t A = 2 * (int64_t)nfx * H * D, B = 2 * (int64_t)W * nfy * D, total = A + B + (int64_t)W * H * nfz;
        const int WH = W * H;
        for (int64_t idx = (int64_t)blockIdx.x * CMP_T + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * CMP_T) {
            int x, y, z;
            if (idx < A) {          // x = TX * f - 1 and TX * f for the interior faces f = 1..nfx (all < W: TX * nfx < W)
                int64_t j = idx;
                const int q = (int)(j % (2 * nfx)); j /= 2 * nfx;
                x = (q / 2 + 1) * TX - 1 + (q & 1);
                y = (int)(j % H); z = (int)(j / H);
            } else if (idx < A + B) {
                int64_t j = idx - A;
                x = (int)(j % W); j /= W;
                const int q = (int)(j % (2 * nfy));
                y = (q / 2 + 1) * TY - 1 + (q & 1); z = (int)(j / (2 * nfy));
            } else {
                int64_t j = idx - A - B;
                x = (int)(j % W); j /= W;
                y = (int)(j % H); z = (int)(j / H + 1) * TZ;
            }
            const int i = (int)(((int64_t)z * H + y) * W + x);
            if (parent[i] < 0) continue;   // membership never changes: hooking only lowers values that are >= 0
            const uint16_t u = label[i];
            cc_for_backward<CONN>([&](int dx, int dy, int dz) {
                const int nx = x + dx, ny = y + dy, nz = z + dz;
                if (nx < 0 || nx >= W || ny < 0 || ny >= H || nz < 0) return;
                if (nx / TX == x / TX && ny / TY == y / TY && nz / TZ == z / TZ) return;   // the tile's own pair
                const int nb = i + dx + dy * W + dz * WH;
                if (parent[nb] >= 0 && label[nb] == u) cc_union(parent, i, nb);
            });
        }
        return;
    }
    const int64_t A = (int64_t)nfx * H * D, B = (int64_t)W * nfy * D, total = A + B + (int64_t)W * H * nfz;
    for (int64_t idx = (int64_t)blockIdx.x * CMP_T + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * CMP_T) {
        int x, y, z, back;
        if (idx < A) {
            int64_t j = idx;
            x = (int)(j % nfx + 1) * TX; j /= nfx;
            y = (int)(j % H); z = (int)(j / H);
            back = 1;
        } else if (idx < A + B) {
            int64_t j = idx - A;
            x = (int)(j % W); j /= W;
            y = (int)(j % nfy + 1) * TY; z = (int)(j / nfy);
            back = W;
        } else {
            int64_t j = idx - A - B;
            x = (int)(j % W); j /= W;
            y = (int)(j % H); z = (int)(j / H + 1) * TZ;
            back = W * H;
        }
        const int i = (int)(((int64_t)z * H + y) * W + x), nb = i - back;
        // membership never changes: hooking only lowers values that are >= 0
        if (parent[i] >= 0 && parent[nb] >= 0 && label[i] == label[nb]) cc_union(parent, i, nb);
    }
}

// ---- GLOBAL --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CMP_T) k_cmp_init(int64_t S, const uint16_t* __restrict__ label, int n_classes,
                                                    const uint8_t* __restrict__ flags, int* __restrict__ parent,
                                                    unsigned* __restrict__ count) {
    for (int64_t i = (int64_t)blockIdx.x * CMP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * CMP_T) {
        const uint16_t u = label[i];
        parent[i] = (int)u < n_classes && flags[u] ? (int)i : -1;
        count[i] = 0u;
    }
}

template <int CONN>
__global__ void __launch_bounds__(CMP_T) k_cmp_link(int W, int H, int S, const uint16_t* __restrict__ label, int* __restrict__ parent) {
    const int WH = W * H;
    for (int64_t i = (int64_t)blockIdx.x * CMP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * CMP_T) {
        if (parent[i] < 0) continue;
        const int v = (int)i, x = v % W, y = (v / W) % H;
        const uint16_t u = label[v];
        if constexpr (CONN == 6) {
            if (x > 0 && parent[v - 1] >= 0 && label[v - 1] == u) cc_union(parent, v, v - 1);
            if (y > 0 && parent[v - W] >= 0 && label[v - W] == u) cc_union(parent, v, v - W);
            if (v >= WH && parent[v - WH] >= 0 && label[v - WH] == u) cc_union(parent, v, v - WH);
        } else {
            cc_for_backward<CONN>([&](int dx, int dy, int dz) {
                if (x + dx < 0 || x + dx >= W || y + dy < 0 || y + dy >= H || (dz < 0 && v < WH)) return;
                const int nb = v + dx + dy * W + dz * WH;
                if (parent[nb] >= 0 && label[nb] == u) cc_union(parent, v, nb);
            });
        }
    }
}

__global__ void __launch_bounds__(CMP_T) k_cmp_count(int S, const int* __restrict__ parent, unsigned* __restrict__ count) {
    cc_count_runs<CMP_T>(S, parent, count);
}

// ---- both ----------------------------------------------------------------------------------------------------------------------
// FINAL == false: a pass that halves the paths (its stores race with other threads' halving, which may leave an entry at an ancestor
// that is not the root).  FINAL == true: a pass that only walks and writes each entry's own root, so nothing races; with ADD it also
// moves the piece count a tile-local root holds to its global root
template <bool FINAL, bool ADD>
__global__ void __launch_bounds__(CMP_T) k_cmp_flatten(int S, int* __restrict__ parent, unsigned* __restrict__ count) {
    for (int64_t i = (int64_t)blockIdx.x * CMP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * CMP_T) {
        const int p = cc_ld(parent + i);
        if (p < 0) continue;
        if constexpr (!FINAL) {
            cc_find(parent, (int)i);
        } else {
            int r = p, next;
            while (r > (next = cc_ld(parent + r))) r = next;
            if (r != p) cc_st(parent + i, r);
            if constexpr (ADD) {
                if (r != (int)i) {   // count[i] of a non-root is written by nobody else; only roots are added to
                    const unsigned c = count[i];
                    if (c) atomicAdd(count + r, c);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(CMP_T) k_cmp_best(int S, const uint16_t* __restrict__ label, const int* __restrict__ parent,
                                                    const unsigned* __restrict__ count, unsigned long long* __restrict__ best) {
    for (int64_t i = (int64_t)blockIdx.x * CMP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * CMP_T) {
        if (parent[i] != (int)i) continue;
        const unsigned long long key = ((unsigned long long)count[i] << 32) | (0xFFFFFFFFu - (unsigned)i);
        unsigned long long* slot = best + label[i];
        // the slot only grows, so a key that is not above what it holds now can never become the maximum
        if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, key);
    }
}

__global__ void __launch_bounds__(CMP_T) k_cmp_zero(int S, int n_classes, uint16_t* __restrict__ label, const int* __restrict__ parent,
                                                    const unsigned long long* __restrict__ best, unsigned* __restrict__ removed) {
    __shared__ unsigned hist[CMP_HIST];
    if (removed) {
        for (int c = threadIdx.x; c < CMP_HIST; c += CMP_T) hist[c] = 0u;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * CMP_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * CMP_T) {
        const int r = parent[i];
        if (r < 0) continue;
        const uint16_t c = label[i];
        if ((unsigned)r == 0xFFFFFFFFu - (unsigned)best[c]) continue;   // the low word: the kept root of the class
        label[i] = 0;
        if (removed) {
            if (c < CMP_HIST) atomicAdd(&hist[c], 1u);
            else atomicAdd(removed + c, 1u);
        }
    }
    if (removed) {
        __syncthreads();
        for (int c = threadIdx.x; c < CMP_HIST && c < n_classes; c += CMP_T)
            if (hist[c]) atomicAdd(removed + c, hist[c]);
    }
}

template <int CONN>
void cmp_hook(int W, int H, int D, int S, const uint16_t* label, int n_classes, int impl, const Scratch& sc, hipStream_t s) {
    const int nb = cmp_blocks(S, CMP_T);
    if (impl == UNET_COMPONENTS_IMPL_GLOBAL) {
        k_cmp_init<<<nb, CMP_T, 0, s>>>(S, label, n_classes, sc.flags, sc.parent, sc.count);
        k_cmp_link<CONN><<<nb, CMP_T, 0, s>>>(W, H, S, label, sc.parent);
    } else {
        const int ntx = (W + TX - 1) / TX, nty = (H + TY - 1) / TY, ntz = (D + TZ - 1) / TZ;   // ntx * nty * ntz <= S < 2^31
        k_cmp_tile<CONN><<<(unsigned)(ntx * nty * ntz), CMP_T, 0, s>>>(W, H, D, ntx, nty, label, n_classes, sc.flags, sc.parent, sc.count);
        const int nfx = ntx - 1, nfy = nty - 1, nfz = ntz - 1;
        const int64_t faces = border_voxels<CONN>(W, H, D, nfx, nfy, nfz);
        if (faces) k_cmp_border<CONN><<<cmp_blocks(faces, CMP_T), CMP_T, 0, s>>>(W, H, D, nfx, nfy, nfz, label, sc.parent);
    }
}

}  // namespace

size_t components_scratch_bytes(int64_t S, int n_classes) {
    return 256 + 2 * cmp_align((size_t)S * 4) + cmp_align((size_t)n_classes * 8) + cmp_align((size_t)n_classes);
}

// The labelling stage, shared with kernels_instances.hip and kernels_morph.hip: after it parent[v] is the smallest linear index of
// v's component (-1 for a voxel that is no member) and count[r] the component's voxels at every root r (elsewhere count is not
// meaningful).  classes: n sorted distinct entries in (0, n_classes), host memory; read before this returns.  n == 0: nothing is a
// member.  connectivity: 6, 18 or 26 (checked by the caller)
ComponentsForest launch_components_label(int W, int H, int D, const uint16_t* label, int n_classes, const uint32_t* classes, int n,
                                         int impl, int connectivity, void* scratch, hipStream_t s) {
    const int S = W * H * D;   // < 2^31 (checked by the caller)
    const Scratch sc = cmp_scratch(scratch, S, n_classes);
    ComponentsForest forest = {sc.parent, sc.count, (char*)sc.best + sc.table_bytes, sc.best};
    if (n == 0) {
        if (hipError_t e = hipMemsetAsync(sc.parent, 0xFF, (size_t)S * 4, s); e != hipSuccess)
            throw std::runtime_error(std::string("unet_components: hipMemsetAsync: ") + hipGetErrorString(e));
        return forest;
    }
    if (hipError_t e = hipMemsetAsync(sc.best, 0, sc.table_bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_components: hipMemsetAsync: ") + hipGetErrorString(e));
    for (int c0 = 0; c0 < n; c0 += CMP_CHUNK) {
        ListChunk chunk;
        const int m = n - c0 < CMP_CHUNK ? n - c0 : CMP_CHUNK;
        for (int i = 0; i < CMP_CHUNK; ++i) chunk.v[i] = i < m ? classes[c0 + i] : 0u;
        k_cmp_mark<<<1, CMP_T, 0, s>>>(sc.flags, chunk, m);
    }
    const int nb = cmp_blocks(S, CMP_T);
    if (connectivity == 26) cmp_hook<26>(W, H, D, S, label, n_classes, impl, sc, s);
    else if (connectivity == 18) cmp_hook<18>(W, H, D, S, label, n_classes, impl, sc, s);
    else cmp_hook<6>(W, H, D, S, label, n_classes, impl, sc, s);
    if (impl == UNET_COMPONENTS_IMPL_GLOBAL) {
        k_cmp_flatten<false, false><<<nb, CMP_T, 0, s>>>(S, sc.parent, sc.count);
        k_cmp_flatten<true, false><<<nb, CMP_T, 0, s>>>(S, sc.parent, sc.count);
        k_cmp_count<<<cmp_blocks(S, CMP_T * CC_RUN), CMP_T, 0, s>>>(S, sc.parent, sc.count);
    } else {
        k_cmp_flatten<false, false><<<nb, CMP_T, 0, s>>>(S, sc.parent, sc.count);
        k_cmp_flatten<true, true><<<nb, CMP_T, 0, s>>>(S, sc.parent, sc.count);
    }
    return forest;
}

// classes: as above
void launch_components_keep_largest(int W, int H, int D, uint16_t* label, int n_classes, const uint32_t* classes, int n,
                                    uint32_t* removed, int impl, int connectivity, void* scratch, hipStream_t s) {
    if (removed)
        if (hipError_t e = hipMemsetAsync(removed, 0, (size_t)n_classes * 4, s); e != hipSuccess)
            throw std::runtime_error(std::string("unet_components: hipMemsetAsync: ") + hipGetErrorString(e));
    if (n == 0) return;
    const int S = W * H * D;   // < 2^31 (checked by the caller)
    const ComponentsForest f = launch_components_label(W, H, D, label, n_classes, classes, n, impl, connectivity, scratch, s);
    const int nb = cmp_blocks(S, CMP_T);
    k_cmp_best<<<nb, CMP_T, 0, s>>>(S, label, f.parent, f.count, f.best);
    k_cmp_zero<<<nb, CMP_T, 0, s>>>(S, n_classes, label, f.parent, f.best, removed);
}

}  // namespace unet
