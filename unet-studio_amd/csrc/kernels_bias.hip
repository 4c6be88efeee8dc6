// The intensity-inhomogeneity correction (include/unet_bias.h): a Q12 log2 field on unet_warp.h's lattice, fitted node by node to
// the int16 residual of the voxels whose tissue is taken to be uniform, and removed by one rounded multiply per voxel.  The lattice,
// a node's support and a voxel's owner are lattice_field.h's; the field has one component and the node update is a closed-form
// integer minimiser, so the sweeps are this file's own.
//
//   k_bias_logcode   a thread per voxel: the float's exponent and 16 squarings of its mantissa
//   k_bias_levels    grid-stride over the voxels; a thread keeps {sum, count} of the K classes in registers (unrolled: no indexing),
//                    a wave reduces them by lane shuffles, the block's waves through LDS, one 64-bit add per block per quantity
//   k_bias_close     one block: m_t = floor(sum / count) per class
//   k_bias_residual  a thread per voxel: the levels staged in LDS, r = q - m_t or "skip"
//   k_bias_node      IMPL_NODE, one colour pass: a block of NT threads (64 = one wave for g = 4, 256 for g = 8, 1024 above) per node of
//                    the colour.  The node's 3x3x3 neighbourhood of B is staged in LDS (27 ints).  A work item is an aligned 16-byte
//                    run of the residual inside one row of the support: one int4 load, the row's three x-node values of n formed once
//                    from LDS (12 reads), then per voxel two multiplies for n and one 32 x 32 -> 64 multiply-add for W * e.  S1 and
//                    S2 are int64 in registers, reduced by lane shuffles, then across waves through LDS; thread 0 updates the node
//   k_bias_vox       IMPL_VOXEL, one colour pass: a thread per voxel finds the one node of the colour whose support holds it and adds
//                    W * e and W * W into the node's two 64-bit counters in the scratch
//   k_bias_update    IMPL_VOXEL: a thread per node of the colour: the update, and the counters zeroed again
//   k_bias_cost      as k_bias_levels, two quantities
//   k_bias_row       one thread: a (level, round)'s report row from the sweeps' counts; the cost pass adds into its tail
//   k_bias_refine    a thread per fine node
//   k_bias_apply     a thread per voxel: c from n, T[c & 4095] from the table in global memory (neighbouring voxels read
//                    neighbouring entries: the field is smooth), one multiply, one scaling
// Every atomic is an integer add: the results do not depend on the schedule.  In a fit every sweep's kernels return at once when
// `prev`, the count of nodes the preceding sweep of the same round changed, is zero (stream order makes it final).
//
// Scratch, each part 256-B aligned: the sweeps' {changed, visited} slots, the levels, the residual, the counters of IMPL_VOXEL (2
// per node of the finest lattice), the fields of all levels but the last.
#include <stdexcept>
#include <string>

#include "../../include/unet_bias.h"
#include "bias_table.h"
#include "kernels.h"
#include "lattice_field.h"

namespace unet {

namespace {

constexpr int BIAS_T = 256;          // threads per block of the per-voxel kernels
constexpr int BIAS_MAXB = 8192;      // their grid cap; they stride over the rest
constexpr int BIAS_REDB = 1024;      // the grid cap of the kernels that end in one atomic per block
constexpr int BIAS_MAXK = UNET_BIAS_MAX_CLASSES;
constexpr int BIAS_SLOTS = UNET_BIAS_MAX_ROWS * UNET_BIAS_MAX_SWEEPS;
constexpr int BIAS_NONE = UNET_BIAS_NONE;
constexpr int BIAS_SKIP = UNET_BIAS_SKIP;
typedef unsigned long long u64;
typedef long long i64;

__device__ const float bias_table[4096] = {BIAS_TABLE_VALUES};

struct BiasClasses {
    int v[BIAS_MAXK];
    int K;
};
struct BiasGrid {
    int sw, sh, sd;
};

// a label as read: uint8 or uint16 at any alignment
__device__ __forceinline__ unsigned bias_label(const void* __restrict__ p, int bytes, int64_t i) {
    return bytes == 1 ? (unsigned)((const uint8_t*)p)[i]
                      : (unsigned)((const uint8_t*)p)[2 * i] | ((unsigned)((const uint8_t*)p)[2 * i + 1] << 8);
}
// the class of a label, -1 for none (the classes are distinct: at most one matches)
__device__ __forceinline__ int bias_class(unsigned label, const BiasClasses& c) {
    int t = -1;
#pragma unroll
    for (int k = 0; k < BIAS_MAXK; ++k)
        if (k < c.K && c.v[k] == (int)label) t = k;
    return t;
}
__device__ __forceinline__ int bias_code(float v) {
    const unsigned b = __float_as_uint(v), ex = (b >> 23) & 0xFFu;
    if ((b >> 31) || ex == 0u || ex == 255u) return BIAS_NONE;
    unsigned x = ((b & 0x7FFFFFu) | 0x800000u) << 8, f = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const u64 y = ((u64)x * x) >> 31;
        if (y >> 32) {
            f = 2u * f + 1u;
            x = (unsigned)(y >> 1);
        } else {
            f = 2u * f;
            x = (unsigned)y;
        }
    }
    return (((int)ex - 127) * 65536 + (int)f) >> 4;
}
// n of voxel (x, y, z) from global memory; a corner of weight 0 is not read
__device__ __forceinline__ int bias_n(const int32_t* __restrict__ B, const WarpLat& L, int x, int y, int z) {
    const int g = L.g, m = g - 1, cx = x >> L.lg, cy = y >> L.lg, cz = z >> L.lg, fx = x & m, fy = y & m, fz = z & m;
    int n = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int w = ((c & 1) ? fx : g - fx) * ((c & 2) ? fy : g - fy) * ((c & 4) ? fz : g - fz);
        if (w) n += w * B[((size_t)(cz + (c >> 2)) * L.ny + (cy + ((c >> 1) & 1))) * L.nx + (cx + (c & 1))];
    }
    return n;
}
__device__ __forceinline__ i64 bias_floor_div(i64 a, i64 b) {   // b > 0
    i64 q = a / b;
    if (a % b < 0) --q;
    return q;
}
// a wave's sum in lane 0
__device__ __forceinline__ i64 bias_wave_sum(i64 s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}
// The update of a node at b0: S1, S2 its sums, dsum the sum of (B_nbr - b0) over its nbrs neighbours, Lam = lam * g^6.  Returns the
// node's new value; visited says whether den > 0
__device__ __forceinline__ int bias_update(int b0, i64 S1, i64 S2, i64 dsum, int nbrs, i64 Lam, bool& visited) {
    const i64 num = S1 + Lam * dsum, den = S2 + Lam * nbrs;
    visited = den > 0;
    if (!visited) return b0;
    i64 nb = (i64)b0 + bias_floor_div(2 * num + den, 2 * den);
    nb = nb > UNET_BIAS_MAX ? UNET_BIAS_MAX : nb < -UNET_BIAS_MAX ? -UNET_BIAS_MAX : nb;
    return (int)nb;
}
__device__ __forceinline__ void bias_colour_node(int64_t b, const WarpLat& L, int colour, int& i, int& j, int& k) {
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const unsigned mx = (unsigned)(L.nx - cx + 1) / 2u, my = (unsigned)(L.ny - cy + 1) / 2u;
    i = cx + 2 * (int)(b % mx);
    j = cy + 2 * (int)((b / mx) % my);
    k = cz + 2 * (int)(b / ((int64_t)mx * my));
}

// ---- the log code, the levels, the residual --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BIAS_T) k_bias_logcode(const float* __restrict__ v, int64_t S, int32_t* __restrict__ q) {
    for (int64_t i = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * BIAS_T) q[i] = bias_code(v[i]);
}

__global__ void __launch_bounds__(BIAS_T) k_bias_levels(const int32_t* __restrict__ q, const void* __restrict__ labels, int lbytes, BiasGrid G,
                                                        BiasClasses cls, const int32_t* __restrict__ B, WarpLat L, u64* __restrict__ acc) {
    __shared__ i64 part[BIAS_T / 64][2 * BIAS_MAXK];
    i64 s[BIAS_MAXK] = {};
    int n[BIAS_MAXK] = {};
    const int64_t S = (int64_t)G.sw * G.sh * G.sd;
    for (int64_t i64v = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i64v < S; i64v += (int64_t)gridDim.x * BIAS_T) {
        const int qq = q[i64v];
        if (qq == BIAS_NONE) continue;
        const int t = bias_class(bias_label(labels, lbytes, i64v), cls);
        if (t < 0) continue;
        const int v = (int)i64v, x = v % G.sw, y = (v / G.sw) % G.sh, z = v / (G.sw * G.sh);
        const int d = qq - (bias_n(B, L, x, y, z) >> (3 * L.lg));
#pragma unroll
        for (int k = 0; k < BIAS_MAXK; ++k)
            if (t == k) {
                s[k] += d;
                ++n[k];
            }
    }
#pragma unroll
    for (int k = 0; k < BIAS_MAXK; ++k)
        if (k < cls.K) {   // uniform
            const i64 a = bias_wave_sum(s[k]), b = bias_wave_sum((i64)n[k]);
            if ((threadIdx.x & 63) == 0) {
                part[threadIdx.x >> 6][2 * k] = a;
                part[threadIdx.x >> 6][2 * k + 1] = b;
            }
        }
    __syncthreads();
    if ((int)threadIdx.x < 2 * cls.K) {
        i64 a = 0;
        for (int w = 0; w < BIAS_T / 64; ++w) a += part[w][threadIdx.x];
        // row t = {m, count, sum}: the sum at 3 t + 2, the count at 3 t + 1
        if (a) atomicAdd(acc + 3 * (threadIdx.x >> 1) + ((threadIdx.x & 1) ? 1 : 2), (u64)a);
    }
}

__global__ void k_bias_close(int64_t* __restrict__ lev) {
    if (threadIdx.x >= BIAS_MAXK) return;
    const int64_t n = lev[3 * threadIdx.x + 1];
    lev[3 * threadIdx.x] = n > 0 ? bias_floor_div(lev[3 * threadIdx.x + 2], n) : (int64_t)BIAS_NONE;
}

__global__ void __launch_bounds__(BIAS_T) k_bias_residual(const int32_t* __restrict__ q, const void* __restrict__ labels, int lbytes, int64_t S,
                                                          BiasClasses cls, const int64_t* __restrict__ lev, int clip, int16_t* __restrict__ r) {
    __shared__ int lm[BIAS_MAXK];
    if (threadIdx.x < BIAS_MAXK) lm[threadIdx.x] = (int)lev[3 * threadIdx.x];   // |m| < 2^20, or BIAS_NONE
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i < S; i += (int64_t)gridDim.x * BIAS_T) {
        const int qq = q[i];
        int out = BIAS_SKIP;
        if (qq != BIAS_NONE) {
            const int t = bias_class(bias_label(labels, lbytes, i), cls);
            const int m = t < 0 ? BIAS_NONE : lm[t];
            if (m != BIAS_NONE) {
                const int d = qq - m;   // |q|, |m| <= 2^19 + 2^13
                if (abs(d) <= clip) out = d;
            }
        }
        r[i] = (int16_t)out;
    }
}

// ---- a colour pass, a block per node ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) k_bias_node(const int16_t* __restrict__ r, BiasGrid G, int32_t* B, WarpLat L, int colour, i64 Lam,
                                                  u64* info, const u64* prev) {
    __shared__ int ld[27];   // the 3x3x3 neighbourhood, x fastest; a node that does not exist holds 0
    __shared__ i64 lsum[(NT / 64) * 2];
    if (prev && *prev == 0ull) return;   // uniform: the preceding sweep is complete (stream order) and changed nothing
    int i, j, k;
    bias_colour_node(blockIdx.x, L, colour, i, j, k);
    const int tid = threadIdx.x;
    if (tid < 27) {
        const int ii = i + tid % 3 - 1, jj = j + (tid / 3) % 3 - 1, kk = k + tid / 9 - 1;
        const bool ok = ii >= 0 && ii < L.nx && jj >= 0 && jj < L.ny && kk >= 0 && kk < L.nz;
        ld[tid] = ok ? B[((size_t)kk * L.ny + jj) * L.nx + ii] : 0;
    }
    __syncthreads();
    int x0, x1, y0, y1, z0, z1;
    warp_support(i, L.g, G.sw, x0, x1);
    warp_support(j, L.g, G.sh, y0, y1);
    warp_support(k, L.g, G.sd, z0, z1);
    i64 S1 = 0, S2 = 0;
    if (x0 <= x1 && y0 <= y1 && z0 <= z1) {   // uniform; a node with an empty support is still tied to its neighbours
        const int g = L.g, lg3 = 3 * L.lg, ey = y1 - y0 + 1, CM = g / 4 + 1;   // a row of <= 2 g - 1 voxels meets <= g / 4 + 1 runs
        const int items = ey * (z1 - z0 + 1) * CM;
        const int64_t S = (int64_t)G.sw * G.sh * G.sd;
        for (int it = tid; it < items; it += NT) {
            const int row = it / CM, ch = it - row * CM, y = y0 + row % ey, z = z0 + row / ey;
            const int64_t base = ((int64_t)z * G.sh + y) * G.sw;
            const int64_t e0 = ((base + x0) & ~(int64_t)7) + 8 * ch;   // r is 16-byte aligned: runs of 8 start at multiples of 8
            if (e0 > base + x1) continue;
            int w[4];
            if (e0 + 8 <= S) {
                const int4 p = *(const int4*)(r + e0);
                w[0] = p.x; w[1] = p.y; w[2] = p.z; w[3] = p.w;
            } else {   // the run leaves the volume: its tail reads as skipped
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned lo = e0 + 2 * u < S ? (uint16_t)r[e0 + 2 * u] : (uint16_t)BIAS_SKIP;
                    const unsigned hi = e0 + 2 * u + 1 < S ? (uint16_t)r[e0 + 2 * u + 1] : (uint16_t)BIAS_SKIP;
                    w[u] = (int)(lo | (hi << 16));
                }
            }
            // the row's n at the three x-nodes of the neighbourhood: n(x) = (g - fx) * P[bx] + fx * P[bx + 1]
            const int dy = y - j * g, dz = z - k * g, by = dy >= 0 ? 1 : 0, bz = dz >= 0 ? 1 : 0;
            const int fy = dy >= 0 ? dy : g + dy, fz = dz >= 0 ? dz : g + dz;
            const int w00 = (g - fy) * (g - fz), w10 = fy * (g - fz), w01 = (g - fy) * fz, w11 = fy * fz;
            const int* c = ld + (bz * 3 + by) * 3;
            const int P0 = w00 * c[0] + w10 * c[3] + w01 * c[9] + w11 * c[12];    // <= g^2 * 8192 = 2^23
            const int P1 = w00 * c[1] + w10 * c[4] + w01 * c[10] + w11 * c[13];
            const int P2 = w00 * c[2] + w10 * c[5] + w01 * c[11] + w11 * c[14];
            const int Wyz = (g - abs(dy)) * (g - abs(dz));
            i64 t1 = 0;   // the run's sum of wx * e: 8 * 2^5 * 2^29
            int t2 = 0;   // and of wx * wx
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = (int)(e0 - base) + u;
                const int rr = (int)(int16_t)((u & 1) ? (unsigned)w[u >> 1] >> 16 : (unsigned)w[u >> 1] & 0xFFFFu);
                if (x < x0 || x > x1 || rr == BIAS_SKIP) continue;
                const int dx = x - i * g, fx = dx >= 0 ? dx : g + dx;
                const int n = (g - fx) * (dx >= 0 ? P1 : P0) + fx * (dx >= 0 ? P2 : P1);   // <= 2^28
                const int wx = g - abs(dx);
                t1 += (i64)wx * (rr * (1 << lg3) - n);
                t2 += wx * wx;
            }
            S1 += t1 * Wyz;
            S2 += (i64)(Wyz * Wyz) * t2;
        }
    }
    S1 = bias_wave_sum(S1);
    S2 = bias_wave_sum(S2);
    if ((tid & 63) == 0) {
        lsum[(tid >> 6) * 2] = S1;
        lsum[(tid >> 6) * 2 + 1] = S2;
    }
    __syncthreads();
    if (tid == 0) {
        i64 a = 0, b = 0;
        for (int w = 0; w < NT / 64; ++w) {
            a += lsum[2 * w];
            b += lsum[2 * w + 1];
        }
        const int b0 = ld[13];
        i64 dsum = 0;
        int nbrs = 0;
        if (i > 0) { dsum += ld[12] - b0; ++nbrs; }
        if (i + 1 < L.nx) { dsum += ld[14] - b0; ++nbrs; }
        if (j > 0) { dsum += ld[10] - b0; ++nbrs; }
        if (j + 1 < L.ny) { dsum += ld[16] - b0; ++nbrs; }
        if (k > 0) { dsum += ld[4] - b0; ++nbrs; }
        if (k + 1 < L.nz) { dsum += ld[22] - b0; ++nbrs; }
        bool visited;
        const int nb = bias_update(b0, a, b, dsum, nbrs, Lam, visited);
        if (nb != b0) {
            B[((size_t)k * L.ny + j) * L.nx + i] = nb;
            atomicAdd(info, 1ull);
        }
        if (visited) atomicAdd(info + 1, 1ull);
    }
}

// ---- a colour pass, a thread per voxel -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BIAS_T) k_bias_vox(const int16_t* __restrict__ r, BiasGrid G, const int32_t* __restrict__ B, WarpLat L,
                                                     int colour, u64* __restrict__ cnt, const u64* prev) {
    if (prev && *prev == 0ull) return;
    const int S = G.sw * G.sh * G.sd, g = L.g;
    for (int64_t i64v = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i64v < S; i64v += (int64_t)gridDim.x * BIAS_T) {
        const int rr = r[i64v];
        if (rr == BIAS_SKIP) continue;
        const int v = (int)i64v, x = v % G.sw, y = (v / G.sw) % G.sh, z = v / (G.sw * G.sh);
        const int i = warp_owner(x, L.lg, g, colour & 1), j = warp_owner(y, L.lg, g, (colour >> 1) & 1), k = warp_owner(z, L.lg, g, colour >> 2);
        if (i < 0 || j < 0 || k < 0) continue;
        const int W = (g - abs(x - i * g)) * (g - abs(y - j * g)) * (g - abs(z - k * g));
        const int e = rr * (1 << (3 * L.lg)) - bias_n(B, L, x, y, z);
        u64* cn = cnt + (((size_t)k * L.ny + j) * L.nx + i) * 2;
        atomicAdd(cn, (u64)((i64)W * e));   // two's complement: the wrapped sum is the signed sum
        atomicAdd(cn + 1, (u64)((i64)W * W));
    }
}

__global__ void __launch_bounds__(BIAS_T) k_bias_update(int32_t* B, WarpLat L, int colour, i64 Lam, u64* __restrict__ cnt, u64* info,
                                                        const u64* prev) {
    if (prev && *prev == 0ull) return;
    const int cx = colour & 1, cy = (colour >> 1) & 1, cz = colour >> 2;
    const int64_t nodes = (int64_t)((L.nx - cx + 1) / 2) * ((L.ny - cy + 1) / 2) * ((L.nz - cz + 1) / 2);
    for (int64_t b = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; b < nodes; b += (int64_t)gridDim.x * BIAS_T) {
        int i, j, k;
        bias_colour_node(b, L, colour, i, j, k);
        const size_t node = ((size_t)k * L.ny + j) * L.nx + i;
        const i64 S1 = (i64)cnt[2 * node], S2 = (i64)cnt[2 * node + 1];
        cnt[2 * node] = 0ull;
        cnt[2 * node + 1] = 0ull;
        const int b0 = B[node];   // the neighbours are of other colours: not written in this pass
        i64 dsum = 0;
        int nbrs = 0;
        if (i > 0) { dsum += B[node - 1] - b0; ++nbrs; }
        if (i + 1 < L.nx) { dsum += B[node + 1] - b0; ++nbrs; }
        if (j > 0) { dsum += B[node - L.nx] - b0; ++nbrs; }
        if (j + 1 < L.ny) { dsum += B[node + L.nx] - b0; ++nbrs; }
        if (k > 0) { dsum += B[node - (size_t)L.nx * L.ny] - b0; ++nbrs; }
        if (k + 1 < L.nz) { dsum += B[node + (size_t)L.nx * L.ny] - b0; ++nbrs; }
        bool visited;
        const int nb = bias_update(b0, S1, S2, dsum, nbrs, Lam, visited);
        if (nb != b0) {
            B[node] = nb;
            atomicAdd(info, 1ull);
        }
        if (visited) atomicAdd(info + 1, 1ull);
    }
}

// ---- the cost, the report, refine, apply -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BIAS_T) k_bias_cost(const int16_t* __restrict__ r, BiasGrid G, const int32_t* __restrict__ B, WarpLat L,
                                                      u64* __restrict__ cost) {
    __shared__ i64 part[BIAS_T / 64][2];
    i64 s = 0, n = 0;
    const int S = G.sw * G.sh * G.sd;
    for (int64_t i64v = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i64v < S; i64v += (int64_t)gridDim.x * BIAS_T) {
        const int rr = r[i64v];
        if (rr == BIAS_SKIP) continue;
        const int v = (int)i64v, x = v % G.sw, y = (v / G.sw) % G.sh, z = v / (G.sw * G.sh);
        const int d = rr - (bias_n(B, L, x, y, z) >> (3 * L.lg));   // |d| <= 2^14
        s += d * d;
        ++n;
    }
    s = bias_wave_sum(s);
    n = bias_wave_sum(n);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = s;
        part[threadIdx.x >> 6][1] = n;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        i64 a = 0;
        for (int w = 0; w < BIAS_T / 64; ++w) a += part[w][threadIdx.x];
        if (a) atomicAdd(cost + threadIdx.x, (u64)a);
    }
}

// slots: the `sweeps` {changed, visited} pairs of this round; sweep s ran when s == 0 or sweep s - 1 changed a node
__global__ void k_bias_row(const u64* __restrict__ slots, int sweeps, int g, int round, int64_t* __restrict__ row) {
    if (threadIdx.x) return;
    int ran = 1;
    while (ran < sweeps && slots[2 * (ran - 1)]) ++ran;
    row[0] = g;
    row[1] = round;
    row[2] = ran;
    row[3] = (int64_t)slots[2 * (ran - 1)];
    row[4] = row[5] = 0;   // the cost pass adds into them
}

__global__ void __launch_bounds__(BIAS_T) k_bias_refine(const int32_t* __restrict__ coarse, WarpLat C, WarpLat F, int32_t* __restrict__ fine) {
    const int64_t nodes = (int64_t)F.nx * F.ny * F.nz;
    for (int64_t e = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; e < nodes; e += (int64_t)gridDim.x * BIAS_T) {
        const int i = (int)(e % F.nx), j = (int)((e / F.nx) % F.ny), k = (int)(e / ((int64_t)F.nx * F.ny));
        const int ia[2] = {i >> 1, min((i >> 1) + (i & 1), C.nx - 1)}, ja[2] = {j >> 1, min((j >> 1) + (j & 1), C.ny - 1)},
                  ka[2] = {k >> 1, min((k >> 1) + (k & 1), C.nz - 1)};
        int s = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) s += coarse[((size_t)ka[c >> 2] * C.ny + ja[(c >> 1) & 1]) * C.nx + ia[c & 1]];
        fine[e] = (s + 4) >> 3;
    }
}

__global__ void __launch_bounds__(BIAS_T) k_bias_apply(const float* __restrict__ v, BiasGrid G, const int32_t* __restrict__ B, WarpLat L,
                                                       float* __restrict__ out, float* __restrict__ gain) {
#pragma clang fp contract(off)
    const int S = G.sw * G.sh * G.sd, sh3 = 3 * L.lg;
    for (int64_t i64v = (int64_t)blockIdx.x * BIAS_T + threadIdx.x; i64v < S; i64v += (int64_t)gridDim.x * BIAS_T) {
        const int i = (int)i64v, x = i % G.sw, y = (i / G.sw) % G.sh, z = i / (G.sw * G.sh);
        const int c = (-bias_n(B, L, x, y, z) + (1 << (sh3 - 1))) >> sh3, k = c >> 12;
        const float t = bias_table[c & 4095];
        const float two_k = __uint_as_float((unsigned)(127 + k) << 23);   // |k| <= 2; ldexpf(p, k) is p * 2^k, one IEEE rounding
        if (out) {
            float o = v[i];
            if (c) {
                const float p = o * t;
                o = p * two_k;
                if (o != o) o = __uint_as_float(0x7FC00000u);
            }
            out[i] = o;
        }
        if (gain) gain[i] = t * two_k;
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
void bias_memset(void* p, int value, size_t bytes, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(p, value, bytes, s); e != hipSuccess)
        throw std::runtime_error(std::string("unet_bias: hipMemsetAsync: ") + hipGetErrorString(e));
}
int bias_blocks(int64_t items, int cap) {
    const int64_t nb = (items + BIAS_T - 1) / BIAS_T;
    return (int)(nb > cap ? cap : nb < 1 ? 1 : nb);
}
BiasClasses bias_classes(const int* classes, int K) {
    BiasClasses c = {};
    c.K = K;
    for (int k = 0; k < K; ++k) c.v[k] = classes[k];
    return c;
}

struct BiasScratch {
    u64* slots;       // BIAS_SLOTS x {changed, visited}
    int64_t* lev;     // {BIAS_MAXK, 3}
    int16_t* r;       // the residual
    u64* cnt;         // 2 per node of the finest lattice
    int32_t* field[UNET_BIAS_MAX_LEVELS];   // the levels but the last
    size_t bytes;     // from the aligned base
};
BiasScratch bias_scratch(void* scratch, int sw, int sh, int sd, const int* levels, int n_levels) {
    char* b = (char*)warp_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    BiasScratch s = {};
    size_t o = 0;
    s.slots = (u64*)(b + o);   o += warp_align((size_t)BIAS_SLOTS * 2 * sizeof(u64));
    s.lev = (int64_t*)(b + o); o += warp_align((size_t)BIAS_MAXK * 3 * sizeof(int64_t));
    s.r = (int16_t*)(b + o);   o += warp_align((size_t)sw * sh * sd * sizeof(int16_t));
    s.cnt = (u64*)(b + o);     o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[3 * (n_levels - 1)])) * 2 * sizeof(u64));
    for (int l = 0; l + 1 < n_levels; ++l) {
        s.field[l] = (int32_t*)(b + o);
        o += warp_align(warp_nodes(warp_lattice(sw, sh, sd, levels[3 * l])) * sizeof(int32_t));
    }
    s.bytes = o;
    return s;
}

void bias_levels_into(const int32_t* q, const void* labels, int lbytes, const BiasGrid& G, const BiasClasses& cls, const int32_t* B,
                      const WarpLat& L, int64_t* lev, hipStream_t s) {
    bias_memset(lev, 0, (size_t)BIAS_MAXK * 3 * sizeof(int64_t), s);
    k_bias_levels<<<bias_blocks((int64_t)G.sw * G.sh * G.sd, BIAS_REDB), BIAS_T, 0, s>>>(q, labels, lbytes, G, cls, B, L, (u64*)lev);
    k_bias_close<<<1, 64, 0, s>>>(lev);
}
void bias_residual_into(const int32_t* q, const void* labels, int lbytes, const BiasGrid& G, const BiasClasses& cls, const int64_t* lev, int clip,
                        int16_t* r, hipStream_t s) {
    const int64_t S = (int64_t)G.sw * G.sh * G.sd;
    k_bias_residual<<<bias_blocks(S, BIAS_MAXB), BIAS_T, 0, s>>>(q, labels, lbytes, S, cls, lev, clip, r);
}
// one sweep: the 8 colour passes.  cnt: zero on entry under IMPL_VOXEL, and left zero
void bias_sweep_into(const int16_t* r, const BiasGrid& G, int32_t* B, const WarpLat& L, int lam, u64* info, const u64* prev, int impl, u64* cnt,
                     hipStream_t s) {
    const i64 Lam = (i64)lam << (6 * L.lg);
    for (int c = 0; c < 8; ++c) {
        const int64_t nodes = (int64_t)((L.nx - (c & 1) + 1) / 2) * ((L.ny - ((c >> 1) & 1) + 1) / 2) * ((L.nz - (c >> 2) + 1) / 2);
        if (impl == UNET_BIAS_IMPL_VOXEL) {
            k_bias_vox<<<bias_blocks((int64_t)G.sw * G.sh * G.sd, BIAS_MAXB), BIAS_T, 0, s>>>(r, G, B, L, c, cnt, prev);
            k_bias_update<<<bias_blocks(nodes, BIAS_MAXB), BIAS_T, 0, s>>>(B, L, c, Lam, cnt, info, prev);
            continue;
        }
        // DEFAULT: NODE
        if (L.g == 4) k_bias_node<64><<<(unsigned)nodes, 64, 0, s>>>(r, G, B, L, c, Lam, info, prev);
        else if (L.g == 8) k_bias_node<256><<<(unsigned)nodes, 256, 0, s>>>(r, G, B, L, c, Lam, info, prev);
        else k_bias_node<1024><<<(unsigned)nodes, 1024, 0, s>>>(r, G, B, L, c, Lam, info, prev);
    }
}
void bias_cost_into(const int16_t* r, const BiasGrid& G, const int32_t* B, const WarpLat& L, int64_t* cost, hipStream_t s) {
    k_bias_cost<<<bias_blocks((int64_t)G.sw * G.sh * G.sd, BIAS_REDB), BIAS_T, 0, s>>>(r, G, B, L, (u64*)cost);
}
void bias_refine_into(const int32_t* coarse, const BiasGrid& G, int g, int32_t* fine, hipStream_t s) {
    const WarpLat C = warp_lattice(G.sw, G.sh, G.sd, g), F = warp_lattice(G.sw, G.sh, G.sd, g / 2);
    k_bias_refine<<<bias_blocks((int64_t)warp_nodes(F), BIAS_MAXB), BIAS_T, 0, s>>>(coarse, C, F, fine);
}

}  // namespace

size_t bias_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels) {
    return 256 + bias_scratch(nullptr, sw, sh, sd, levels, n_levels).bytes;
}
size_t bias_sweep_scratch_bytes(int sw, int sh, int sd, int g) {   // the aligned base, then the counters alone
    return 256 + warp_align(warp_nodes(warp_lattice(sw, sh, sd, g)) * 2 * sizeof(u64));
}

void launch_bias_logcode(const float* v, int64_t voxels, int32_t* q, hipStream_t s) {
    k_bias_logcode<<<bias_blocks(voxels, BIAS_MAXB), BIAS_T, 0, s>>>(v, voxels, q);
}

void launch_bias_levels(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, const int32_t* B,
                        int g, int64_t* levels_out, hipStream_t s) {
    bias_levels_into(q, labels, lbytes, {sw, sh, sd}, bias_classes(classes, K), B, warp_lattice(sw, sh, sd, g), levels_out, s);
}

void launch_bias_residual(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K,
                          const int64_t* levels_in, int clip, int16_t* r, hipStream_t s) {
    bias_residual_into(q, labels, lbytes, {sw, sh, sd}, bias_classes(classes, K), levels_in, clip, r, s);
}

void launch_bias_sweep(const int16_t* r, int sw, int sh, int sd, int32_t* B, int g, int lam, int64_t* info, int impl, void* scratch,
                       hipStream_t s) {
    u64* cnt = (u64*)warp_align((size_t)(uintptr_t)scratch);   // bias_sweep_scratch_bytes: nothing but the counters
    const WarpLat L = warp_lattice(sw, sh, sd, g);
    bias_memset(info, 0, 2 * sizeof(int64_t), s);
    if (impl == UNET_BIAS_IMPL_VOXEL) bias_memset(cnt, 0, warp_nodes(L) * 2 * sizeof(u64), s);
    bias_sweep_into(r, {sw, sh, sd}, B, L, lam, (u64*)info, nullptr, impl, cnt, s);
}

void launch_bias_refine(const int32_t* coarse, int sw, int sh, int sd, int g, int32_t* fine, hipStream_t s) {
    bias_refine_into(coarse, {sw, sh, sd}, g, fine, s);
}

void launch_bias_cost(const int16_t* r, int sw, int sh, int sd, const int32_t* B, int g, int64_t* cost, hipStream_t s) {
    bias_memset(cost, 0, 2 * sizeof(int64_t), s);
    bias_cost_into(r, {sw, sh, sd}, B, warp_lattice(sw, sh, sd, g), cost, s);
}

void launch_bias_fit(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, int clip,
                     const int* levels, int n_levels, int outer, int32_t* B_out, int64_t* report, int impl, void* scratch, hipStream_t s) {
    const BiasScratch sc = bias_scratch(scratch, sw, sh, sd, levels, n_levels);
    const BiasGrid G = {sw, sh, sd};
    const BiasClasses cls = bias_classes(classes, K);
    bias_memset(report, 0xFF, (size_t)UNET_BIAS_MAX_ROWS * 6 * sizeof(int64_t), s);   // -1 in every row
    bias_memset(sc.slots, 0, (size_t)BIAS_SLOTS * 2 * sizeof(u64), s);
    if (impl == UNET_BIAS_IMPL_VOXEL)
        bias_memset(sc.cnt, 0, warp_nodes(warp_lattice(sw, sh, sd, levels[3 * (n_levels - 1)])) * 2 * sizeof(u64), s);
    int row = 0, slot = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* lv = levels + 3 * l;
        const WarpLat L = warp_lattice(sw, sh, sd, lv[0]);
        int32_t* B = l + 1 < n_levels ? sc.field[l] : B_out;
        if (l == 0) bias_memset(B, 0, warp_nodes(L) * sizeof(int32_t), s);
        for (int o = 0; o < outer; ++o, ++row) {
            bias_levels_into(q, labels, lbytes, G, cls, B, L, sc.lev, s);
            bias_residual_into(q, labels, lbytes, G, cls, sc.lev, clip, sc.r, s);
            const int first = slot;
            for (int k = 0; k < lv[1]; ++k, ++slot)
                bias_sweep_into(sc.r, G, B, L, lv[2], sc.slots + 2 * slot, k ? sc.slots + 2 * (slot - 1) : nullptr, impl, sc.cnt, s);
            k_bias_row<<<1, 64, 0, s>>>(sc.slots + 2 * first, lv[1], lv[0], o, report + 6 * row);
            bias_cost_into(sc.r, G, B, L, report + 6 * row + 4, s);
        }
        if (l + 1 < n_levels) bias_refine_into(B, G, lv[0], l + 2 < n_levels ? sc.field[l + 1] : B_out, s);
    }
}

void launch_bias_apply(const float* v, int sw, int sh, int sd, const int32_t* B, int g, float* out, float* gain, hipStream_t s) {
    k_bias_apply<<<bias_blocks((int64_t)sw * sh * sd, BIAS_MAXB), BIAS_T, 0, s>>>(v, {sw, sh, sd}, B, warp_lattice(sw, sh, sd, g), out, gain);
}

}  // namespace unet
