// The geometry of a fitted lattice warp (include/unet_deform.h): the Jacobian determinant of map + field on the subject grid, and a
// subject-grid volume pulled onto the template grid through the inverse of map + field, a fixed-point iteration per template voxel.
// The lattice and the map are lattice_field.h's (shared with kernels_warp.hip and kernels_cowarp.hip); the trilinear sampler is
// device_util.h's (what k_cowarp_resample samples with).
//
//   k_deform_init       one thread: info's start values (the voxel count, the keys of the extremes; zeros for a pull)
//   k_deform_jacobian   a thread per subject voxel of a 16 x 4 x 4 brick, a block walking over several bricks (below): the cell's 8 corners read from global memory (a
//                       wave is a 16 x 4 slab of one z: at g >= 4 it reads at most 5 x 2 x 2 nodes, every address shared by 16 lanes
//                       or more, so the loads are broadcasts out of L1; staging them would put a barrier in front of a kernel
//                       that is bound by its 4-byte store), nine exact integer derivatives, the determinant, and the block's folded
//                       count and extreme keys reduced by lane shuffles, then LDS, then one atomic per block per quantity
//   k_deform_pull<K, TILE>   a thread per template voxel of the same bricks: s0, `iters` rounds of e(s) (8 corners x 3 components
//                       per round), one more e(s) for the residual, the sample, pos, and the block's two counts reduced the same
//                       way.  TILE: the brick's lattice window staged in LDS first; a cell outside the window, or a window that
//                       does not fit, reads global memory.  The two paths run the same arithmetic on the same integers
// Bricks: the grid is capped at DF_MAXB blocks (what the device holds at once) and a block walks over its share of the bricks with
// its counts and extremes in registers, so that a call ends in at most DF_MAXB atomics per quantity: with a block per brick the
// 65536 blocks of a 256^3 jacobian spent 1.5 ms queueing on the three words of info.  As in device_util.h's
// brick_walk each XCD (blocks are dealt round-robin to the 8) works through one contiguous range of bricks.
// Contraction is off for the whole file: every product and every sum is rounded, as the restatement's are.
#include <stdexcept>
#include <string>

#include "../../include/unet_deform.h"
#include "device_util.h"
#include "kernels.h"
#include "lattice_field.h"

#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int DF_T = 256;                           // a 16 x 4 x 4 brick
constexpr int DF_WAVES = DF_T / 64;
constexpr int DF_MAXB = 1280;                       // blocks of a launch: 256 CUs x 5, what every kernel here keeps resident
constexpr int DF_MARGIN = 2;                        // nodes added around the window the brick's s0 spans
constexpr int DF_WINDOW = UNET_DEFORM_MAX_WINDOW;   // nodes a block stages at most: 1536 x 12 B = 18 KiB, 8 blocks a CU
typedef unsigned long long u64;
static_assert(WARP_MAX_DISP == UNET_DEFORM_MAX_DISP, "lattice_field.h's range is this header's");
static_assert(DF_T == BRICK_X * BRICK_Y * BRICK_Z, "a thread per voxel of a brick");

__device__ __forceinline__ unsigned df_key(float v) {   // kernels_stats.hip's st_key
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float df_store(float v) {   // a NaN is stored as the one quiet NaN 0x7FC00000, whatever its sign and payload
    return v == v ? v : __uint_as_float(0x7FC00000u);
}

__global__ void k_deform_init(u64* info, u64 a, u64 b, u64 c, u64 d, int n) {
    const u64 v[4] = {a, b, c, d};
    if (threadIdx.x == 0 && blockIdx.x == 0)
        for (int e = 0; e < n; ++e) info[e] = v[e];
}

// sum / min / max of one value per thread over the block; the result is valid in thread 0
template <typename Op> __device__ __forceinline__ unsigned df_reduce(unsigned v, unsigned* lds, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (unsigned)__shfl_xor((int)v, o));
    __syncthreads();   // lds may still be read by the reduction before this one
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < DF_WAVES; ++w) v = op(v, lds[w]);
    return v;
}

// body(x0, y0, z0) for every brick of this block, a uniform loop (barriers inside the body are safe)
template <typename Body> __device__ __forceinline__ void df_bricks(int W, int H, int D, Body body) {
    const unsigned gx = (W + BRICK_X - 1) / BRICK_X, gy = (H + BRICK_Y - 1) / BRICK_Y, gz = (D + BRICK_Z - 1) / BRICK_Z;
    const unsigned nb = gx * gy * gz, per = (nb + 7) / 8, first = (blockIdx.x & 7) * per, last = min(first + per, nb);
    for (unsigned b = first + (blockIdx.x >> 3); b < last; b += gridDim.x >> 3) {
        const unsigned bx = b % gx, r = b / gx;
        body((int)(bx * BRICK_X), (int)((r % gy) * BRICK_Y), (int)((r / gy) * BRICK_Z));
    }
}
unsigned df_grid(int w, int h, int d) {   // a multiple of 8
    const int64_t nb = space_bricks(w, h, d);
    return (unsigned)(nb < DF_MAXB ? nb : DF_MAXB);
}

// ---- the Jacobian -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DF_T) k_deform_jacobian(int sw, int sh, int sd, WarpMap map, const int32_t* __restrict__ D, WarpLat L,
                                                          float* __restrict__ det, u64* info) {
    __shared__ unsigned lds[DF_WAVES];
    unsigned folded = 0u, kmin = 0xFFFFFFFFu, kmax = 0u;
    df_bricks(sw, sh, sd, [&](int x0, int y0, int z0) {
        const int x = x0 + (threadIdx.x & (BRICK_X - 1)), y = y0 + ((threadIdx.x / BRICK_X) & (BRICK_Y - 1)), z = z0 + threadIdx.x / (BRICK_X * BRICK_Y);
        if (x >= sw || y >= sh || z >= sd) return;
        const int g = L.g, m = g - 1, cx = x >> L.lg, cy = y >> L.lg, cz = z >> L.lg, fx = x & m, fy = y & m, fz = z & m;
        int G[3][3] = {};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int wx = (c & 1) ? fx : g - fx, wy = (c & 2) ? fy : g - fy, wz = (c & 4) ? fz : g - fz;
            const int ax = ((c & 1) ? 1 : -1) * wy * wz, ay = ((c & 2) ? 1 : -1) * wx * wz, az = ((c & 4) ? 1 : -1) * wx * wy;
            const int32_t* d = D + (((size_t)(cz + (c >> 2)) * L.ny + (cy + ((c >> 1) & 1))) * L.nx + (cx + (c & 1))) * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int v = d[r];
                G[r][0] += ax * v;
                G[r][1] += ay * v;
                G[r][2] += az * v;
            }
        }
        float J[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = (float)G[r][c] * L.scale;   // a power of two: exact
                J[3 * r + c] = map.v[3 * r + c] + d;
            }
        const float t0 = J[4] * J[8] - J[5] * J[7], t1 = J[3] * J[8] - J[5] * J[6], t2 = J[3] * J[7] - J[4] * J[6];
        const float v = (J[0] * t0 - J[1] * t1) + J[2] * t2;
        if (det) det[((int64_t)z * sh + y) * sw + x] = df_store(v);
        folded += !(v > 0.f) ? 1u : 0u;
        if (v == v) {
            kmin = min(kmin, df_key(v));
            kmax = max(kmax, df_key(v));
        }
    });
    folded = df_reduce(folded, lds, [](unsigned a, unsigned b) { return a + b; });
    kmin = df_reduce(kmin, lds, [](unsigned a, unsigned b) { return min(a, b); });
    kmax = df_reduce(kmax, lds, [](unsigned a, unsigned b) { return max(a, b); });
    if (threadIdx.x == 0) {
        if (folded) atomicAdd(info + 1, (u64)folded);
        if (kmin <= kmax) {   // some det entered
            atomicMin(info + 2, (u64)kmin);
            atomicMax(info + 3, (u64)kmax);
        }
    }
}

// ---- the continuous field -----------------------------------------------------------------------------------------------------------
struct DfCell {
    int c;
    float f;
};
__device__ __forceinline__ DfCell df_cell(float s, float inv_g, int n) {
    float t = s * inv_g;
    t = t > 0.f ? t : 0.f;
    const float top = (float)(n - 1);
    t = t < top ? t : top;
    DfCell r;
    r.c = min((int)floorf(t), n - 2);
    r.f = t - (float)r.c;
    return r;
}
__device__ __forceinline__ float df_lerp(float f, float a, float b) { return a + f * (b - a); }

// e(s): node(ix, iy, iz) -> the three components of a node of the lattice
template <typename Node> __device__ __forceinline__ void df_field(const DfCell& X, const DfCell& Y, const DfCell& Z, Node node, float* e) {
    int v[8][3];
#pragma unroll
    for (int c = 0; c < 8; ++c) node(X.c + (c & 1), Y.c + ((c >> 1) & 1), Z.c + (c >> 2), v[c]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float c00 = df_lerp(X.f, (float)v[0][r], (float)v[1][r]), c10 = df_lerp(X.f, (float)v[2][r], (float)v[3][r]);
        const float c01 = df_lerp(X.f, (float)v[4][r], (float)v[5][r]), c11 = df_lerp(X.f, (float)v[6][r], (float)v[7][r]);
        e[r] = df_lerp(Z.f, df_lerp(Y.f, c00, c10), df_lerp(Y.f, c01, c11)) * 0.00390625f;
    }
}

struct DfWindow {   // nodes [x0, x0 + nx) x [y0, y0 + ny) x [z0, z0 + nz) staged in LDS, x fastest then component; nx = 0: none
    int x0, y0, z0, nx, ny, nz;
};
// the window along one axis from the extremes of the brick's s0 (NaN extremes give the whole axis: fmaxf / fminf drop a NaN)
__device__ __forceinline__ void df_span(float lo, float hi, float inv_g, int n, int& first, int& count) {
    const float a = fminf(fmaxf(lo * inv_g, 0.f), (float)(n - 1)), b = fminf(fmaxf(hi * inv_g, 0.f), (float)(n - 1));
    first = max((int)a - DF_MARGIN, 0);
    count = min((int)b + 1 + DF_MARGIN, n - 1) - first + 1;
}

template <int KIND> struct DfType;
template <> struct DfType<UNET_DEFORM_KIND_F32> { typedef float T; };
template <> struct DfType<UNET_DEFORM_KIND_U8> { typedef uint8_t T; };
template <> struct DfType<UNET_DEFORM_KIND_U16> { typedef uint16_t T; };

struct DfArgs {
    const void* vol;
    int sw, sh, sd, tw, th, td, iters;
    WarpMap map, inv;
    const int32_t* D;   // or null
    WarpLat L;
    void* out;
    float* pos;         // or null
    u64* info;
};

template <int KIND, bool TILE> __global__ void __launch_bounds__(DF_T) k_deform_pull(const DfArgs A) {
    typedef typename DfType<KIND>::T T;
    __shared__ unsigned lds[DF_WAVES];
    __shared__ int ld[TILE ? DF_WINDOW * 3 : 1];
    const int32_t* __restrict__ D = A.D;
    const WarpLat L = A.L;
    const float* inv = A.inv.v;
    const float inv_g = 1.f / (float)L.g;   // a power of two
    unsigned inside = 0u, open = 0u;

    df_bricks(A.tw, A.th, A.td, [&](int x0, int y0, int z0) {
        DfWindow W = {0, 0, 0, 0, 0, 0};
        if (TILE && D) {   // uniform: the window of this brick
            const int x1 = min(x0 + BRICK_X, A.tw) - 1, y1 = min(y0 + BRICK_Y, A.th) - 1, z1 = min(z0 + BRICK_Z, A.td) - 1;
            float lo[3], hi[3];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float s[3];
                warp_affine(inv, (c & 1) ? x1 : x0, (c & 2) ? y1 : y0, (c & 4) ? z1 : z0, s[0], s[1], s[2]);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    lo[r] = c ? fminf(lo[r], s[r]) : s[r];
                    hi[r] = c ? fmaxf(hi[r], s[r]) : s[r];
                }
            }
            df_span(lo[0], hi[0], inv_g, L.nx, W.x0, W.nx);
            df_span(lo[1], hi[1], inv_g, L.ny, W.y0, W.ny);
            df_span(lo[2], hi[2], inv_g, L.nz, W.z0, W.nz);
            if ((int64_t)W.nx * W.ny * W.nz > DF_WINDOW) W.nx = 0;   // does not fit: the whole block reads global memory
            const int row = W.nx * 3, total = row * W.ny * W.nz;     // <= DF_WINDOW * 3
            __syncthreads();                                         // the brick before this one is done with ld
            for (int e = threadIdx.x; e < total; e += DF_T) {
                const int i = e % row, r2 = e / row, j = r2 % W.ny, k = r2 / W.ny;
                ld[e] = D[(((size_t)(W.z0 + k) * L.ny + (W.y0 + j)) * L.nx + W.x0) * 3 + i];
            }
            __syncthreads();
        }
        const int x = x0 + (threadIdx.x & (BRICK_X - 1)), y = y0 + ((threadIdx.x / BRICK_X) & (BRICK_Y - 1)), z = z0 + threadIdx.x / (BRICK_X * BRICK_Y);
        if (x >= A.tw || y >= A.th || z >= A.td) return;   // after the barriers

        auto node = [&](int ix, int iy, int iz, int* v) {
            if (TILE) {
                const int kx = ix - W.x0, ky = iy - W.y0, kz = iz - W.z0;
                if (kx >= 0 && kx < W.nx && ky >= 0 && ky < W.ny && kz >= 0 && kz < W.nz) {
                    const int* p = ld + ((kz * W.ny + ky) * W.nx + kx) * 3;
                    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
                    return;
                }
            }
            const int32_t* p = D + (((size_t)iz * L.ny + iy) * L.nx + ix) * 3;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        };
        auto field = [&](const float* s, float* e) {
            df_field(df_cell(s[0], inv_g, L.nx), df_cell(s[1], inv_g, L.ny), df_cell(s[2], inv_g, L.nz), node, e);
        };

        float s0[3], s[3], e[3] = {0.f, 0.f, 0.f};
        warp_affine(inv, x, y, z, s0[0], s0[1], s0[2]);
        s[0] = s0[0]; s[1] = s0[1]; s[2] = s0[2];
        if (D) {
            for (int it = 0; it < A.iters; ++it) {
                field(s, e);
#pragma unroll
                for (int r = 0; r < 3; ++r) s[r] = s0[r] - ((inv[3 * r] * e[0] + inv[3 * r + 1] * e[1]) + inv[3 * r + 2] * e[2]);
            }
            field(s, e);
        }
        const int64_t o = ((int64_t)z * A.th + y) * A.tw + x, n = (int64_t)A.tw * A.th * A.td;
        if (A.pos) {
            A.pos[o] = df_store(s[0]);
            A.pos[n + o] = df_store(s[1]);
            A.pos[2 * n + o] = df_store(s[2]);
        }
        const float q0 = s[0] + 0.5f, q1 = s[1] + 0.5f, q2 = s[2] + 0.5f;
        const bool in = q0 >= 0.f && q1 >= 0.f && q2 >= 0.f && q0 < (float)A.sw && q1 < (float)A.sh && q2 < (float)A.sd;
        const T* vol = (const T*)A.vol;
        T val = (T)0;
        if (KIND == UNET_DEFORM_KIND_F32) {
            const Tri t = locate(s[0], s[1], s[2], A.sw, A.sh, A.sd);
            if (t.ok) val = (T)trilinear(t, (const float*)A.vol);
        } else if (in) {
            val = vol[((int64_t)(int)floorf(q2) * A.sh + (int)floorf(q1)) * A.sw + (int)floorf(q0)];
        }
        ((T*)A.out)[o] = val;
        if (in) {
            const float* m = A.map.v;
            const float u[3] = {(float)x, (float)y, (float)z};
            bool ok = true;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float p = ((m[3 * r] * s[0] + m[3 * r + 1] * s[1]) + m[3 * r + 2] * s[2]) + m[9 + r];
                ok = ok && fabsf((p + e[r]) - u[r]) <= 0.0625f;
            }
            inside += 1u;
            open += ok ? 0u : 1u;
        }
    });
    inside = df_reduce(inside, lds, [](unsigned a, unsigned b) { return a + b; });
    open = df_reduce(open, lds, [](unsigned a, unsigned b) { return a + b; });
    if (threadIdx.x == 0) {
        if (inside) atomicAdd(A.info, (u64)inside);
        if (open) atomicAdd(A.info + 1, (u64)open);
    }
}

template <int KIND> void df_pull(const DfArgs& A, bool tile, unsigned blocks, hipStream_t s) {
    if (tile) k_deform_pull<KIND, true><<<blocks, DF_T, 0, s>>>(A);
    else k_deform_pull<KIND, false><<<blocks, DF_T, 0, s>>>(A);
}

}  // namespace

void launch_deform_jacobian(int sw, int sh, int sd, const float* map, const int32_t* D, int g, float* det, int64_t* info, hipStream_t s) {
    k_deform_init<<<1, 64, 0, s>>>((u64*)info, (u64)((int64_t)sw * sh * sd), 0ull, 0xFFFFFFFFull, 0ull, 4);
    k_deform_jacobian<<<df_grid(sw, sh, sd), DF_T, 0, s>>>(sw, sh, sd, warp_map(map), D, warp_lattice(sw, sh, sd, g), det, (u64*)info);
}

void launch_deform_pull(const void* volume, int kind, int sw, int sh, int sd, int tw, int th, int td, const float* map, const float* inv,
                        const int32_t* D, int g, int iters, void* out, float* pos, int64_t* info, int impl, hipStream_t s) {
    DfArgs A;
    A.vol = volume;
    A.sw = sw; A.sh = sh; A.sd = sd; A.tw = tw; A.th = th; A.td = td;
    A.iters = iters;
    A.map = warp_map(map);
    A.inv = warp_map(inv);
    A.D = D;
    A.L = warp_lattice(sw, sh, sd, g);
    A.out = out;
    A.pos = pos;
    A.info = (u64*)info;
    k_deform_init<<<1, 64, 0, s>>>((u64*)info, 0ull, 0ull, 0ull, 0ull, 2);
    // DEFAULT: GLOBAL
    const bool tile = impl == UNET_DEFORM_IMPL_TILE;
    const unsigned blocks = df_grid(tw, th, td);
    if (kind == UNET_DEFORM_KIND_F32) df_pull<UNET_DEFORM_KIND_F32>(A, tile, blocks, s);
    else if (kind == UNET_DEFORM_KIND_U8) df_pull<UNET_DEFORM_KIND_U8>(A, tile, blocks, s);
    else df_pull<UNET_DEFORM_KIND_U16>(A, tile, blocks, s);
}

}  // namespace unet
