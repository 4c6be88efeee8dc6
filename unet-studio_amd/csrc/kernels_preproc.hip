// The pre-processing commands a model carries (include/unet_preproc.h; run_preproc, evaluate.cpp:201).
//
//   k_preproc_filter_lds<KIND>    the 3x3x3 filters, the hot path.  A block of 256 threads owns a 32 x 8 tile in (x, y) of one channel
//                                 and marches along z through a chunk of PF_ZC planes.  Per step it stages ONE halo'd plane
//                                 (34 x 10, border voxels already replicated by clamped loads) in LDS, double buffered, one barrier
//                                 per step; each thread reads its 3 x 3 of the new plane and keeps the two planes before it in
//                                 registers, so a source voxel is fetched from global memory once per block that needs it
//                                 (1.33x for the x/y halo, 34/32 for the chunk ends) instead of 27 times per voxel, and LDS
//                                 serves 9 reads per voxel, not 27.  The 27 taps are then accumulated in (kz, ky, kx) order
//                                 exactly as binomial3 (device_util.h) does, so the bits are those of the per-voxel form.
//                                 The next plane's global loads are issued before the current plane's arithmetic.
//                                 LDS rows are 34 dwords: a wave reads two rows of 32 consecutive dwords per instruction, the
//                                 two 32-lane halves of ds_read_b32 never conflict; the staging writes are consecutive dwords.
//   k_preproc_filter_voxel<KIND>  one thread per voxel over binomial3 / its mean twin: the baseline
//   k_preproc_downsample / _upsample / _permute   one thread per destination voxel, channel = blockIdx.y
//   normalize                     the feed's max + divide (launch_feed_prepare: block partials, a fold, x / max when max > 0)
#include "../../include/unet_preproc.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int PF_T = 256, PF_TX = 32, PF_TY = 8, PF_ZC = 32;
constexpr int PF_LW = PF_TX + 2, PF_LH = PF_TY + 2, PF_N = PF_LW * PF_LH;   // the halo'd plane tile: 340 floats
static_assert(PF_TX * PF_TY == PF_T && PF_N <= 2 * PF_T, "one or two staged values per thread");

struct FilterGrid {   // tiles along x and y, chunks along z, blocks in all (before rounding up to a multiple of 8)
    int W, H, D, gx, gy, gz;
    unsigned nb;
    int64_t S;
};

// 27 taps of the three 3x3 windows a (z-1), b (z), c (z+1), each [ky*3 + kx], in (kz, ky, kx) order
template <int KIND>
__device__ __forceinline__ float filter27(const float (&a)[9], const float (&b)[9], const float (&c)[9]) {
#pragma clang fp contract(off)   // w * v then + in fp32, as binomial3 and oracle/augment_ref.py:_smooth round
    float acc = 0.f;
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = kz == 0 ? a[k] : kz == 1 ? b[k] : c[k];
            if constexpr (KIND == UNET_PREPROC_GAUSSIAN) {
                const float w = (float)((kz == 1 ? 2 : 1) * (k / 3 == 1 ? 2 : 1) * (k % 3 == 1 ? 2 : 1)) * (1.0f / 64.0f);
                acc += w * v;
            } else {
                acc += v;
            }
        }
    }
    if constexpr (KIND == UNET_PREPROC_MEAN) acc = acc * (1.0f / 27.0f);
    return acc;
}

template <int KIND>
__global__ void __launch_bounds__(PF_T) k_preproc_filter_lds(const float* __restrict__ src, float* __restrict__ dst, FilterGrid g) {
    __shared__ float tile[2][PF_N];
    // blocks are dealt round-robin to the 8 XCDs: renumber so each XCD works through one contiguous run of tiles (brick_walk's rule)
    const unsigned per = gridDim.x / 8;
    unsigned b = (blockIdx.x & 7) * per + (blockIdx.x >> 3);   // uniform
    if (b >= g.nb) return;                                     // the whole block leaves before any barrier
    const int bx = b % g.gx; b /= g.gx;
    const int by = b % g.gy; b /= g.gy;
    const int bz = b % g.gz;
    const int64_t cbase = (int64_t)(b / g.gz) * g.S;
    const float* __restrict__ s = src + cbase;
    float* __restrict__ d = dst + cbase;
    const int x0 = bx * PF_TX, y0 = by * PF_TY, zs = bz * PF_ZC, ze = min(zs + PF_ZC, g.D);
    const unsigned WH = (unsigned)g.W * (unsigned)g.H;
    const int t = threadIdx.x;
    // the one or two values of a halo'd plane this thread stages: replicated borders = clamped coordinates
    const int k1 = t + PF_T;
    const bool has1 = k1 < PF_N;
    const unsigned o0 = (unsigned)min(max(y0 + t / PF_LW - 1, 0), g.H - 1) * g.W + min(max(x0 + t % PF_LW - 1, 0), g.W - 1);
    const unsigned o1 = has1 ? (unsigned)min(max(y0 + k1 / PF_LW - 1, 0), g.H - 1) * g.W + min(max(x0 + k1 % PF_LW - 1, 0), g.W - 1) : o0;
    const int lx = t & (PF_TX - 1), ly = t / PF_TX;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < g.W && y < g.H;
    const unsigned out = (unsigned)y * g.W + x;
    const int l0 = ly * PF_LW + lx;

    float r0, r1;
    {
        const unsigned po = (unsigned)min(max(zs - 1, 0), g.D - 1) * WH;
        r0 = s[po + o0];
        r1 = s[po + o1];
        tile[0][t] = r0;
        if (has1) tile[0][k1] = r1;
    }
    __syncthreads();
    float wa[9], wb[9] = {}, wc[9] = {};
    int buf = 0;
    for (int p = zs - 1; p <= ze; ++p) {   // tile[buf] holds plane p (clamped); outputs zs .. ze-1
        const bool more = p < ze;
        if (more) {                        // plane p+1: in flight under the arithmetic below
            const unsigned po = (unsigned)min(max(p + 1, 0), g.D - 1) * WH;
            r0 = s[po + o0];
            r1 = s[po + o1];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            wa[k] = wb[k];
            wb[k] = wc[k];
            wc[k] = tile[buf][l0 + (k / 3) * PF_LW + k % 3];
        }
        if (p > zs && inside) d[(unsigned)(p - 1) * WH + out] = filter27<KIND>(wa, wb, wc);
        if (more) {                        // the other buffer was last read one step ago, before that step's barrier
            tile[buf ^ 1][t] = r0;
            if (has1) tile[buf ^ 1][k1] = r1;
        }
        __syncthreads();
        buf ^= 1;
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) k_preproc_filter_voxel(const float* __restrict__ src, float* __restrict__ dst, int W, int H, int D) {
    const unsigned S = (unsigned)W * H * D;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= S) return;
    const float* __restrict__ s = src + (int64_t)blockIdx.y * S;
    const int x = i % W, y = (i / W) % H, z = i / ((unsigned)W * H);
    float v;
    if constexpr (KIND == UNET_PREPROC_GAUSSIAN) {
        v = binomial3(W, H, D, x, y, z, [&](unsigned j) { return s[j]; });
    } else {
#pragma clang fp contract(off)
        float acc = 0.f;
        for (int kz = 0; kz < 3; ++kz) {
            const int zz = min(max(z + kz - 1, 0), D - 1);
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = min(max(y + ky - 1, 0), H - 1);
                for (int kx = 0; kx < 3; ++kx) acc += s[(unsigned)((zz * H + yy) * W + min(max(x + kx - 1, 0), W - 1))];
            }
        }
        v = acc * (1.0f / 27.0f);
    }
    dst[(int64_t)blockIdx.y * S + i] = v;
}

// dst voxel i of a dw x dh x dd grid -> (x, y, z); false past the end
__device__ __forceinline__ bool dst_voxel(int dw, int dh, int dd, unsigned& i, int& x, int& y, int& z) {
    i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)dw * dh * dd) return false;
    x = i % dw; y = (i / dw) % dh; z = i / ((unsigned)dw * dh);
    return true;
}

__global__ void __launch_bounds__(256) k_preproc_downsample(const float* __restrict__ src, float* __restrict__ dst, int W, int H, int D,
                                                            int dw, int dh, int dd) {
#pragma clang fp contract(off)
    unsigned i;
    int x, y, z;
    if (!dst_voxel(dw, dh, dd, i, x, y, z)) return;
    const float* __restrict__ s = src + (int64_t)blockIdx.y * ((int64_t)W * H * D);
    float acc = 0.f;
    int n = 0;
    for (int kz = 0; kz < 2; ++kz)
        for (int ky = 0; ky < 2; ++ky)
            for (int kx = 0; kx < 2; ++kx) {
                const int xx = 2 * x + kx, yy = 2 * y + ky, zz = 2 * z + kz;
                if (xx < W && yy < H && zz < D) {
                    acc += s[(unsigned)((zz * H + yy) * W + xx)];
                    ++n;
                }
            }
    dst[(int64_t)blockIdx.y * ((int64_t)dw * dh * dd) + i] = acc / (float)n;   // n is 1, 2, 4 or 8
}

__global__ void __launch_bounds__(256) k_preproc_upsample(const float* __restrict__ src, float* __restrict__ dst, int W, int H, int D) {
#pragma clang fp contract(off)
    unsigned i;
    int x, y, z;
    if (!dst_voxel(2 * W, 2 * H, 2 * D, i, x, y, z)) return;
    const float px = fminf(fmaxf(0.5f * (float)x - 0.25f, 0.f), (float)(W - 1));
    const float py = fminf(fmaxf(0.5f * (float)y - 0.25f, 0.f), (float)(H - 1));
    const float pz = fminf(fmaxf(0.5f * (float)z - 0.25f, 0.f), (float)(D - 1));
    const Tri t = locate(px, py, pz, W, H, D);   // always inside after the clamp
    const int64_t S = (int64_t)W * H * D;
    dst[(int64_t)blockIdx.y * 8 * S + i] = t.ok ? trilinear(t, src + (int64_t)blockIdx.y * S) : 0.f;
}

__global__ void __launch_bounds__(256) k_preproc_permute(const float* __restrict__ src, float* __restrict__ dst, int W, int H, int D,
                                                         int dw, int dh, int dd, int op) {
    unsigned i;
    int x, y, z;
    if (!dst_voxel(dw, dh, dd, i, x, y, z)) return;
    int sx = x, sy = y, sz = z;
    switch (op) {
        case UNET_PREPROC_FLIP_X: sx = W - 1 - x; break;
        case UNET_PREPROC_FLIP_Y: sy = H - 1 - y; break;
        case UNET_PREPROC_FLIP_Z: sz = D - 1 - z; break;
        case UNET_PREPROC_SWAP_XY: sx = y; sy = x; break;
        case UNET_PREPROC_SWAP_YZ: sy = z; sz = y; break;
        default: sx = z; sz = x; break;   // UNET_PREPROC_SWAP_XZ
    }
    const int64_t S = (int64_t)W * H * D;
    dst[blockIdx.y * S + i] = src[blockIdx.y * S + (unsigned)((sz * H + sy) * W + sx)];
}

FilterGrid filter_grid(int w, int h, int d, int channels) {
    FilterGrid g{w, h, d, (w + PF_TX - 1) / PF_TX, (h + PF_TY - 1) / PF_TY, (d + PF_ZC - 1) / PF_ZC, 0, (int64_t)w * h * d};
    g.nb = (unsigned)((int64_t)g.gx * g.gy * g.gz * channels);
    return g;
}

dim3 voxel_grid(int64_t voxels, int channels) { return dim3(cdiv64(voxels, 256), (unsigned)channels); }

size_t preproc_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// blocks of the LDS filter over a w x h x d x channels buffer, rounded up to a multiple of 8
int64_t preproc_filter_blocks(int w, int h, int d, int channels) {
    const int64_t b = (int64_t)((w + PF_TX - 1) / PF_TX) * ((h + PF_TY - 1) / PF_TY) * ((d + PF_ZC - 1) / PF_ZC) * channels;
    return (b + 7) / 8 * 8;
}

void launch_preproc_filter(const float* src, float* dst, int w, int h, int d, int channels, int kind, int impl, hipStream_t s) {
    if (impl == UNET_PREPROC_IMPL_VOXEL) {
        const dim3 grid = voxel_grid((int64_t)w * h * d, channels);
        if (kind == UNET_PREPROC_MEAN) k_preproc_filter_voxel<UNET_PREPROC_MEAN><<<grid, 256, 0, s>>>(src, dst, w, h, d);
        else k_preproc_filter_voxel<UNET_PREPROC_GAUSSIAN><<<grid, 256, 0, s>>>(src, dst, w, h, d);
        return;
    }
    const FilterGrid g = filter_grid(w, h, d, channels);
    const unsigned nb = (unsigned)preproc_filter_blocks(w, h, d, channels);
    if (kind == UNET_PREPROC_MEAN) k_preproc_filter_lds<UNET_PREPROC_MEAN><<<nb, PF_T, 0, s>>>(src, dst, g);
    else k_preproc_filter_lds<UNET_PREPROC_GAUSSIAN><<<nb, PF_T, 0, s>>>(src, dst, g);
}

void launch_preproc_downsample(const float* src, float* dst, int w, int h, int d, int channels, hipStream_t s) {
    const int dw = (w + 1) / 2, dh = (h + 1) / 2, dd = (d + 1) / 2;
    k_preproc_downsample<<<voxel_grid((int64_t)dw * dh * dd, channels), 256, 0, s>>>(src, dst, w, h, d, dw, dh, dd);
}

void launch_preproc_upsample(const float* src, float* dst, int w, int h, int d, int channels, hipStream_t s) {
    k_preproc_upsample<<<voxel_grid(8 * (int64_t)w * h * d, channels), 256, 0, s>>>(src, dst, w, h, d);
}

void launch_preproc_permute(const float* src, float* dst, int w, int h, int d, int channels, int op, hipStream_t s) {
    int dw = w, dh = h, dd = d;
    if (op == UNET_PREPROC_SWAP_XY) { dw = h; dh = w; }
    if (op == UNET_PREPROC_SWAP_YZ) { dh = d; dd = h; }
    if (op == UNET_PREPROC_SWAP_XZ) { dw = d; dd = w; }
    k_preproc_permute<<<voxel_grid((int64_t)w * h * d, channels), 256, 0, s>>>(src, dst, w, h, d, dw, dh, dd, op);
}

// the feed's reduction scratch for the stacked buffer, and 256 B of slack for any scratch alignment
size_t preproc_scratch_bytes(int64_t values) { return 256 + feed_scratch_bytes(values); }

// tipl::normalize on the whole stacked buffer: no image0, no shift, no label maximum wanted
void launch_preproc_normalize(float* buf, int64_t values, void* scratch, hipStream_t s) {
    launch_feed_prepare(nullptr, buf, values, 1, 0, nullptr, (void*)preproc_align((size_t)(uintptr_t)scratch), s);
}

}  // namespace unet
