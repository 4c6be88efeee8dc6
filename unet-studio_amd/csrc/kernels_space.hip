// Between a scan's own grid and the model's grid (include/unet_space.h; read_image_and_label train.cpp:13-40, handle_fov_post before
// run_postproc evaluate.cpp:274).
//
//   k_space_resample<MODE>  dst voxel -> map -> source position -> trilinear / majority gather, every channel from one footprint.
//                           With normalize the finished buffer goes through the feed's max + divide (launch_feed_prepare: block
//                           partials, a fold, x / max when max > 0): no host sync, no float atomics
//   k_space_postproc        the softmax / create_mask / argmax pass of kernels_postproc.hip on the native grid: each of the out_c
//                           logits of a native voxel is interpolated from the model-grid planes and fed to the same accumulator
//                           (pp_acc, device_util.h), so the out_c native-size planes are never stored
//
// Both walk the destination in the 16 x 4 x 4 bricks of the augmentation's gather passes (brick_walk, device_util.h): the 256
// footprints of a block overlap in a compact source region that stays in the CU's L1, and each XCD works through one z-range.
// The footprint (8 corner offsets, 3 fractions) is computed once per voxel; the loop runs planes outside, corners inside, so the
// lanes of a wave load corner k of plane c together from a few rows of one brick footprint.  32-bit offsets inside a plane.
#include "../../include/unet_space.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int SP_T = 256;
static_assert(BRICK_X * BRICK_Y * BRICK_Z == SP_T, "brick = block");

struct SpaceGrid {   // the grid the threads walk
    int W, H, D, gx, gy;
    int64_t S;
};

SpaceGrid space_grid(int w, int h, int d) {
    return SpaceGrid{w, h, d, (w + BRICK_X - 1) / BRICK_X, (h + BRICK_Y - 1) / BRICK_Y, (int64_t)w * h * d};
}

// map(x, y, z) in fp32, left to right, no fused multiply-add: oracle/augment_ref.py _affine rounds identically
__device__ __forceinline__ Tri space_locate(const UnetSpaceMap& a, int xi, int yi, int zi, int sw, int sh, int sd) {
#pragma clang fp contract(off)
    const float x = (float)xi, y = (float)yi, z = (float)zi;
    const float px = a.m[0] * x + a.m[1] * y + a.m[2] * z + a.t[0];
    const float py = a.m[3] * x + a.m[4] * y + a.m[5] * z + a.t[1];
    const float pz = a.m[6] * x + a.m[7] * y + a.m[8] * z + a.t[2];
    return locate(px, py, pz, sw, sh, sd);
}

template <int MODE>
__global__ void __launch_bounds__(SP_T) k_space_resample(const float* __restrict__ src, int sw, int sh, int sd, float* __restrict__ dst,
                                                         SpaceGrid g, int channels, UnetSpaceMap map) {
    int x, y, z;
    if (!brick_walk(g.W, g.H, g.D, g.gx, g.gy, x, y, z)) return;
    const int64_t i = ((int64_t)z * g.H + y) * g.W + x;
    const int64_t ss = (int64_t)sw * sh * sd;
    const Tri t = space_locate(map, x, y, z, sw, sh, sd);
    for (int c = 0; c < channels; ++c) {
        float v = 0.f;
        if (t.ok) v = MODE == UNET_SPACE_MAJORITY ? majority(t, src + c * ss) : trilinear(t, src + c * ss);
        dst[c * g.S + i] = v;
    }
}

// k_pp_softmax<1>'s body with x_c = trilinear(plane c) in place of the load: same order of pp_acc calls, same argmax rule
__global__ void __launch_bounds__(SP_T) k_space_postproc(const float* __restrict__ lg, int C, int mw, int mh, int md, SpaceGrid g,
                                                         UnetSpaceMap map, float thr, float* __restrict__ lp, float* __restrict__ fg,
                                                         uint16_t* __restrict__ lab) {
    int x, y, z;
    if (!brick_walk(g.W, g.H, g.D, g.gx, g.gy, x, y, z)) return;
    const int64_t v = ((int64_t)z * g.H + y) * g.W + x;
    const int64_t sm = (int64_t)mw * mh * md;
    const Tri t = space_locate(map, x, y, z, mw, mh, md);
    if (!t.ok) {   // outside the model's field of view: background, not the softmax of nothing
        if (fg) fg[v] = 0.f;
        if (lab) lab[v] = 0;
        if (lp)
            for (int c = 1; c < C; ++c) lp[(c - 1) * g.S + v] = 0.f;
        return;
    }
    float m = -INFINITY, s = 0.f, sf = 0.f, best = 0.f;
    int arg = 1;
    pp_acc(trilinear(t, lg), m, s, sf, 0.f);
#pragma unroll 2
    for (int c = 1; c < C; ++c) {
        const float xc = trilinear(t, lg + c * sm);
        pp_acc(xc, m, s, sf, 1.f);
        if (c == 1 || xc > best) { best = xc; arg = c; }   // torch.argmax: the first index wins a tie
    }
    const bool bad = !(fabsf(m) < INFINITY) || s != s;
    if (fg || lab) {
        const float f = bad ? NAN : sf / s;
        if (fg) fg[v] = f;
        if (lab) lab[v] = f > thr ? (uint16_t)arg : (uint16_t)0;   // NaN > thr is false
    }
    if (lp) {
#pragma unroll 2
        for (int c = 1; c < C; ++c) {
            const float xc = trilinear(t, lg + c * sm);
            lp[(c - 1) * g.S + v] = bad ? NAN : expf(xc - m) / s;
        }
    }
}

size_t sp_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// bricks of a w x h x d grid, rounded up to a multiple of 8 (brick_walk's renumbering)
int64_t space_bricks(int w, int h, int d) {
    const int64_t b = (int64_t)((w + BRICK_X - 1) / BRICK_X) * ((h + BRICK_Y - 1) / BRICK_Y) * ((d + BRICK_Z - 1) / BRICK_Z);
    return (b + 7) / 8 * 8;
}

// the feed's reduction scratch for the stacked buffer, and 256 B of slack for any scratch alignment
size_t space_scratch_bytes(int64_t dst_voxels, int channels) { return 256 + feed_scratch_bytes(dst_voxels * channels); }

void launch_space_resample(const float* src, int sw, int sh, int sd, float* dst, int dw, int dh, int dd, int channels,
                           const UnetSpaceMap& map, int mode, int normalize, void* scratch, hipStream_t s) {
    const SpaceGrid g = space_grid(dw, dh, dd);
    const unsigned nb = (unsigned)space_bricks(dw, dh, dd);
    if (mode == UNET_SPACE_MAJORITY) k_space_resample<UNET_SPACE_MAJORITY><<<nb, SP_T, 0, s>>>(src, sw, sh, sd, dst, g, channels, map);
    else k_space_resample<UNET_SPACE_LINEAR><<<nb, SP_T, 0, s>>>(src, sw, sh, sd, dst, g, channels, map);
    // tipl::normalize on the whole stacked buffer: no image0, no shift, no label maximum wanted
    if (normalize)
        launch_feed_prepare(nullptr, dst, g.S * channels, 1, 0, nullptr, (void*)sp_align((size_t)(uintptr_t)scratch), s);
}

void launch_space_postproc(const float* logits, int C, int mw, int mh, int md, const UnetSpaceMap& map, int nw, int nh, int nd, float thr,
                           float* lp, float* fg, uint16_t* lab, hipStream_t s) {
    k_space_postproc<<<(unsigned)space_bricks(nw, nh, nd), SP_T, 0, s>>>(logits, C, mw, mh, md, space_grid(nw, nh, nd), map, thr, lp, fg,
                                                                        lab);
}

}  // namespace unet
