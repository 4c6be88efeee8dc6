// A scan larger than the model's field of view, evaluated in overlapping tiles (include/unet_tiles.h): the blend of the tiles'
// logits onto the canvas.
//
//   k_tiles_blend     canvas voxel -> the tiles that cover it -> (sum w*x) / (sum w), or the one value bit for bit
//   k_tiles_postproc  the softmax / create_mask / argmax pass of kernels_postproc.hip on the canvas: each logit of a voxel is
//                     blended from the stack and fed to the same accumulator (pp_acc, device_util.h), as k_space_postproc does
//                     with interpolated logits, so the canvas logits are never stored
//
// Both are gathers, one thread per canvas voxel, walking the canvas in the 16 x 4 x 4 bricks of the other gather passes
// (brick_walk, device_util.h).  The tiles a BRICK meets are found once per block from the origins in the launch arguments (uniform:
// scalar loads and scalar loop bounds); a lane takes part in a tile under its own cover test.  The loop runs classes outside,
// tiles inside, the per-axis cover tests and weights hoisted to their loop level.  Every tile voxel belongs to exactly one canvas
// voxel, so a pass reads the stack once: a lane's row of 16 voxels is one 64-byte segment of a tile row, at whatever alignment the
// tile's integer origin gives it.  No LDS, no atomics, no scratch.  32-bit offsets inside a tile plane (<= 512^3 voxels) and inside
// a canvas plane, 64-bit plane bases.
#include "../../include/unet_tiles.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int TL_T = 256;
static_assert(BRICK_X * BRICK_Y * BRICK_Z == TL_T, "brick = block");

struct TileGrid {   // the canvas the threads walk and the tiles they read
    int W, H, D, gx, gy;
    int64_t S;
    int tw, th, td, C;
    int64_t tv;     // voxels of one tile plane
};

struct Cover {      // one lane's voxel and the tiles its brick meets (lo..hi per axis, uniform), its own cover count and weight sum
    int x, y, z;
    int lo[3], hi[3];
    int cnt;
    float den;
};

__device__ __forceinline__ int tile_w(int p, int T) { return min(p, T - 1 - p) + 1; }

// the tiles of one axis that meet [b0, b1]: a contiguous run, the origins ascend (uniform arguments, uniform result)
__device__ __forceinline__ void axis_range(const int* o, int n, int T, int b0, int b1, int& lo, int& hi) {
    lo = n;
    hi = -1;
    for (int i = 0; i < n; ++i)
        if (o[i] <= b1 && o[i] + T > b0) {
            lo = min(lo, i);
            hi = i;
        }
}

// walks the tiles of the lane's brick in ascending tile index; f(tile, offset inside a tile plane, weight) for those covering the lane
template <typename F> __device__ __forceinline__ void for_covering(const UnetTilePlan& P, const TileGrid& g, const Cover& k, F f) {
    for (int iz = k.lo[2]; iz <= k.hi[2]; ++iz) {
        const int lz = k.z - P.origin[2][iz];
        const bool cz = (unsigned)lz < (unsigned)g.td;
        const int wz = tile_w(lz, g.td);
        for (int iy = k.lo[1]; iy <= k.hi[1]; ++iy) {
            const int ly = k.y - P.origin[1][iy];
            const bool czy = cz && (unsigned)ly < (unsigned)g.th;
            const int wzy = wz * tile_w(ly, g.th);
            const int row = (lz * g.th + ly) * g.tw;
            const int t0 = (iz * P.n[1] + iy) * P.n[0];
            for (int ix = k.lo[0]; ix <= k.hi[0]; ++ix) {
                const int lx = k.x - P.origin[0][ix];
                if (czy && (unsigned)lx < (unsigned)g.tw) f(t0 + ix, (unsigned)(row + lx), (float)(wzy * tile_w(lx, g.tw)));   // <= 2^24: exact
            }
        }
    }
}

__device__ __forceinline__ bool tiles_cover(const UnetTilePlan& P, const TileGrid& g, Cover& k) {
#pragma clang fp contract(off)
    if (!brick_walk(g.W, g.H, g.D, g.gx, g.gy, k.x, k.y, k.z)) return false;
    // the brick's corner is the same in every lane of the block
    const int bx = __builtin_amdgcn_readfirstlane(k.x & ~(BRICK_X - 1)), by = __builtin_amdgcn_readfirstlane(k.y & ~(BRICK_Y - 1)),
              bz = __builtin_amdgcn_readfirstlane(k.z & ~(BRICK_Z - 1));
    axis_range(P.origin[0], P.n[0], g.tw, bx, bx + BRICK_X - 1, k.lo[0], k.hi[0]);
    axis_range(P.origin[1], P.n[1], g.th, by, by + BRICK_Y - 1, k.lo[1], k.hi[1]);
    axis_range(P.origin[2], P.n[2], g.td, bz, bz + BRICK_Z - 1, k.lo[2], k.hi[2]);
    int cnt = 0;
    float den = 0.f;
    for_covering(P, g, k, [&](int, unsigned, float w) { ++cnt; den += w; });
    k.cnt = cnt;
    k.den = den;
    return true;
}

// BLEND of include/unet_tiles.h for class c at the lane's voxel
__device__ __forceinline__ float tiles_blend_at(const float* __restrict__ tiles, const UnetTilePlan& P, const TileGrid& g, const Cover& k,
                                                int c) {
#pragma clang fp contract(off)
    float num = 0.f, one = 0.f;
    for_covering(P, g, k, [&](int t, unsigned off, float w) {
        const float x = tiles[((int64_t)t * g.C + c) * g.tv + off];
        one = x;
        num += w * x;
    });
    return k.cnt == 1 ? one : num / k.den;
}

__global__ void __launch_bounds__(TL_T) k_tiles_blend(const float* __restrict__ tiles, TileGrid g, UnetTilePlan P, float* __restrict__ canvas) {
    Cover k;
    if (!tiles_cover(P, g, k)) return;
    const int64_t v = ((int64_t)k.z * g.H + k.y) * g.W + k.x;
    for (int c = 0; c < g.C; ++c) canvas[c * g.S + v] = tiles_blend_at(tiles, P, g, k, c);
}

// k_pp_softmax<1>'s body with x_c = the blend in place of the load: same order of pp_acc calls, same argmax rule
__global__ void __launch_bounds__(TL_T) k_tiles_postproc(const float* __restrict__ tiles, TileGrid g, UnetTilePlan P, float thr,
                                                         float* __restrict__ lp, float* __restrict__ fg, uint16_t* __restrict__ lab) {
    Cover k;
    if (!tiles_cover(P, g, k)) return;
    const int64_t v = ((int64_t)k.z * g.H + k.y) * g.W + k.x;
    const int C = g.C;
    float m = -INFINITY, s = 0.f, sf = 0.f, best = 0.f;
    int arg = 1;
    pp_acc(tiles_blend_at(tiles, P, g, k, 0), m, s, sf, 0.f);
    for (int c = 1; c < C; ++c) {
        const float xc = tiles_blend_at(tiles, P, g, k, c);
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
        for (int c = 1; c < C; ++c) {
            const float xc = tiles_blend_at(tiles, P, g, k, c);
            lp[(c - 1) * g.S + v] = bad ? NAN : expf(xc - m) / s;
        }
    }
}

TileGrid tile_grid(int C, int tw, int th, int td, int cw, int ch, int cd) {
    return TileGrid{cw, ch, cd, (cw + BRICK_X - 1) / BRICK_X, (ch + BRICK_Y - 1) / BRICK_Y, (int64_t)cw * ch * cd, tw, th, td, C,
                    (int64_t)tw * th * td};
}

}  // namespace

void launch_tiles_blend(const float* tiles, int C, int tw, int th, int td, const UnetTilePlan& plan, int cw, int ch, int cd, float* canvas,
                        hipStream_t s) {
    k_tiles_blend<<<(unsigned)space_bricks(cw, ch, cd), TL_T, 0, s>>>(tiles, tile_grid(C, tw, th, td, cw, ch, cd), plan, canvas);
}

void launch_tiles_postproc(const float* tiles, int C, int tw, int th, int td, const UnetTilePlan& plan, int cw, int ch, int cd, float thr,
                           float* lp, float* fg, uint16_t* lab, hipStream_t s) {
    k_tiles_postproc<<<(unsigned)space_bricks(cw, ch, cd), TL_T, 0, s>>>(tiles, tile_grid(C, tw, th, td, cw, ch, cd), plan, thr, lp, fg, lab);
}

}  // namespace unet
