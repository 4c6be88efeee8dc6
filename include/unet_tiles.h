/* C ABI of the evaluation of a scan larger than the model's field of view in overlapping tiles, exported by libunet_hip.so.
 *
 * The reference's evaluate_unet::evaluate() loops over several model_io chunks per file (evaluate.cpp:223-230); the code that makes
 * more than one chunk, TIPL's handle_fov_pre / handle_fov_post, is not in the reference tree.  The canvas, the plan, the weight and
 * the blend below are therefore this project's definitions: parity with TIPL is NOT pinned.
 *
 * CANVAS  a virtual grid at the model's voxel size that covers the scan: per axis max(model_dim, ceil(image_dim * image_vs /
 *   model_vs)), the ratio in float64, a ratio within 1e-6 of an integer counting as that integer (tiles.canvas_dims; host only).
 * PLAN    per axis, independently, from the tile size T (the model's dim), the canvas size C >= T and the overlap 0 <= ov < 0.5:
 *   O = ceil(ov*T), S = T - O, n = 1 when C == T, else 1 + ceil((C-T)/S); the integer origins o_i = (i*(C-T) + (n-1)/2) / (n-1)
 *   (integer divisions).  o_0 = 0, o_{n-1} = C-T, 0 < o_{i+1} - o_i <= S, n is minimal.  At most UNET_TILES_MAX_AXIS tiles per
 *   axis.  The tile index is (iz*ny + iy)*nx + ix.
 * WEIGHT  for the tile-local coordinate p on an axis of size T: w(p) = min(p, T-1-p) + 1; a voxel's weight in a tile is the product
 *   over the three axes, an exact integer in fp32 for T <= 512 (a larger tile dim is refused).
 * BLEND   for a canvas voxel and a class, over the tiles that cover the voxel: exactly one -> that tile's value, copied bit for bit;
 *   otherwise (sum_t w_t * x_t) / (sum_t w_t), both sums from +0 over the covering tiles in ascending tile index, in fp32, every
 *   product and every sum rounded (no fused multiply-add).  NaN and inf follow that arithmetic.
 *
 * tiles   the contiguous stack {nz*ny*nx, out_c, td, th, tw} of level-0 logits, fp32 (x fastest; any number of values)
 * canvas  {out_c, cd, ch, cw}, fp32, fewer than 2^31 voxels
 * The plan is read from HOST memory at the call and travels in the launch arguments.
 *
 * unet_tiles_blend     canvas = BLEND(tiles): one gather pass, the stack read once and the canvas written once:
 *   4 * out_c * (tiles * tile voxels + canvas voxels) bytes.
 * unet_tiles_postproc  the fused softmax / create_mask / argmax pass of include/unet_postproc.h (same definitions, same NULL-output
 *   rule, same NaN / inf rules) on the canvas, each logit it reads being the BLEND of the stack, never stored.  The results equal
 *   unet_tiles_blend + unet_postproc_softmax bit for bit.
 *
 * Any pointer alignment works.  Argument errors (NULL, non-positive sizes, n outside 1..UNET_TILES_MAX_AXIS, origins that do not
 * ascend, do not start at 0 or do not end at c - t, a step above the tile size, a canvas of 2^31 voxels or more, a tile dim above
 * UNET_TILES_MAX_DIM, out_c < 2 or > 65536, no output wanted) are found before any device call.  Everything runs on the caller's
 * stream and needs no scratch.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_TILES_H
#define UNET_TILES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_TILES_MAX_AXIS 16    /* tiles per axis */
#define UNET_TILES_MAX_DIM 512    /* voxels per tile axis: (T/2)^3 <= 2^24 */

typedef struct { int n[3]; int origin[3][UNET_TILES_MAX_AXIS]; } UnetTilePlan;   /* x, y, z */

int unet_tiles_blend(const float* tiles, int out_c, int tw, int th, int td, const UnetTilePlan* plan, int cw, int ch, int cd,
                     float* canvas, void* stream);

int unet_tiles_postproc(const float* tiles, int out_c, int tw, int th, int td, const UnetTilePlan* plan, int cw, int ch, int cd,
                        float threshold, float* label_prob, float* fg_prob, uint16_t* label, void* stream);

#ifdef __cplusplus
}
#endif
#endif
