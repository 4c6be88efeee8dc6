/* C ABI of the patch feed: training windows of model.dim cut out of a canvas larger than the field of view, class-balanced, on the
 * device; exported by libunet_hip.so.
 *
 * EvaluateUNet(fov_strategy="tiles") covers a scan larger than the model's field of view with windows of model.dim (unet_tiles.h).
 * This is the training-time counterpart: a window of a resident canvas is chosen around a voxel of a wanted class and cut out,
 * without the host reading anything back per sample.  The reference has no such code (its reader resamples every scan to model.dim,
 * train.cpp:13-40), so the definitions below are this project's.  Every choice is made on integer counts.
 *
 * CANVAS  a label volume {D, H, W} and an image {channels, D, H, W}, fp32, x fastest, fewer than 2^31 voxels (V = W*H*D).  The linear
 *   index of a voxel is v = (z*H + y)*W + x.
 * CLASS   of a voxel with label value l, for `classes` = K in 1..UNET_PATCHES_MAX_CLASSES: c = (int)l, toward zero, when 0 <= c < K
 *   (that is, when -1 < l < K); otherwise the voxel has no class; NaN has none.  For `classes` = 0 (continuous labels): class 1 when
 *   l > 0, else class 0 (NaN: 0), and K = 2.
 * INDEX   over the label in linear order, in segments of UNET_PATCHES_SEGMENT = 1024 consecutive voxels, S = ceil(V / 1024) of them
 *   (the last one may be short).  int32[K + K*S]:
 *     index[c]               c in 0..K-1   the number of voxels of class c (the totals, first: the host reads K words)
 *     index[K + c*S + s]     s in 0..S-1   the number of voxels of class c in the segments before s (an exclusive prefix)
 * PICK    (cls, u_rank, u_x, u_y, u_z): an int32 class and four uint32 draws.  With T the window and C the canvas size of an axis:
 *   when 0 <= cls < K and n = index[cls] > 0 (the class rule, flag 1):
 *     r      = (u_rank * n) >> 32                 in 64-bit integers: 0 <= r < n
 *     centre = the r-th voxel of class cls in linear order
 *     origin = clamp(centre - ((u * T) >> 32), 0, C - T)   per axis, with that axis' centre coordinate and draw: the chosen voxel
 *              lands at a uniformly drawn position inside the window, and the window stays inside the canvas
 *   otherwise (cls = -1, cls outside 0..K-1, or a class without voxels: the uniform rule, flag 0):
 *     origin = (u * (C - T + 1)) >> 32            per axis
 *   The result is int32[4] per pick: origin x, y, z and the flag.  If the index does not belong to the label (a stale index) and the
 *   segment holds fewer voxels of the class than the index says, the centre is the segment's first voxel and the flag is 0.
 * DRAWS   a pure function of (seed, sample index, k), all arithmetic modulo 2^64:
 *     mix(z)  : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31     (splitmix64's finaliser)
 *     draw(seed, index, k) = mix(mix(mix(seed + G) ^ index) + (k + 1) * G) >> 32,      G = 0x9E3779B97F4A7C15
 *   The feed uses k = 0 for the foreground decision, 1 for the class, 2 for u_rank and 3, 4, 5 for u_x, u_y, u_z.
 *
 * unet_patches_index   builds the INDEX: one block per segment counts, one block per class forms the prefix and the total.  The label
 *   may start at any 4-byte alignment.  4 * V bytes read.
 * unet_patches_pick    n <= UNET_PATCHES_MAX_PICKS picks, read from HOST memory at the call; they travel in the launch arguments (no
 *   host-to-device copy).  One block of one wave per pick: a binary search of the prefix table (32 steps at most), then the voxel
 *   inside the segment with ballots and popcounts (16 steps).  Every loop has a fixed bound.  origins: device int32[n][4].
 * unet_patches_crop    x {channels, td, th, tw} = the window of the image, lab {td, th, tw} = the window of the label (lab and label
 *   may both be NULL), copied bit for bit (NaN payloads survive).  origin: DEVICE int32[3] (x, y, z), typically a row of
 *   unet_patches_pick; the kernel clamps each word into [0, C - T] itself, so whatever the three words hold it reads inside the
 *   canvas.  Source and destination may start at any 4-byte alignment; stores are 16 bytes wide when tw is a multiple of 4 and x and
 *   lab are 16-byte aligned.
 * unet_patches_draws   out[i] = draw(seed, index, first_k + i) for i in 0..count-1; host only.
 *
 * Argument errors (NULL, non-positive sizes, a canvas of 2^31 voxels or more, classes outside 0..256, a window larger than the canvas,
 * n outside 1..32, an index buffer too small) are found before any device call.  Everything runs on the caller's stream; the index
 * memory is the caller's and no other scratch is needed.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_PATCHES_H
#define UNET_PATCHES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_PATCHES_SEGMENT 1024       /* voxels per index segment */
#define UNET_PATCHES_MAX_CLASSES 256
#define UNET_PATCHES_MAX_PICKS 32       /* picks per launch */

typedef struct { int32_t cls; uint32_t u_rank, u_x, u_y, u_z; } UnetPatchPick;

int unet_patches_index_bytes(int64_t voxels, int classes, size_t* bytes);

int unet_patches_index(const float* label, int64_t voxels, int classes, int32_t* index, size_t index_bytes, void* stream);

int unet_patches_pick(const float* label, const int32_t* index, int classes, int W, int H, int D, int tw, int th, int td,
                      const UnetPatchPick* picks, int n, int32_t* origins, void* stream);

int unet_patches_crop(const float* image, int channels, const float* label, int W, int H, int D, int tw, int th, int td,
                      const int32_t* origin, float* x, float* lab, void* stream);

int unet_patches_draws(uint64_t seed, uint64_t index, uint32_t first_k, int count, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif
