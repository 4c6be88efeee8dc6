/* C ABI of the step between a scan's own grid and the model's grid (read_image_and_label, train.cpp:13-40; handle_fov_post before
 * run_postproc, evaluate.cpp:274), exported by libunet_hip.so.
 *
 * The way in is written out in the reference tree; the sampling rules it calls (tipl::linear, tipl::majority, tipl::normalize,
 * tipl::transformation_matrix) are TIPL's and not in it, so they are this project's definitions, the ones the augmentation already
 * uses (include/unet_augment.h, oracle/augment_ref.py): parity with TIPL is NOT pinned.
 *
 * Volumes are fp32, W x H x D with x fastest, fewer than 2^31 voxels per grid; channels / planes are stacked along z (plane c at
 * base + c * W*H*D).  A UnetSpaceMap takes a DESTINATION voxel (x, y, z) to a SOURCE position in voxel units:
 *     px = m0*x + m1*y + m2*z + t0      py = m3*x + m4*y + m5*z + t1      pz = m6*x + m7*y + m8*z + t2
 *   evaluated in fp32 in exactly that order (left to right, every product and every sum rounded: no fused multiply-add).
 *   inside    0 <= p <= dim-1 on every axis of the source; a NaN position is outside
 *   corners   the lower neighbour floor(p), the upper neighbour min(floor(p)+1, dim-1), the fraction t = p - floor(p)
 *   LINEAR    a + t*(b - a) along x for the four corner pairs, then along y, then along z (each step rounded)
 *   MAJORITY  the corner value with the largest summed trilinear weight ((1-tx | tx) * (1-ty | ty) * (1-tz | tz), summed in corner
 *             order, x fastest); the first corner wins a tie
 * The map is read from HOST memory at the call and travels in the launch arguments.
 *
 * unet_space_resample   dst[c] = sample(src[c]) at map(dst voxel) for every channel; a voxel whose position is outside gets 0.
 *   normalize != 0 (LINEAR only): afterwards the whole stacked dst buffer is divided by its maximum when that is > 0
 *   (tipl::normalize, train.cpp:30; NaN voxels are skipped by the maximum).  The maximum is read on the device: no host sync.
 *   scratch: unet_space_scratch_bytes(dst voxels, channels); needed only with normalize (NULL / 0 otherwise).
 *
 * unet_space_postproc   the fused softmax / create_mask / argmax pass of include/unet_postproc.h (same definitions, same
 *   NULL-output rule, same NaN / inf rules) evaluated on the native grid nw x nh x nd: the out_c logits of a native voxel are the
 *   LINEAR samples of the model-grid planes (mw x mh x md) at map(native voxel), never stored.  A native voxel whose position is
 *   outside the model grid gets label 0, fg_prob 0 and label_prob 0 in every plane -- not the softmax of all-zero logits, whose
 *   fg_prob (C-1)/C would label everything outside the model's field of view 1.  Inside, the results equal
 *   unet_space_resample(LINEAR) + unet_postproc_softmax bit for bit.
 *
 * Any pointer alignment works.  Argument errors (NULL, non-positive sizes, a grid of 2^31 voxels or more, unknown mode, normalize
 * with MAJORITY, out_c < 2 or > 65536, scratch too small) are found before any device call.  Everything runs on the caller's stream
 * with the caller's scratch: calls on different streams with different scratch may run concurrently.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_SPACE_H
#define UNET_SPACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float m[9]; float t[3]; } UnetSpaceMap;   /* p_src = m (row-major) * (x,y,z)_dst + t, voxel units, x fastest */
enum { UNET_SPACE_LINEAR = 0, UNET_SPACE_MAJORITY = 1 };

int unet_space_scratch_bytes(int64_t dst_voxels, int channels, size_t* bytes);

int unet_space_resample(const float* src, int sw, int sh, int sd, float* dst, int dw, int dh, int dd, int channels,
                        const UnetSpaceMap* map, int mode, int normalize, void* scratch, size_t scratch_bytes, void* stream);

int unet_space_postproc(const float* logits, int out_c, int mw, int mh, int md, const UnetSpaceMap* map,
                        int nw, int nh, int nd, float threshold, float* label_prob, float* fg_prob, uint16_t* label, void* stream);

#ifdef __cplusplus
}
#endif
#endif
