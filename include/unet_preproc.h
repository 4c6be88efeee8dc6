/* C ABI of the pre-processing commands a model carries (run_preproc(model->preproc), evaluate.cpp:201; the command names are
 * evaluate.cpp:5-17), exported by libunet_hip.so.
 *
 * The names are in the reference tree; their bodies are TIPL's (tipl::filter::gaussian, tipl::filter::mean, tipl::downsampling,
 * tipl::upsampling, tipl::flip_*, tipl::swap_*, tipl::normalize) and are not, so what follows are this project's definitions:
 * parity with TIPL is NOT pinned.
 *
 * Volumes are fp32, W x H x D with x fastest, fewer than 2^31 voxels per grid; channels are stacked along z (channel c at
 * base + c * W*H*D).  Every command acts on each channel volume separately -- taps and cells never cross a channel boundary --
 * except normalize, which acts on the whole stacked buffer (tipl::normalize, train.cpp:30).
 *
 * unet_preproc_filter   out of place, 3x3x3, border voxels replicated, taps visited in (kz, ky, kx) order, fp32, no fused
 *   multiply-add:
 *     UNET_PREPROC_GAUSSIAN   the binomial (1,2,1)^3/64: acc = 0; acc += w * v per tap -- the project's stand-in for
 *                             tipl::filter::gaussian, bit-identical to simulate_modality's and gaussian_smoothing's filter
 *     UNET_PREPROC_MEAN       acc = 0; acc += v per tap; the result is acc * (1.0f / 27.0f)
 *   impl: UNET_PREPROC_IMPL_DEFAULT picks the shipped kernel; _LDS (a block marches along z, the planes staged in LDS, each
 *   thread's 27 taps in registers) and _VOXEL (one thread per voxel, 27 loads) name one; all give the same bits.
 * unet_preproc_downsample   dst is ceil(w/2) x ceil(h/2) x ceil(d/2): each voxel the fp32 sum, in (kz, ky, kx) order, of the source
 *   voxels of its 2x2x2 cell that exist, divided by their count.
 * unet_preproc_upsample     dst is 2w x 2h x 2d (refused at 2^31 voxels or more): dst voxel x samples the source LINEAR (the
 *   sampler of include/unet_space.h) at 0.5f*x - 0.25f per axis, clamped to [0, dim-1].
 * unet_preproc_permute      an exact copy: FLIP_X dst(x,y,z) = src(w-1-x,y,z) (FLIP_Y, FLIP_Z alike); SWAP_XY dst is h x w x d with
 *   dst(x,y,z) = src(y,x,z); SWAP_YZ dst is w x d x h with dst(x,y,z) = src(x,z,y); SWAP_XZ dst is d x h x w with
 *   dst(x,y,z) = src(z,y,x).
 * unet_preproc_normalize    in place: the `values` floats of the stacked buffer are divided by their maximum when that is > 0 (NaN
 *   values are skipped by the maximum).  The maximum is read on the device: no host sync, no float atomics.
 *   scratch: unet_preproc_scratch_bytes(values).
 *
 * w, h, d are always the SOURCE's dimensions.  Any 4-byte-aligned pointer works.  Argument errors (NULL, non-positive sizes,
 * src == dst, a grid of 2^31 voxels or more, more than 65535 channels, unknown kind / impl / op, scratch too small) are found before
 * any device call.  Everything runs on the caller's stream with the caller's buffers and scratch: calls on different streams with
 * different buffers may run concurrently.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_PREPROC_H
#define UNET_PREPROC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_PREPROC_GAUSSIAN = 0, UNET_PREPROC_MEAN = 1 };
enum { UNET_PREPROC_IMPL_DEFAULT = 0, UNET_PREPROC_IMPL_LDS = 1, UNET_PREPROC_IMPL_VOXEL = 2 };
enum { UNET_PREPROC_FLIP_X = 0, UNET_PREPROC_FLIP_Y = 1, UNET_PREPROC_FLIP_Z = 2,
       UNET_PREPROC_SWAP_XY = 3, UNET_PREPROC_SWAP_YZ = 4, UNET_PREPROC_SWAP_XZ = 5 };

int unet_preproc_filter(const float* src, float* dst, int w, int h, int d, int channels, int kind, int impl, void* stream);

int unet_preproc_downsample(const float* src, float* dst, int w, int h, int d, int channels, void* stream);

int unet_preproc_upsample(const float* src, float* dst, int w, int h, int d, int channels, void* stream);

int unet_preproc_permute(const float* src, float* dst, int w, int h, int d, int channels, int op, void* stream);

int unet_preproc_scratch_bytes(int64_t values, size_t* bytes);

int unet_preproc_normalize(float* buf, int64_t values, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
