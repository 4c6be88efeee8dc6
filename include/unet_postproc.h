/* C ABI of the inference post-processing chain (postproc, unet.cpp:112; evaluate.cpp:274,303-376), exported by libunet_hip.so.
 *
 * The definitions are this project's: TIPL's run_postproc, softmax, argmax, defragment_by_size_ratio and normalize are not in the
 * reference tree, so parity with TIPL is NOT pinned (as for the augmentation).
 *
 * Input: the level-0 logits {C, S} of one volume, fp32, NCDHW (S = D*H*W voxels, plane c at logits + c*S), channel 0 the
 * background (as calc_losses treats it, train.cpp:501-552).  C >= 2 and C-1 <= 65535.  A result holds up to three outputs:
 *   label_prob  the C-1 foreground probability planes {C-1, S}, fp32
 *   fg_prob     one plane {S}, fp32
 *   label       {S}, uint16
 *
 * unet_postproc_softmax      one fused pass: "softmax", "create_mask" and "argmax" with a per-voxel online max and rescaled sum
 *   softmax      p_c = exp(x_c - m) / sum_k exp(x_k - m), m = max_c x_c, in fp32; label_prob = p_1..p_{C-1}.  As torch.softmax(dim=0):
 *                a NaN logit, a +inf logit or all logits -inf make every p of that voxel NaN
 *   create_mask  fg_prob = sum_{c>=1} exp(x_c - m) / sum_k exp(x_k - m)  (from the exponentials, not 1 - p_0)
 *   argmax       label = fg_prob > threshold ? 1 + argmax_{c>=1} p_c : 0; the first index wins a tie; NaN > threshold is false.
 *                argmax of p over c >= 1 is taken as argmax of x over c >= 1
 *   A NULL output is not written.  label and fg_prob need one read of the logits; label_prob reads the foreground planes again.
 *
 * unet_postproc_argmax_planes  "argmax" on the current state, for a chain where a command changed label_prob or fg_prob after the
 *   fused pass: label = fg_prob > threshold ? 1 + argmax_c label_prob_c : 0 over the n_planes planes (the first plane wins a tie;
 *   a NaN fg_prob gives 0).  All three pointers are required.
 *
 * unet_postproc_defragment   6-connected components (face neighbours) of the mask plane > threshold; a component is kept iff
 *   count >= size_ratio * largest count (in double).  In the mask voxels that are not kept:
 *     each == 0 ("defragment")       the mask is fg_prob (required); zeroes fg_prob, the n_planes planes of label_prob and label,
 *                                    whichever are not NULL
 *     each != 0 ("defragment_each")  every one of the n_planes planes of label_prob is its own mask and only that plane is zeroed;
 *                                    fg_prob and label are not read or written.  Planes are processed UNET_POSTPROC_CHUNK at a time,
 *                                    so the scratch does not grow with C beyond that
 *   The component roots are the components' smallest linear indices and the sizes integer counts: the result does not depend on
 *   the order the device runs in.
 *
 * unet_postproc_plane_op     in place on each of the n_planes planes of label_prob:
 *     UNET_PP_UPPER_THRESHOLD  x > param ? param : x          UNET_PP_LOWER_THRESHOLD  x < param ? param : x
 *     UNET_PP_MINUS            x - param                      UNET_PP_BINARIZE         x > param ? 1 : 0
 *     UNET_PP_NORMALIZE        x / max(plane) when max(plane) > 0 (NaN voxels are skipped by the max; param unused)
 *     UNET_PP_SMOOTH           the 3x3x3 binomial (1,2,1)^3/64, border voxels replicated, taps in (kz, ky, kx) order: the filter
 *                              the augmentation uses for tipl::filter::gaussian (param unused)
 *
 * Volumes are W x H x D (x fastest); defragment and the plane ops take fewer than 2^31 voxels, D <= 65535 and H <= 4 x 65535.
 * Any alignment works.  All calls run on the caller's stream; all scratch is the caller's (unet_postproc_scratch_bytes for out_c classes covers every call on that volume): calls on different streams with different
 * scratch may run concurrently.  Argument errors are found before any device call.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_POSTPROC_H
#define UNET_POSTPROC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    UNET_PP_UPPER_THRESHOLD = 1,
    UNET_PP_LOWER_THRESHOLD = 2,
    UNET_PP_MINUS = 3,
    UNET_PP_BINARIZE = 4,
    UNET_PP_NORMALIZE = 5,
    UNET_PP_SMOOTH = 6
};
#define UNET_POSTPROC_CHUNK 4   /* planes per round of defragment_each, normalize_each and smoothing */

int unet_postproc_scratch_bytes(int out_c, int64_t voxels, size_t* bytes);

int unet_postproc_softmax(const float* logits, int out_c, int64_t voxels, float threshold, float* label_prob, float* fg_prob,
                          uint16_t* label, void* stream);

int unet_postproc_argmax_planes(const float* label_prob, int n_planes, int64_t voxels, const float* fg_prob, float threshold,
                                uint16_t* label, void* stream);

int unet_postproc_defragment(int w, int h, int d, int each, float threshold, double size_ratio, float* fg_prob, float* label_prob,
                             int n_planes, uint16_t* label, void* scratch, size_t scratch_bytes, void* stream);

int unet_postproc_plane_op(int op, float param, int w, int h, int d, float* label_prob, int n_planes, void* scratch,
                           size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
