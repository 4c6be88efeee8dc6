/* C ABI of test-time mirroring, exported by libunet_hip.so: a volume is run through the network under every combination of axis
 * flips, and the members' logits are flipped back, their lateralised channels swapped back, and averaged before softmax / argmax.
 *
 * The reference has no counterpart (its flips are the orientation's only).  The members, the swap, the combine and the agreement
 * below are therefore this project's definitions: parity with TIPL is NOT pinned.
 *
 * AXES     A, a subset of {x, y, z}, written as a string such as "x", "xz", "xyz" or "" (letters in any order; a repeated or unknown
 *   letter is an error; mirror.parse_axes, host only).
 * MEMBERS  all K = 2^|A| subsets of A, in ascending mask, bit 0 = x, bit 1 = y, bit 2 = z: member 0 is always the identity and K is
 *   1, 2, 4 or 8 ("xz": the masks 0, 1, 4, 5).  The ABI takes the explicit ascending list (n_members, masks) and refuses one that
 *   does not start at 0, does not strictly ascend, holds a mask above 7, or whose length is not 1, 2, 4 or 8.
 * FLIP_m   of the voxel (x, y, z) of a W x H x D grid: x -> W-1-x when bit 0 of m is set, likewise y (bit 1) and z (bit 2).
 * SWAP     optional: swap_axis in {-1 (none), 0, 1, 2} and up to UNET_MIRROR_MAX_PAIRS pairs (a, b) of channels, disjoint, a != b,
 *   both in [0, out_c).  A model with lateralised classes answers an image mirrored along that axis with the OTHER class of each
 *   pair, so such a member's channels are swapped back as well as its voxels.  sigma is the involution that swaps each pair;
 *   sigma_m = sigma when bit swap_axis of m is set, else the identity.  Pairs with swap_axis = -1, and a swap_axis that no member
 *   mirrors (not in the union of the masks' bits), are errors.
 * COMBINE  mean(c, v) = (sum_m stack[m][sigma_m(c)][FLIP_m(v)]) * (1.0f / K): the sum starts from member 0's value and goes over
 *   ascending m in fp32, every add rounded; 1/K is a power of two, so the scale is exact, and K = 1 copies member 0 bit for bit.
 *   NaN and +-inf follow that arithmetic.
 * AGREEMENT  per voxel a uint8 in 0..K: the number of members m with amax(stack[m][sigma_m(.)][FLIP_m(v)]) == amax(mean(., v)),
 *   where amax(x) is: best = 0; for c in 1..C-1: if x[c] > x[best]: best = c.  All channels take part, the background included; the
 *   first index wins a tie and a comparison with NaN is false.  It is defined on comparisons only (no exponentials), so it is the
 *   same bits on every run and in numpy: how many mirrored views voted for the ensemble's top class.  It says nothing about
 *   `label`, which also depends on the fg_prob threshold.
 *
 * stack      {K, out_c, d, h, w} fp32, contiguous, x fastest: member m's logits for the input flipped by FLIP_m; fewer than 2^31
 *            voxels per volume, 2 <= out_c <= 65536
 * mean       {out_c, d, h, w} fp32;  agreement {d, h, w} uint8
 * masks and pairs (2 * n_pairs ints, or NULL) are read from HOST memory at the call and travel in the launch arguments.
 *
 * unet_mirror_combine   one gather pass, the stack read once and the mean written once: 4 * out_c * (K + 1) * voxels bytes (+ 1 per
 *   voxel for the agreement).  mean or agreement may be NULL (not wanted), not both.
 * unet_mirror_postproc  the fused softmax / create_mask / argmax pass of include/unet_postproc.h (same definitions, same
 *   NULL-output rule, same NaN / inf rules), each logit it reads being the COMBINE of the stack, never stored.  label_prob, fg_prob
 *   and label equal unet_mirror_combine followed by that header's softmax pass bit for bit; agreement equals unet_mirror_combine's.
 *   At least one of the four outputs must be wanted.
 *
 * Any 4-byte pointer alignment works: 16-byte loads are used when w % 4 == 0 and every plane of the stack and of the outputs is
 * 16-byte aligned, scalar ones otherwise, with the same bits.  Argument errors (NULL stack, non-positive sizes, a volume of 2^31
 * voxels or more, out_c outside [2, 65536], a bad member list, a bad swap, no output wanted) are found before any device call.
 * Everything runs on the caller's stream and needs no scratch.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_MIRROR_H
#define UNET_MIRROR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_MIRROR_MAX_PAIRS 64    /* channel pairs of one swap */
#define UNET_MIRROR_MAX_MEMBERS 8   /* 2^3 axis subsets */

int unet_mirror_combine(const float* stack, int out_c, int w, int h, int d, int n_members, const int* masks, int swap_axis,
                        const int* pairs, int n_pairs, float* mean, uint8_t* agreement, void* stream);

int unet_mirror_postproc(const float* stack, int out_c, int w, int h, int d, int n_members, const int* masks, int swap_axis,
                         const int* pairs, int n_pairs, float threshold, float* label_prob, float* fg_prob, uint16_t* label,
                         uint8_t* agreement, void* stream);

#ifdef __cplusplus
}
#endif
#endif
