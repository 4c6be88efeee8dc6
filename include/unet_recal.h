/* C ABI of the recalibration pass, exported by libunet_hip.so: temperature scaling of a segmentation's level-0 logits.  The negative
 * log-likelihood of a validation set under softmax(beta * x) is a convex function of the one number beta = 1 / T.  One fused pass
 * over the level-0 logits of a volume, the truth label and an optional mask evaluates that function and its slope for up to
 * UNET_RECAL_MAX_BETAS candidates at once, as integer sums; the host brackets the minimiser from them (recal.py) and folds it into
 * the level-0 head's weight and bias, so that a recalibrated model is an ordinary model.
 *
 * The reference has no counterpart.  The classification, the terms and their quantisation below are therefore this project's
 * definitions: parity with TIPL is NOT pinned.  Only integers are summed, so a result does not depend on the order
 * of the sum or on the schedule: the device is pinned to itself bit for bit across load widths, candidate counts and splits of a
 * volume, and to an fp64 numpy restatement within an a-priori round-off bound (tests/test_recal_host.py).
 *
 * logits     {C, S} fp32 planes, plane c at logits + c*S (the offset is 64-bit), 4-byte aligned, 2 <= C <= UNET_RECAL_MAX_CLASSES,
 *            1 <= S < 2^31.
 * label      {S} fp32, 4-byte aligned.  mask: {S} uint8 or NULL, any alignment.  Both are read as unet_calib.h reads them.
 * betas      host, n_betas values, 1 <= n_betas <= UNET_RECAL_MAX_BETAS, each finite and > 0; read before the return and passed to
 *            the device by value.
 *
 * Per voxel v, in this order:
 *   1. mask != NULL and mask[v] == 0: counted in `skipped`.
 *   2. l = label[v] is valid iff l > -1.0f && l < (float)C (a NaN is not); t = (int)l, truncating toward zero.  Otherwise the voxel
 *      is counted in `invalid_label`.
 *   3. a NaN logit, a +inf logit, or all channels -inf: counted in `bad`.
 *   4. x_t == -inf: counted in `impossible` (its likelihood is 0 at every beta).
 *   5. otherwise it is counted in `valid`, with, in fp32 and without contraction into fused multiply-adds,
 *        M = max_c x_c, d_c = x_c - M, dt = d_t
 *        per candidate beta, over ascending c:  e_c = expf(beta * d_c) (0 for d_c == -inf),  s = sum e_c,
 *                                               a = sum e_c * d_c over the c with d_c != -inf
 *        nll = logf(s) - beta * dt
 *        g   = a / s - dt                        d nll / d beta, formed without the cancellation of sum p_c x_c - x_t
 *      beta > 0, so one max serves every candidate, every e_c <= 1 and s >= 1.
 *      A term u (nll or g) is clamped when fabsf(u) > UNET_RECAL_CLAMP, to +-UNET_RECAL_CLAMP, and added as
 *      q = llrintf(u * 2^UNET_RECAL_SCALE_BITS): the product is exact, |q| <= 2^32, and S < 2^31 keeps every sum inside int64.  A
 *      voxel for which any term of any candidate was clamped is counted once in `saturated` (and stays in `valid`).
 *
 * tables     device int64[UNET_RECAL_TABLE_LEN], 8-byte aligned: filled completely when accumulate == 0 (a caller may pass garbage),
 *            added to when accumulate != 0 (a set of cases accumulates without a host readback).
 *              head[6]          valid, bad, invalid_label, skipped, impossible, saturated
 *              (nll_k, g_k)     for k = 0..7: the sums of q over the valid voxels; the candidates from n_betas on read 0
 * scratch    device, from unet_recal_scratch_bytes(C, S, &bytes): the running table lives there, nothing per voxel.  Any alignment.
 *
 * A thread takes units of UNET_RECAL_UNIT consecutive voxels, a block has UNET_RECAL_BLOCK_UNITS threads, the capped grid takes
 * UNET_RECAL_GRID_UNITS units per stride.  16-byte loads are used when S % 4 == 0 and logits and label are 16-byte aligned, scalar
 * ones otherwise; up to UNET_RECAL_CACHE channels of a unit stay in registers between the max sweep and the sum sweep, beyond that
 * they are read again.  A thread keeps its sums in registers; they reduce across the wave, across the block through LDS, and the
 * block sends one 64-bit integer add per table entry.  The bits are the same in every case.
 *
 * The call runs on the caller's stream and does not synchronise with the host.  Argument errors (a null logits, label, betas,
 * tables, scratch or bytes; out_c, voxels or n_betas out of range; a beta that is not finite or not positive; a misaligned logits,
 * label or tables; a scratch that is too small) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with the last-error call declared there).
 */
#ifndef UNET_RECAL_H
#define UNET_RECAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_RECAL_MAX_CLASSES 256
#define UNET_RECAL_MAX_BETAS 8
#define UNET_RECAL_HEAD 6             /* valid, bad, invalid_label, skipped, impossible, saturated */
#define UNET_RECAL_TABLE_LEN 22       /* head[6], then (nll_k, g_k) for k = 0..7 */
#define UNET_RECAL_SCALE_BITS 20      /* a term is added as llrintf(term * 2^20) */
#define UNET_RECAL_CLAMP 4096         /* a term beyond +-4096 is clamped to it */
#define UNET_RECAL_CACHE 8            /* channels of a unit that stay in registers between the two sweeps */
#define UNET_RECAL_UNIT 4             /* consecutive voxels a thread takes at once: one 16-byte load per plane */
#define UNET_RECAL_BLOCK_UNITS 256    /* units a block takes at once: one per thread */
#define UNET_RECAL_GRID_UNITS 131072  /* units the capped grid (512 blocks) takes per stride */

int unet_recal_scratch_bytes(int out_c, int64_t voxels, size_t* bytes);

int unet_recal_eval(const float* logits, int out_c, int64_t voxels, const float* label, const uint8_t* mask, const float* betas, int n_betas,
                    int accumulate, int64_t* tables, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
