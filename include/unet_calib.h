/* C ABI of the calibration tables, exported by libunet_hip.so: whether the probabilities of a segmentation mean anything.  One fused
 * pass over the per-voxel probabilities of a volume (formed from level-0 logits on the fly, or read from the planes of an ensemble
 * state), the truth label and an optional mask fills one table of integer counts and sums, from which the host derives the
 * reliability diagram, ECE and MCE, the class-wise ECE, the Brier score and a rigorously bracketed negative log-likelihood; an
 * optional byte map marks every counted voxel correct or wrong, so that an uncertainty map can be histogrammed against it (the
 * per-region histogram of unet_stats.h takes it as a label map as it is).
 *
 * The reference has no counterpart.  The codes, bins, keys and tables below are therefore this project's definitions: parity with
 * TIPL is NOT pinned.  Everything the device does is a compare, a coding or an integer add, so the device is pinned to
 * a numpy restatement bit for bit (tests/test_calib_host.py).
 *
 * src        {C, S} fp32 planes, plane c at src + c*S (the offset is 64-bit), 4-byte aligned, 2 <= C <= UNET_CALIB_MAX_CLASSES,
 *            1 <= S < 2^31.
 *   UNET_CALIB_SRC_LOGITS  level-0 logits.  Per voxel the online softmax state m, s of the fused softmax pass of unet_postproc.h over
 *            ascending c, then d_c = x_c - m, e_c = expf(d_c), p_c = e_c / s: that pass's and the ensemble's own expressions, so p_c
 *            equals, bit for bit, planes 0..C-1 of an ensemble state (unet_ensemble.h) that one member of weight 1.0f wrote as the
 *            first from the same logits.  A bad voxel by that pass's rule (a NaN logit, a +inf logit, or all channels -inf) has no
 *            probabilities.
 *   UNET_CALIB_SRC_PROBS   the planes are probabilities already (the first C planes of an ensemble state qualify: its plane stride
 *            is S); p_c is read as is, and a voxel with any NaN p_c is bad.
 * label      {S} fp32, 4-byte aligned, as the QC counts of unet_qc.h read it.  mask: {S} uint8 or NULL, any alignment.
 *
 * Per voxel v, in this order:
 *   1. mask != NULL and mask[v] == 0: counted in `skipped`.
 *   2. l = label[v] is valid iff l > -1.0f && l < (float)C (a NaN is not); t = (int)l, truncating toward zero.  Otherwise the voxel
 *      is counted in `invalid_label`.
 *   3. a bad voxel is counted in `bad`.
 *   4. otherwise it is counted in `valid`, with
 *        code(p)  u = p * 65536.0f (exact), q = u < 0 ? 0 : (u >= 65535.0f ? 65535 : (int)u)
 *        bin(q)   (q * 20) >> 16: 20 bins (UNET_CALIB_BINS), which merge into 10, 5, 4, 2 or 1
 *        pred     argmax_c p_c over the p values (not the logits), ascending c from 0, the first index wins a tie
 *        conf     p_pred, qc = code(conf), correct = (pred == t)
 *        key(p)   p <= 0 ? 0 : (p >= 1 ? 4064 : float_bits(p) >> 18): sign, exponent and 5 mantissa bits, 32 log-spaced bins per
 *                 octave, 4065 of them (UNET_CALIB_LOG_BINS)
 *      Subnormal probabilities are unspecified (the tests use none).
 *
 * tables     device int64[unet_calib_table_len(C)], 8-byte aligned: filled completely when accumulate == 0 (a caller may pass
 *            garbage), added to when accumulate != 0 (a set of cases accumulates without a host readback).
 *              head[4]        valid, bad, invalid_label, skipped
 *              top[20][3]     at row bin(qc): n, correct, the sum of qc
 *              cls[C][20][5]  for every class c of every valid voxel, at row bin(code(p_c)): n, pos (t == c), the sum of q, the sum
 *                             of q over the positives, the sum of q * q (exact: 65535^2 * 2^31 < 2^63)
 *              logh[4065]     the valid voxels by key(p_t)
 * wrong      device uint8[S] or NULL (not written): 0 for a voxel that was not counted as valid, 1 for correct, 2 for wrong.
 *
 * impl       UNET_CALIB_IMPL_GLOBAL   every update is a global atomic: the baseline and the second witness of the bits
 *            UNET_CALIB_IMPL_LDS      a block gathers its updates in LDS and flushes one global update per touched entry.  Held:
 *                                     head, top, the cls rows of the classes below UNET_CALIB_LDS_CLASSES and the uppermost
 *                                     UNET_CALIB_LDS_LOG_BINS entries of logh (p_t >= 2^-32); the rest goes to global memory
 *            UNET_CALIB_IMPL_DEFAULT  the faster of the two as measured
 *            In both a thread takes units of UNET_CALIB_UNIT consecutive voxels and merges the consecutive voxels of a unit that
 *            send the same update into one: a saturated probability map is a handful of updates per unit, not one per voxel and
 *            class.  A block has UNET_CALIB_BLOCK_UNITS threads, the capped grid takes UNET_CALIB_GRID_UNITS units per stride.
 *            16-byte loads are used when S % 4 == 0 and src and label are 16-byte aligned, scalar ones otherwise; up to
 *            UNET_CALIB_CACHE channels of a unit stay in registers between the two sweeps, beyond that they are read again.  The
 *            bits are the same in every case.
 * scratch    device, from unet_calib_scratch_bytes(C, S, &bytes): the running table lives there, nothing per voxel.  Any alignment.
 *
 * The call runs on the caller's stream and does not synchronise with the host.  Argument errors (a null src, label, tables, scratch
 * or bytes; out_c or voxels out of range; an unknown src_kind or impl; a misaligned src, label or tables; a scratch that is too
 * small) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with the last-error call declared there).
 */
#ifndef UNET_CALIB_H
#define UNET_CALIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_CALIB_SRC_LOGITS = 0, UNET_CALIB_SRC_PROBS = 1 };
enum { UNET_CALIB_IMPL_DEFAULT = 0, UNET_CALIB_IMPL_LDS = 1, UNET_CALIB_IMPL_GLOBAL = 2 };

#define UNET_CALIB_MAX_CLASSES 256
#define UNET_CALIB_BINS 20
#define UNET_CALIB_LOG_BINS 4065
#define UNET_CALIB_CODES 65536
#define UNET_CALIB_LDS_CLASSES 16     /* x 20 rows x 5 columns x 8 bytes = 12.5 KiB of a block's LDS */
#define UNET_CALIB_LDS_LOG_BINS 1024  /* x 8 bytes = 8 KiB of a block's LDS */
#define UNET_CALIB_CACHE 8            /* channels of a unit that stay in registers between the two sweeps */
#define UNET_CALIB_UNIT 8             /* consecutive voxels a thread takes at once */
#define UNET_CALIB_BLOCK_UNITS 256    /* units a block takes at once: one per thread */
#define UNET_CALIB_GRID_UNITS 131072  /* units the capped grid (512 blocks) takes per stride */

int unet_calib_table_len(int out_c, size_t* count);

int unet_calib_scratch_bytes(int out_c, int64_t voxels, size_t* bytes);

int unet_calib_tables(const float* src, int src_kind, int out_c, int64_t voxels, const float* label, const uint8_t* mask, int accumulate,
                      int64_t* tables, uint8_t* wrong, int impl, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
