/* C ABI of the per-region intensity statistics, exported by libunet_hip.so: what is IN the regions of a parcellation.  One pass over a
 * label map and a scalar volume (the scan, a probability channel, a co-registered FA, T1 or SUV map) gives, per label, the counts, the
 * integer moments and the exact extremes of the volume; a second call gives a 256-bin histogram per label, a third any eight
 * quantiles per label (the median among them) by a two-level radix select: no sort, nothing stored per voxel.  Without a label map
 * the whole volume is one region: its exact range and its percentiles, what a robust normalisation or a display window starts from.
 * The reference has no counterpart: these are this project's definitions (parity NOT pinned, as for the tables of a label map in
 * unet_table.h).  Every result is an integer count, sum or extreme, so the device is pinned to a numpy restatement bit for bit
 * (tests/test_stats_host.py).
 *
 * labels     uint8 or uint16 (label_bytes 1 or 2), `voxels` elements, 1 <= voxels < 2^31, read only, any alignment.  L = n_labels.
 *            A value above L reads as 0.  Row 0 is tabulated like any other row.  L may exceed what a uint8 map can hold.
 *            labels == NULL means one region: n_labels must then be 0, there is the single row 0 and label_bytes is ignored.
 * image      float32, 4-byte aligned, `voxels` elements, read only.
 * lo, hi     finite, lo < hi, and scale = 65536.0f / (hi - lo) finite and positive: one fp32 subtraction and one fp32 division,
 *            done once on the host.
 * Rows       L + 1 of them.  L <= 65535 for the moments, L <= UNET_STATS_MAX_QUANTILE_LABELS for the histograms and the quantiles,
 *            whose scratch grows by 1 KiB per row and per quantile.
 *
 * The code of a voxel with value v
 *            A NaN has no code: it is counted in the `nan` column and nowhere else.  Otherwise t = (v - lo) * scale, one fp32
 *            subtraction and one fp32 multiplication, each rounded to nearest (never an FMA); q = 0 if t < 0, q = 65535 if
 *            t >= 65535.0f, otherwise q = (int)t.  +inf and -inf therefore clamp to a code.  v < lo counts in `below`, v > hi in
 *            `above` (plain float compares on v); v == hi has code 65535 and counts in neither.  Subnormal inputs and subnormal
 *            differences v - lo are unspecified (the tests use none).
 * The key of a voxel
 *            the order-preserving image of the float's bits b: b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), unsigned 32-bit, over the
 *            non-NaN voxels, in range or not: the exact float extremes come back (-0.0 sorts below +0.0).
 *
 * unet_stats_moments -- PINNED (integer adds, minima and maxima only)
 *   rows     device int64[(L + 1) * 10], 8-byte aligned, filled completely (a caller may pass garbage).  Row l, over the voxels that
 *            read l:
 *                [0] n, those that are not NaN   [1] the NaNs   [2] below   [3] above   [4] the sum of q   [5] the sum of q * q
 *                [6] min q   [7] max q   [8] min key   [9] max key
 *            The sum of q * q is exact: 65535^2 * 2^31 < 2^63.  An empty row: 0, its NaNs, 0, 0, 0, 0, 65536, -1, 0xFFFFFFFF, -1.
 *
 * unet_stats_hist -- PINNED (integer adds only)
 *   rows     device int64[(L + 1) * 256], 8-byte aligned, filled completely: the coded voxels of row l whose q >> 8 is the column.
 *
 * unet_stats_quantiles -- PINNED (integer adds only)
 *   permille host int[n_quantiles], 1 <= n_quantiles <= UNET_STATS_MAX_QUANTILES, each in [0, 1000], duplicates allowed; read
 *            before the return.
 *   out      device int32[(L + 1) * n_quantiles], 4-byte aligned, filled completely.  For row l with n coded voxels and entry p the
 *            rank is r = p * (n - 1) / 1000 in 64-bit integer arithmetic, and the result is the r-th smallest code of the row,
 *            0-based; -1 when n = 0.
 *            Pass A is the coarse histogram above; a small kernel finds per (row, quantile) the coarse bin that holds rank r and
 *            the rank left inside it; pass B reads both volumes again and counts q & 255 for the voxels whose q >> 8 is a chosen bin
 *            of their row; a last kernel picks the fine bin.  Five launches, nothing read back.
 *
 * impl       UNET_STATS_IMPL_GLOBAL   every update is a global atomic: the measured baseline and the second witness of the bits
 *            UNET_STATS_IMPL_LDS      a block gathers its updates in LDS and flushes one global update per touched entry.  Moments:
 *                                     the rows below UNET_STATS_LDS_ROWS are held, the others are updated in global memory.
 *                                     Histograms: a row costs 1 KiB, so a block keeps UNET_STATS_LDS_SLOTS slots of
 *                                     UNET_STATS_SLOT_BINS consecutive counters of one row behind a (row, bin) -> slot cache
 *                                     (open addressing, at most UNET_STATS_LDS_PROBES probes); an update that finds no slot
 *                                     goes to global memory
 *            UNET_STATS_IMPL_DEFAULT  the faster of the two as measured
 *            In both a thread takes units of UNET_STATS_UNIT consecutive voxels and merges consecutive voxels that send the same
 *            update into one: a constant region, a 0/1 mask or a saturated probability map is a handful of updates, not millions
 *            on one address.  A wave takes UNET_STATS_WAVE_UNITS consecutive units at a time, the capped grid
 *            UNET_STATS_GRID_UNITS units per stride.
 * scratch    device, from unet_stats_scratch_bytes(voxels, n_labels, n_quantiles, &bytes), n_quantiles 0 for the moments and the
 *            histograms: the running tables live there, nothing per voxel.  Any alignment.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and the scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Argument errors (a null pointer; labels == NULL with n_labels != 0
 * or the reverse; label_bytes other than 1 or 2; a misaligned image, rows or out; voxels or n_labels out of range for the call; lo or
 * hi not finite or not ordered, or a scale that is not finite; n_quantiles or a permille out of range; a scratch that is too small;
 * an unknown impl) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with the last-error call declared there).
 */
#ifndef UNET_STATS_H
#define UNET_STATS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_STATS_IMPL_DEFAULT = 0, UNET_STATS_IMPL_LDS = 1, UNET_STATS_IMPL_GLOBAL = 2 };

#define UNET_STATS_MAX_LABELS 65535
#define UNET_STATS_MAX_QUANTILE_LABELS 4095
#define UNET_STATS_MAX_QUANTILES 8
#define UNET_STATS_MOMENT_COLUMNS 10
#define UNET_STATS_HIST_BINS 256
#define UNET_STATS_CODES 65536
#define UNET_STATS_LDS_ROWS 1024   /* x 56 bytes (six 64-bit sums, two 32-bit keys) = 56 KiB of a block's LDS */
#define UNET_STATS_LDS_SLOTS 512   /* x 64 bytes (UNET_STATS_SLOT_BINS 32-bit counters) = 32 KiB of a block's LDS */
#define UNET_STATS_SLOT_BINS 16
#define UNET_STATS_LDS_PROBES 8
#define UNET_STATS_UNIT 8          /* consecutive voxels a thread takes at once */
#define UNET_STATS_WAVE_UNITS 512  /* consecutive units a wave takes at once: 8 per lane */
#define UNET_STATS_GRID_UNITS 2097152 /* units the capped grid (512 blocks of 8 waves) takes per stride */

int unet_stats_scratch_bytes(int64_t voxels, int n_labels, int n_quantiles, size_t* bytes);

int unet_stats_moments(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                       int64_t* rows, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_stats_hist(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                    int64_t* rows, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_stats_quantiles(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                         const int* permille, int n_quantiles, int32_t* out, int impl, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
