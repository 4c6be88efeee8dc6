/* C ABI of the tables of a label map, exported by libunet_hip.so: what a parcellation is consumed as.  One pass over a region map
 * gives, per label, its size, where it is and its bounding box; one pass over two label maps gives what a Dice coefficient per label
 * needs.  The reference loads a template and an atlas (evaluate.cpp:488-496) and stops before using them, so nothing there
 * tabulates a label map: these are this project's definitions (parity NOT pinned).  Every column is an
 * integer count or an integer extreme, so the device is pinned to a numpy restatement bit for bit (tests/test_table_host.py).
 *
 * Maps       uint8 or uint16 (label_bytes, a_bytes, b_bytes: 1 or 2), x fastest, fewer than 2^31 voxels, read only, any alignment.
 * Labels     L = n_labels, 1 <= L <= 65535.  A value above L reads as 0.  L may exceed what a uint8 map can hold.
 * Rows       L + 1 of them, row 0 the background, tabulated like any other row.
 *
 * unet_table_regions -- PINNED (integer adds, minima and maxima only)
 *   labels   w x h x d.
 *   rows     device int64[(L + 1) * 10], 8-byte aligned, filled completely (a caller may pass garbage).  Row l, over the voxels
 *            (x, y, z) that read l:
 *                [0] their number   [1] the sum of x   [2] of y   [3] of z   [4] min x  [5] min y  [6] min z   [7] max x  [8] max y  [9] max z
 *            An empty row: number 0, sums 0, minima (w, h, d), maxima -1.  The sums are exact: the sum of x of one label
 *            filling 6 x 70000 voxels passes 2^32.
 *
 * unet_table_overlap -- PINNED (integer adds only)
 *   a, b     two maps of `voxels` elements each, uint8 or uint16 independently of each other.
 *   rows     device int64[(L + 1) * 3], 8-byte aligned, filled completely.  Row l:
 *                [0] the voxels where a reads l   [1] those where b reads l   [2] those where both read l
 *
 * impl       UNET_TABLE_IMPL_LDS      a block gathers the rows below UNET_TABLE_LDS_ROWS in its LDS table and flushes one global
 *                                     update per touched row; a row at or above it is updated in global memory directly (atlas
 *                                     ids are sparse: FreeSurfer's run to 2035)
 *            UNET_TABLE_IMPL_GLOBAL   global atomics only: the measured baseline and the second witness of the bits
 *            UNET_TABLE_IMPL_DEFAULT  the faster of the two as measured
 *            In both a thread takes a unit of consecutive voxels along x and merges equal consecutive labels into one update per
 *            run: number += n, the sum of x += the run's arithmetic series, the sums of y and z += n * y and n * z, the extremes
 *            from the run's two ends.  A thread's units lie a few rows apart and its last run stays open from one to the next,
 *            so in a solid map it sends far fewer updates than it takes units.
 * scratch    device, from unet_table_scratch_bytes(voxels, n_labels, &bytes): one size serves both calls.  The running table
 *            lives there (64-bit sums, 32-bit extremes); a last launch widens it into rows.  Any alignment.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and the scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Argument errors (a null pointer, label_bytes / a_bytes / b_bytes
 * other than 1 or 2, n_labels or a dimension out of range, a grid of 2^31 voxels or more, misaligned rows, a scratch that is too
 * small, an unknown impl) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_TABLE_H
#define UNET_TABLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_TABLE_IMPL_DEFAULT = 0, UNET_TABLE_IMPL_LDS = 1, UNET_TABLE_IMPL_GLOBAL = 2 };

#define UNET_TABLE_MAX_LABELS 65535
#define UNET_TABLE_LDS_ROWS 1024   /* x 56 bytes (four 64-bit sums, six 32-bit extremes) = 56 KiB of a block's LDS */
#define UNET_TABLE_REGION_COLUMNS 10
#define UNET_TABLE_OVERLAP_COLUMNS 3

int unet_table_scratch_bytes(int64_t voxels, int n_labels, size_t* bytes);

int unet_table_regions(const void* labels, int label_bytes, int w, int h, int d, int n_labels, int64_t* rows, int impl, void* scratch,
                       size_t scratch_bytes, void* stream);

int unet_table_overlap(const void* a, int a_bytes, const void* b, int b_bytes, int64_t voxels, int n_labels, int64_t* rows, int impl,
                       void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
