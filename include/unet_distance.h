/* C ABI of the boundary distances of label maps, exported by libunet_hip.so: an exact Euclidean distance transform on the device and
 * what Hausdorff distance, its 95th percentile and average symmetric surface distance per label need from it.  The reference
 * (evaluate.cpp, qc.cpp) measures no boundary distance, so these are this project's definitions (parity NOT pinned, as in DESIGN.md
 * §18, §20 and §21).  Everything the device decides is an integer, so it is pinned to a numpy restatement bit for bit, with scipy's
 * distance_transform_edt as an independent second witness (tests/test_distance_host.py).
 *
 * Maps       uint8 or uint16 (label_bytes, a_bytes, b_bytes, at_bytes: 1 or 2), w x h x d, x fastest, fewer than 2^31 voxels, read
 *            only, any alignment.  With n_labels given, a value above it reads as 0.
 * Metric     three positive integer weights (wx, wy, wz).  The squared distance between two voxels is wx dx^2 + wy dy^2 + wz dz^2,
 *            an int32.  A call is refused unless wx (w-1)^2 + wy (h-1)^2 + wz (d-1)^2 < 2^31 - 1 = UNET_DIST_INF, so no distance
 *            inside the grid reaches UNET_DIST_INF, which means "the feature set is empty".  No kernel forms a sum that can wrap:
 *            an INF entry is skipped, never added to.  (How a voxel size in mm becomes weights is the caller's: distance.py:metric.)
 * Surface    S(m, l): the voxels of m that read l and have a 6-neighbour that does not read l, or lie on a face of the volume
 *            (mask & ~binary_erosion(mask, 6-connected structure, border_value=0)).
 *
 * unet_dist_transform -- PINNED (integer multiplies, adds and minima only)
 *   label    in [1, 65535].
 *   of       UNET_DIST_OF_SURFACE: the feature set is S(labels, label); UNET_DIST_OF_LABEL: every voxel that reads label.
 *   out      device int32[w * h * d], 4-byte aligned, filled completely: per voxel the least squared distance to a feature voxel,
 *            0 at a feature voxel, UNET_DIST_INF everywhere when the feature set is empty.
 *   Three passes.  x: the feature predicate from the label map and wx * (distance along x to the nearest feature of the line)^2,
 *   or INF.  y, then z: out[p] = min_i (w (p - i)^2 + g[i]) along the line, by a search outward from p that stops when
 *   w delta^2 >= the best value so far or both ends of the line are passed: exact, and at most one line long whatever the data.
 *   impl     UNET_DIST_IMPL_LDS      x: a block keeps its lines' feature flags as 64-bit masks in LDS and a thread finds the nearest
 *                                    set bit on either side by word scans; y, z: a block holds a slab of UNET_DIST_SLAB_MAX_X or
 *                                    fewer consecutive x by the whole line in LDS (a line longer than UNET_DIST_LDS_MAX_LINE takes
 *                                    the global pass)
 *            UNET_DIST_IMPL_GLOBAL   the same passes from global memory, one thread per voxel: the measured baseline and the second
 *                                    witness of the bits
 *            UNET_DIST_IMPL_DEFAULT  the faster of the two as measured
 *   scratch  device, from unet_dist_scratch_bytes(w, h, d, &bytes): one int32 per voxel between the passes.  Any alignment.
 *
 * unet_dist_surface_counts -- PINNED (integer adds only)
 *   rows     device int64[(n_labels + 1) * 2], 8-byte aligned, filled completely: row l = |S(a, l)|, |S(b, l)|; row 0 is the
 *            surface of what reads 0.  1 <= n_labels <= 65535.  A block gathers the rows below UNET_DIST_LDS_ROWS in its LDS table.
 *
 * unet_dist_gather -- PINNED as a multiset (the order within the list is unspecified: sort it)
 *   Appends dist[v] for every v in S(at, label): values[*cursor + k], the cursor advanced atomically by the number appended.  A slot
 *   at or past capacity is never written, and the cursor still counts it, so a caller can see an overflow.  cursor: device, 8-byte
 *   aligned, the caller's to zero.  dist, values: 4-byte aligned int32.  capacity >= 0.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Argument errors (a null pointer, bytes other than 1 or 2, a label
 * or n_labels out of [1, 65535], a non-positive dimension or weight, the metric bound, a grid of 2^31 voxels or more, a misaligned
 * pointer, a scratch that is too small, an unknown impl or of) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_DISTANCE_H
#define UNET_DISTANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_DIST_IMPL_DEFAULT = 0, UNET_DIST_IMPL_LDS = 1, UNET_DIST_IMPL_GLOBAL = 2 };
enum { UNET_DIST_OF_SURFACE = 0, UNET_DIST_OF_LABEL = 1 };

#define UNET_DIST_INF 2147483647
#define UNET_DIST_MAX_LABEL 65535
#define UNET_DIST_LDS_ROWS 1024       /* x two 32-bit counters = 8 KiB of a block's LDS */
#define UNET_DIST_SLAB_MAX_X 32       /* the widest slab of the y and z passes; halved down to 8 until line x slab x 4 B <= 64 KiB */
#define UNET_DIST_LDS_MAX_LINE 2048   /* 2048 x 8 x 4 B = 64 KiB */

int unet_dist_scratch_bytes(int w, int h, int d, size_t* bytes);

int unet_dist_transform(const void* labels, int label_bytes, int w, int h, int d, int label, int of, int wx, int wy, int wz, int32_t* out,
                        int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_dist_surface_counts(const void* a, int a_bytes, const void* b, int b_bytes, int w, int h, int d, int n_labels,
                             int64_t* rows /* {n_labels + 1, 2}: |S(a, l)|, |S(b, l)| */, void* stream);

int unet_dist_gather(const void* at, int at_bytes, int w, int h, int d, int label, const int32_t* dist, int32_t* values, int64_t capacity,
                     unsigned long long* cursor, void* stream);

#ifdef __cplusplus
}
#endif
#endif
