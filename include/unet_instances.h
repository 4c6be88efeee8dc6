/* C ABI of the instances of a label map, exported by libunet_hip.so: a class seen as a set of objects.  One call numbers every
 * 6-connected component of the listed classes and tabulates it; one call counts the overlap of every pair of instances of two such
 * maps; one call removes the instances below a size.  Lesion-wise detection scores (how many found, how many invented) are host
 * arithmetic on those tables (unet-studio_amd/instances.py).
 *
 * The reference stops at voxel counts (evaluate.cpp, qc.cpp): nothing there numbers or matches objects.  These are this project's
 * definitions (parity NOT pinned, as for the tables of a label map and the boundary distances).  Every value is
 * an integer count, sum, extreme or index, so the device is pinned to the numpy restatements of tests/test_instances_host.py bit for
 * bit, whatever the schedule and whichever implementation.
 *
 * unet_inst_label -- PINNED
 *   label    a uint16 map on a W x H x D grid (x fastest, S = W*H*D voxels, fewer than 2^31), read only, any alignment.
 *   Members  exactly as in unet_components.h: a class is listed when it appears in the list (host memory, consumed before the call
 *            returns; an entry that is 0 or >= n_classes is an argument error naming it; duplicates are allowed); a component is a
 *            maximal 6-connected set of voxels holding the same listed value.  Two touching components of different classes never
 *            merge.  An empty list makes nothing a member.
 *   inst     device int32[S], 4-byte aligned, filled completely: 0 for a voxel that is no member, else the id 1..N of its component.
 *            Ids are dense and increase with the smallest linear index of the component, over all listed classes together (the
 *            order scipy.ndimage.label numbers one binary mask in).
 *   info     device int64[2], 8-byte aligned: [0] N, the true number of instances, also when it exceeds max_instances;
 *            [1] min(N, max_instances), the rows that hold an instance.
 *   rows     device int64[(max_instances + 1) * 12], 8-byte aligned, filled completely and never written outside.  Row k:
 *                [0] the class   [1] the voxels   [2] the sum of x  [3] of y  [4] of z   [5] min x  [6] min y  [7] min z
 *                [8] max x  [9] max y  [10] max z   [11] the smallest linear index
 *            Row 0 and every row above N are the empty row: 0, 0, 0, 0, 0, (w, h, d), -1, -1, -1, -1.  An instance whose id exceeds
 *            max_instances has no row; inst still holds its id.
 *   impl     UNET_INST_LABEL_TILED / _GLOBAL select the labelling stage single_component_label uses (a tile's union-find in LDS and
 *            hooks across the tile faces / every voxel hooked in global memory, and with it the table gathered in global memory
 *            only: the second witness of the bits); UNET_INST_LABEL_DEFAULT is the faster as measured.  The dense
 *            numbering is an exclusive scan of "is a root" in three launches (sums per block, a scan of the sums, the
 *            assignment): no block ever waits for another.
 *   scratch  device, unet_inst_scratch_bytes(voxels, n_classes, max_instances, &bytes), any alignment.
 *
 * unet_inst_match -- PINNED after a sort
 *   ia, ib   two instance maps, device int32[voxels], 4-byte aligned, read only.  A voxel with ia > 0 and ib > 0 belongs to the pair
 *            (ia << 32) | ib; every other voxel to none.
 *   keys     device uint64[max_pairs], counts device int64[max_pairs], 8-byte aligned: every distinct pair once with its number of
 *            voxels, in no particular order.  Entries at and above info[0] are not written.
 *   info     device int64[2]: [0] the pairs written; [1] non-zero exactly when the distinct pairs exceed max_pairs.  Then what keys
 *            and counts hold is unspecified, nothing outside them is written and the call ends normally: call again with more.
 *   impl     UNET_INST_IMPL_GLOBAL  every run of equal consecutive pairs goes to the open-addressing table in the scratch: an
 *                                   empty slot is claimed by compare-and-swap, the count is an integer add, probing is bounded by
 *                                   the number of slots and then raises the flag.  The measured baseline and the second witness
 *            UNET_INST_IMPL_LDS     a block first gathers its runs in an LDS table of UNET_INST_LDS_SLOTS slots and flushes one
 *                                   update per touched pair; a run that finds no slot there goes to the global table directly
 *            UNET_INST_IMPL_DEFAULT the faster of the two as measured
 *   scratch  device, unet_inst_match_scratch_bytes(max_pairs, &bytes), any alignment.
 *
 * unet_inst_remove_small
 *   label    device uint16[voxels], changed in place; inst and rows as unet_inst_label left them for it.  A voxel with
 *            1 <= inst <= max_instances whose row counts fewer than min_voxels voxels becomes 0.  An id above max_instances has no
 *            row and is left alone.  removed: optional device uint32[n_classes], zero-filled first, removed[c] = the voxels of class
 *            c set to zero (n_classes is read only with it; a value >= n_classes is zeroed and not counted).
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  No loop of any kernel waits for another thread.  Argument errors
 * (a null pointer, a misaligned output, a size out of range, a grid of 2^31 voxels or more, a scratch that is too small, an unknown
 * impl, a bad list entry) are found before any device call, with a message naming the argument.
 *
 * Out of scope: 18- and 26-connectivity here (unet_connectivity.h has the labelling call with a connectivity argument); an optimal
 * one-to-one assignment between instances.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_INSTANCES_H
#define UNET_INSTANCES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_INST_LABEL_DEFAULT = 0, UNET_INST_LABEL_TILED = 1, UNET_INST_LABEL_GLOBAL = 2 };
enum { UNET_INST_IMPL_DEFAULT = 0, UNET_INST_IMPL_LDS = 1, UNET_INST_IMPL_GLOBAL = 2 };

#define UNET_INST_COLUMNS 12
#define UNET_INST_LDS_ROWS 1024    /* ids below it are tabulated in a block's LDS: x 48 bytes (three 64-bit sums, six 32-bit extremes) */
#define UNET_INST_LDS_SLOTS 2048   /* the slots of a block's LDS pair table: x 12 bytes (a 64-bit key, a 32-bit count) */
#define UNET_INST_MAX_INSTANCES 2147483646
#define UNET_INST_MAX_PAIRS 1073741824

int unet_inst_scratch_bytes(int64_t voxels, int n_classes, int64_t max_instances, size_t* bytes);

int unet_inst_label(int w, int h, int d, const uint16_t* label, int n_classes, const uint32_t* listed /* host */, int n_listed,
                    int32_t* inst, int64_t* rows, int64_t max_instances, int64_t* info, int impl, void* scratch, size_t scratch_bytes,
                    void* stream);

int unet_inst_match_scratch_bytes(int64_t max_pairs, size_t* bytes);

int unet_inst_match(const int32_t* ia, const int32_t* ib, int64_t voxels, uint64_t* keys, int64_t* counts, int64_t max_pairs,
                    int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_inst_remove_small(uint16_t* label, const int32_t* inst, int64_t voxels, const int64_t* rows, int64_t max_instances,
                           int64_t min_voxels, uint32_t* removed /* device, n_classes entries, or NULL */, int n_classes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
