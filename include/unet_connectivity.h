/* C ABI of connected components with a chosen connectivity, exported by libunet_hip.so: the keep-largest call of
 * unet_components.h, the instance labelling of unet_instances.h and the hole filling of unet_morph.h, each with a `connectivity`
 * argument of 6, 18 or 26.  Those three headers stay as they are and keep their 6-connected definitions; with connectivity 6 every
 * call here writes exactly the bytes of its sibling there.
 *
 * The reference numbers no objects, and TIPL's evalution_set is not in the reference tree: these are this project's definitions
 * (parity NOT pinned).  Every value is a label, a bit or an integer count, so the device is pinned bit for bit to the restatements
 * of tests/test_connectivity_host.py, which are scipy.ndimage.label and binary_fill_holes with generate_binary_structure(3, 1 | 2 | 3).
 *
 * Neighbourhood  connectivity 6, 18 or 26 (UNET_CONN_6 / _18 / _26): the offsets (dx, dy, dz) in {-1, 0, 1}^3 with
 *            1 <= |dx| + |dy| + |dz| <= 1, 2 or 3: face, face and edge, face and edge and corner neighbours.  Any other value is an
 *            argument error that names it.
 * Component  a maximal set of voxels that hold the same listed value and are joined by steps of the neighbourhood.  Two touching
 *            components of different classes never merge.  The kernels hook every member to the neighbours of the backward half
 *            N-(c) of the neighbourhood (the 3, 9 or 13 offsets whose neighbour has the smaller linear index) inside the grid.
 * Grid       W x H x D, x fastest, S = W*H*D voxels, fewer than 2^31.
 *
 * unet_conn_keep_largest
 *   Input      a label map {S} uint16, changed in place; n_classes; a list of classes.
 *   Listed     a class v is listed when it appears in the list.  An entry that is 0 or >= n_classes is an argument error (the
 *              message names the entry).  Duplicates are allowed.
 *   Component  as above.  Voxels of an unlisted value (0 and values >= n_classes among them) never join anything and are never
 *              written.
 *   Kept       for each listed class the component with the largest voxel count; among equal counts the component that contains
 *              the smallest linear index.  Every other voxel of that class becomes 0.
 *   removed    optional device uint32[n_classes]: removed[v] = the number of voxels of class v set to zero, 0 for unlisted classes.
 *   listed is HOST memory and is consumed before the call returns.  n_listed == 0 leaves the label map untouched; removed is still
 *   zero-filled when it is given.  1 <= n_classes <= 65536.  Any alignment of label and of scratch works.
 *   scratch    device, unet_conn_scratch_bytes(voxels, n_classes, &bytes).
 *
 * unet_conn_label
 *   label    a uint16 map, read only, any alignment.  Members and the list as above; an empty list makes nothing a member.
 *   inst     device int32[S], 4-byte aligned, filled completely: 0 for a voxel that is no member, else the id 1..N of its component.
 *            Ids are dense and increase with the smallest linear index of the component, over all listed classes together (the
 *            order scipy.ndimage.label numbers one binary mask in, with every structure).
 *   info     device int64[2], 8-byte aligned: [0] N, the true number of instances, also when it exceeds max_instances;
 *            [1] min(N, max_instances), the rows that hold an instance.
 *   rows     device int64[(max_instances + 1) * 12], 8-byte aligned, filled completely and never written outside.  Row k:
 *                [0] the class   [1] the voxels   [2] the sum of x  [3] of y  [4] of z   [5] min x  [6] min y  [7] min z
 *                [8] max x  [9] max y  [10] max z   [11] the smallest linear index
 *            Row 0 and every row above N are the empty row: 0, 0, 0, 0, 0, (w, h, d), -1, -1, -1, -1.  An instance whose id exceeds
 *            max_instances has no row; inst still holds its id.  0 <= max_instances <= 2147483646.
 *   scratch  device, unet_conn_label_scratch_bytes(voxels, n_classes, max_instances, &bytes), any alignment.
 *
 * unet_conn_holes
 *   in, out  bit-packed masks as in unet_morph.h: uint64[D][H][ceil(W / 64)], 8-byte aligned, voxel x of a line in bit (x & 63) of
 *            word (x >> 6); out has the bits at and above W zero; out may be in.
 *   Holes    connectivity is the BACKGROUND's: a hole is a c-connected component of the complement (the voxels of the grid whose
 *            bit is 0) that holds no voxel on a face of the volume; out = in OR every hole:
 *            scipy.ndimage.binary_fill_holes(m, structure=generate_binary_structure(3, 1 | 2 | 3)).  6 is the older header's
 *            definition, under which a shell that leaks through a diagonal alone counts as closed; 26 is the strict one: a
 *            cavity is filled only when no face, edge or corner step leads out of it.
 *   info     optional device int64[2], 8-byte aligned: [0] the voxels filled, [1] the holes.
 *   scratch  device, unet_conn_holes_scratch_bytes(w, h, d, &bytes), any alignment.
 *
 * impl       UNET_CONN_IMPL_TILED    a block builds the union-find of its 32 x 8 x 8 tile in LDS; a second kernel hooks the tiles
 *                                    together: with 18 and 26 a backward neighbour can lie across a high x or y face and across two
 *                                    or three faces at once, so the voxels on both sides of every interior x and y face and on the
 *                                    low side of every interior z face hook every pair that leaves their tile
 *            UNET_CONN_IMPL_GLOBAL   every voxel hooks to its backward neighbours in global memory: the baseline and the second
 *                                    witness of the bits (for unet_conn_label also the table gathered in global memory only)
 *            UNET_CONN_IMPL_DEFAULT  TILED for all three connectivities
 *
 * The result of every call is a pure function of its input: the same bits on every run and from both implementations.  No call
 * synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on different
 * streams with different scratch may run concurrently.  No loop of any kernel waits for another thread; every atomic is an integer
 * compare-and-swap, add or maximum.  Argument errors (a null pointer, a misaligned output, a bad size, a grid of 2^31 voxels or
 * more, a scratch that is too small, an unknown impl or connectivity, a bad list entry) are found before any device call, with a
 * message that carries the function's name.
 *
 * Out of scope: the defragment command of the post-processing chain, which keeps its own 6-connected scheme; a connectivity for
 * the surface definition of unet_distance.h; the C++ host.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_CONNECTIVITY_H
#define UNET_CONNECTIVITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_CONN_IMPL_DEFAULT = 0, UNET_CONN_IMPL_TILED = 1, UNET_CONN_IMPL_GLOBAL = 2 };

#define UNET_CONN_6 6
#define UNET_CONN_18 18
#define UNET_CONN_26 26

int unet_conn_scratch_bytes(int64_t voxels, int n_classes, size_t* bytes);

int unet_conn_keep_largest(int w, int h, int d, uint16_t* label, int n_classes, const uint32_t* listed /* host */, int n_listed,
                           uint32_t* removed /* device, n_classes entries, or NULL */, int connectivity, int impl, void* scratch,
                           size_t scratch_bytes, void* stream);

int unet_conn_label_scratch_bytes(int64_t voxels, int n_classes, int64_t max_instances, size_t* bytes);

int unet_conn_label(int w, int h, int d, const uint16_t* label, int n_classes, const uint32_t* listed /* host */, int n_listed,
                    int32_t* inst, int64_t* rows, int64_t max_instances, int64_t* info, int connectivity, int impl, void* scratch,
                    size_t scratch_bytes, void* stream);

int unet_conn_holes_scratch_bytes(int w, int h, int d, size_t* bytes);

int unet_conn_holes(int w, int h, int d, const uint64_t* in, uint64_t* out, int64_t* info /* or NULL */, int connectivity, int impl,
                    void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
