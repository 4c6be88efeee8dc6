/* C ABI of a model's single_component_label (unet.hpp:23; handed to every evaluation set before the forward, evaluate.cpp:199),
 * exported by libunet_hip.so: every listed class of a label map keeps its largest 6-connected component.
 *
 * The definition is this project's: TIPL's evalution_set is not in the reference tree, so parity with TIPL is NOT pinned (as for
 * the augmentation, the post-processing chain, the resampling and the pre-processing chain).
 *
 * Input      a label map {S} uint16 on a W x H x D grid (x fastest, S = W*H*D), changed in place; n_classes; a list of classes.
 * Listed     a class v is listed when it appears in the list.  An entry that is 0 or >= n_classes is an argument error (the message
 *            names the entry).  Duplicates are allowed.
 * Component  a maximal 6-connected set of voxels (face neighbours) that hold the same listed value.  Voxels of an unlisted value
 *            (0 and values >= n_classes among them) never join anything and are never written.
 * Kept       for each listed class the component with the largest voxel count; among equal counts the component that contains the
 *            smallest linear index.  Every other voxel of that class becomes 0.
 * removed    optional device uint32[n_classes]: removed[v] = the number of voxels of class v set to zero, 0 for unlisted classes
 *            (the per-region "erased" report of reclassify_labels_by_template, evaluate.cpp:96-108, on the device).
 * The result is a pure function of the input: the same bits on every run and from both implementations.
 *
 * impl       UNET_COMPONENTS_IMPL_TILED   a block builds the union-find of its TX x TY x TZ tile in LDS, a second kernel hooks the
 *                                         tiles together across their low faces
 *            UNET_COMPONENTS_IMPL_GLOBAL  every voxel hooks to its neighbours in global memory (the defragment command's scheme
 *                                         with equal values in place of a mask): the measured baseline and a second witness
 *            UNET_COMPONENTS_IMPL_DEFAULT the faster of the two on solid label maps as measured: TILED
 *
 * listed is HOST memory and is consumed before the call returns.  The call makes no host synchronisation: everything is ordered on
 * the caller's stream.  All scratch is the caller's (unet_components_scratch_bytes): calls on different streams with different
 * scratch may run concurrently.  n_listed == 0 leaves the label map untouched; removed is still zero-filled when it is given.
 * Limits: fewer than 2^31 voxels, 1 <= n_classes <= 65536.  Any alignment of label works.  Argument errors (a null pointer, a bad
 * size, a scratch that is too small, an unknown impl, a bad list entry) are found before any device call.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_COMPONENTS_H
#define UNET_COMPONENTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_COMPONENTS_IMPL_DEFAULT = 0, UNET_COMPONENTS_IMPL_TILED = 1, UNET_COMPONENTS_IMPL_GLOBAL = 2 };

/* the tile of UNET_COMPONENTS_IMPL_TILED */
#define UNET_COMPONENTS_TILE_X 32
#define UNET_COMPONENTS_TILE_Y 8
#define UNET_COMPONENTS_TILE_Z 8

int unet_components_scratch_bytes(int64_t voxels, int n_classes, size_t* bytes);

int unet_components_keep_largest(int w, int h, int d, uint16_t* label, int n_classes, const uint32_t* listed /* host */, int n_listed,
                                 uint32_t* removed /* device, n_classes entries, or NULL */, int impl, void* scratch,
                                 size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
