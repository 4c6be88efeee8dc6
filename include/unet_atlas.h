/* C ABI of the atlas preparation of evaluate_unet::load_atlas (evaluate.cpp:112-179) and reclassify_labels_by_template
 * (evaluate.cpp:60-110), exported by libunet_hip.so: tissue votes, the per-region majority tissue, the erase pass, and the growth
 * of the regions back into the unlabelled voxels of a tissue.
 *
 * Grid       S = W*H*D voxels, x fastest.
 * tissue     the "template" image: uint8 or uint16 (tissue_bytes 1 or 2), read only.  Any tissue map, the uint16 label output of an
 *            evaluation among them (the reference's function is a template over this image, evaluate.cpp:60).
 * atlas      uint16, changed in place.
 * Counts     T = n_tissues, 1 <= T <= 256;  R = n_regions, 0 <= R <= 65535.
 * Flags      UNET_ATLAS_CLAMP     a tissue value >= T reads as 0 (load_template's replace_if(v >= 5, 0), evaluate.hpp:38, on the fly)
 *            UNET_ATLAS_PRESERVE  a voxel whose tissue reads 0 has its atlas value read as 0, and written as 0 by every call that
 *                                 writes the atlas (tipl::preserve, evaluate.cpp:134, on the fly)
 *            UNET_ATLAS_COUNT_ONLY (reclassify only) the atlas is not written; every report is that of a full call
 *            The flags apply in this order: tissue is read (CLAMP), then the atlas value is read (PRESERVE), then everything below.
 * Above R    an atlas value, as read, above R is never counted and never written by reclassify.
 *
 * unet_atlas_reclassify -- PINNED: evaluate.cpp:63-94 and :136-152 literally, integer adds only, so the same bits on every run and
 * from every implementation.
 *   tissue_total[t]  voxels whose tissue reads t, t < T                                        (tipl::histogram, :137)
 *   votes[a*T + t]   voxels with atlas a, 1 <= a <= R, and tissue t < T; row 0 is all zero     (:68-74)
 *   covered[t]       sum over a >= 1 of votes[a*T + t]                                         (:145-147)
 *   majority[a]      the FIRST index of the largest entry of row a (std::max_element: ties go to the smallest t, 0 included);
 *                    0 for a = 0 and for an empty row                                          (:76-83)
 *   erase            a voxel with 1 <= a <= R whose tissue, as read, differs from majority[a] becomes 0 and adds one to erased[a];
 *                    a tissue value >= T without CLAMP differs from every majority (:89 is an inequality)   (:86-94)
 *   Outputs, each optional (NULL), each a device array the call fills completely (no memset by the caller):
 *   votes uint32[(R+1)*T], tissue_total uint32[T], covered uint32[T], majority uint8[R+1], erased uint32[R+1].
 *   impl  UNET_ATLAS_IMPL_LDS      a block gathers the first UNET_ATLAS_LDS_ENTRIES entries of votes (whole rows only) and the T
 *                                  totals in LDS and flushes them with one global add per non-zero entry; the rows that do not fit
 *                                  go through global adds, so every R is legal.  The erase pass gathers erased[a] for
 *                                  a < UNET_ATLAS_LDS_ENTRIES the same way
 *         UNET_ATLAS_IMPL_GLOBAL   the same run merging with global adds only: the measured baseline, a second witness of the bits
 *         UNET_ATLAS_IMPL_DEFAULT  the faster of the two on a solid atlas as measured
 *
 * unet_atlas_grow -- this project's definition in place of tipl::morphology::fill_and_smooth_labels (evaluate.cpp:162-175; TIPL is
 * not in the reference tree, so parity is NOT pinned, as for the other evaluation stages).
 *   grow     HOST array of T flags, consumed before the call returns: the tissues to work on.
 *   active   a voxel whose tissue, as read, is t < T with grow[t] != 0 (and, under PRESERVE, t != 0).
 *   peers    the face neighbours inside the volume whose tissue reads the same value.
 *   Fill     synchronous rounds r = 1, 2, ...: every voxel reads the state before the round; an active voxel with label 0 and at
 *            least one peer with a non-zero label takes the most frequent non-zero label among its peers, the smallest among equal
 *            counts.  The fill ends after the first round that fills nothing (converged = 1) or after max_rounds rounds
 *            (0 <= max_rounds <= 65534, converged = 0): the state is then exactly that after max_rounds rounds.
 *   Smooth   smooth_rounds (0..16) further synchronous rounds: an active voxel with label L != 0 counts the labels of itself and of
 *            its peers with non-zero labels; M is the most frequent, the smallest among equal counts; it takes M when
 *            count(M) > count(L).  Label-0 voxels are untouched.
 *   Peers share a tissue, so several flagged tissues in one call equal one call per tissue (the reference's loop, :166-174).
 *   Reports, each optional, device arrays filled completely: filled uint32[T] (voxels the fill labelled, per tissue), relabelled
 *   uint32[T] (label changes summed over the smoothing rounds, per tissue), info uint32[2] = {fill rounds that filled something,
 *   converged}.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's
 * (unet_atlas_scratch_bytes; one size serves both calls, max_rounds = 0 for a caller that only reclassifies), so calls on different
 * streams with different scratch may run concurrently.  Any alignment of tissue works; atlas needs its type's 2 bytes.  Fewer than
 * 2^31 voxels.  Argument errors (a null pointer, a bad size, tissue_bytes other than 1 or 2, T or R out of range, max_rounds or
 * smooth_rounds out of range, a scratch that is too small, an unknown impl or flag) are found before any device call.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_ATLAS_H
#define UNET_ATLAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_ATLAS_IMPL_DEFAULT = 0, UNET_ATLAS_IMPL_LDS = 1, UNET_ATLAS_IMPL_GLOBAL = 2 };
enum { UNET_ATLAS_CLAMP = 1, UNET_ATLAS_PRESERVE = 2, UNET_ATLAS_COUNT_ONLY = 4 };

/* the votes entries (and erased entries) a block of UNET_ATLAS_IMPL_LDS keeps in LDS */
#define UNET_ATLAS_LDS_ENTRIES 8192

int unet_atlas_scratch_bytes(int64_t voxels, int n_regions, int n_tissues, int max_rounds, size_t* bytes);

/* evaluate.cpp:63-94 (votes, majority, erase), :134 (PRESERVE), :136-152 (tissue_total, covered) */
int unet_atlas_reclassify(int64_t voxels, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_regions, int n_tissues, int flags,
                          uint32_t* votes, uint32_t* tissue_total, uint32_t* covered, uint8_t* majority, uint32_t* erased, int impl,
                          void* scratch, size_t scratch_bytes, void* stream);

/* evaluate.cpp:162-175 (the mask per tissue and fill_and_smooth_labels, by this project's definition) */
int unet_atlas_grow(int w, int h, int d, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_tissues, int flags,
                    const uint8_t* grow /* host, consumed before return */, int max_rounds, int smooth_rounds, uint32_t* filled,
                    uint32_t* relabelled, uint32_t* info, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
