/* C ABI of binary morphology on bit-packed masks, exported by libunet_hip.so: a label map is turned into a mask of one bit a voxel,
 * the mask is dilated, eroded or has its holes filled, and the result is written back into the label map.  Opening and closing
 * are chains of those calls on the host (unet-studio_amd/morph.py).
 *
 * The reference leaves the repair of a mask to TIPL (defragment_smoothing, fill_and_smooth_labels), which is absent.  These are
 * this project's definitions (parity with TIPL is NOT pinned).  Every value is a bit or an integer count, so the device is pinned
 * to the numpy restatements of tests/test_morph_host.py bit for bit, whichever implementation, with scipy.ndimage as the second
 * witness of the restatements.
 *
 * Grid     W x H x D, x fastest, S = W*H*D voxels, fewer than 2^31.
 * Mask     uint64[D][H][WPL], WPL = ceil(W / 64), 8-byte aligned: voxel x of a line is bit (x & 63) of word (x >> 6).  Every call
 *          that writes a mask leaves the bits at and above W zero, whatever those bits of its input held.
 * Neighbourhood  connectivity 6, 18 or 26: the offsets (dx, dy, dz) in {-1, 0, 1}^3 with 1 <= |dx| + |dy| + |dz| <= 1, 2 or 3.
 *          Any other value is an argument error.
 * Dilate   one step: out = in OR every neighbour inside the grid; outside the grid reads 0.
 * Erode    one step: out = in AND every neighbour; a neighbour outside the grid reads border, 0 or 1.  border = 1 means that a
 *          face of the volume is not an edge of the object; border = 0 is scipy.ndimage's default.
 * Iterations  n steps one after the other, 0 <= n <= 255; n = 0 copies.  in and out must not be the same pointer.
 * Holes    a hole is a 6-connected component of the complement (the voxels of the grid whose bit is 0) that holds no voxel on a
 *          face of the volume; out = in OR every hole: scipy.ndimage.binary_fill_holes with its default structure.  The
 *          background is 6-connected only, so a shell that leaks through a diagonal alone counts as closed and is filled.
 *
 * unet_morph_pack    the bit is set where the label (uint8 or uint16: label_bytes 1 or 2, any alignment) is a listed class.  The
 *                    list follows the rules of unet_components.h: host memory, consumed before the call returns; an entry that is
 *                    0 or >= n_classes is an argument error naming it; duplicates are allowed; an empty list gives the empty
 *                    mask.  A label >= n_classes is no member.  A wave takes 64 consecutive x of a line and its ballot is the word.
 * unet_morph_unpack  mask: device uint8[S], 1 where the bit is set, else 0.
 * unet_morph_count   count: device int64[1], 8-byte aligned, the set bits below W of every line.
 * unet_morph_step    op UNET_MORPH_DILATE or UNET_MORPH_ERODE, iterations steps.  Erosion runs as the complement of a dilation
 *                    with the outside read as !border.
 *                      UNET_MORPH_IMPL_GLOBAL  one thread per output word: it reads the up to 9 rows x 3 words it needs from
 *                                              global memory and forms a row's x-neighbours as w | w << 1 | w >> 1 with the carry
 *                                              bits of the two adjacent words; one launch per iteration, through the scratch.
 *                                              The baseline and the second witness of the bits
 *                      UNET_MORPH_IMPL_LDS     a block loads a brick of UNET_MORPH_BRICK_XW words x UNET_MORPH_BRICK_Y x
 *                                              UNET_MORPH_BRICK_Z rows into LDS with a halo of k rows in y and z and one word in
 *                                              x, runs k <= UNET_MORPH_FUSE_MAX iterations there (the valid region shrinks by one
 *                                              per iteration) and writes the brick: ceil(n / FUSE_MAX) launches
 *                      UNET_MORPH_IMPL_DEFAULT the faster of the two as measured
 * unet_morph_holes   info: optional device int64[2], 8-byte aligned: [0] the voxels filled, [1] the holes.  The complement goes
 *                    through the exact union-find labelling of unet_components.h (impl LDS: its tiled labelling, GLOBAL: its
 *                    global one, DEFAULT: the faster as measured), one pass over the six faces marks the roots that touch one,
 *                    one pass ballots the voxels of the unmarked roots into the words: a fixed number of launches.  out may be in.
 * unet_morph_apply   labels: device uint16[S], 2-byte aligned, changed in place; value in [1, 65535].
 *                      UNET_MORPH_SET   a voxel whose bit is 1 and whose label is 0 becomes value
 *                      UNET_MORPH_KEEP  a voxel whose label is value and whose bit is 0 becomes 0
 *                    No other voxel is written.  changed: optional device int64[1], 8-byte aligned, the voxels written.
 * scratch  device, unet_morph_scratch_bytes(w, h, d, &bytes): one size serves every call, any alignment.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's.  No loop of
 * any kernel waits for another thread or block, and every loop has a bound known at launch.  Argument errors (a null pointer, a
 * misaligned mask, a bad size, a grid of 2^31 voxels or more, an unknown op / mode / impl / connectivity, iterations out of range,
 * in == out, a scratch that is too small, a bad list entry) are found before any device call, with a message naming the argument.
 *
 * Out of scope: grey-scale morphology; structuring elements other than the three; hole filling with an 18- or 26-connected
 * background here (unet_connectivity.h has the hole filling call with a connectivity argument); geodesic reconstruction.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_MORPH_H
#define UNET_MORPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_MORPH_IMPL_DEFAULT = 0, UNET_MORPH_IMPL_LDS = 1, UNET_MORPH_IMPL_GLOBAL = 2 };
enum { UNET_MORPH_DILATE = 0, UNET_MORPH_ERODE = 1 };
enum { UNET_MORPH_SET = 0, UNET_MORPH_KEEP = 1 };

#define UNET_MORPH_FUSE_MAX 4          /* iterations one launch of the LDS step runs on its brick */
#define UNET_MORPH_BRICK_XW 2          /* the brick a block of the LDS step writes: words along x, */
#define UNET_MORPH_BRICK_Y 16          /* rows along y */
#define UNET_MORPH_BRICK_Z 16          /* and along z; two copies with the halo: 2 x 4 x 24 x 24 x 8 bytes = 36 KiB of LDS */
#define UNET_MORPH_MAX_ITERATIONS 255

int unet_morph_scratch_bytes(int w, int h, int d, size_t* bytes);

int unet_morph_pack(int w, int h, int d, const void* labels, int label_bytes, int n_classes, const uint32_t* listed /* host */,
                    int n_listed, uint64_t* bits, void* scratch, size_t scratch_bytes, void* stream);

int unet_morph_unpack(int w, int h, int d, const uint64_t* bits, uint8_t* mask, void* stream);

int unet_morph_count(int w, int h, int d, const uint64_t* bits, int64_t* count, void* stream);

int unet_morph_step(int w, int h, int d, const uint64_t* in, uint64_t* out, int op, int connectivity, int iterations, int border,
                    int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_morph_holes(int w, int h, int d, const uint64_t* in, uint64_t* out, int64_t* info /* or NULL */, int impl, void* scratch,
                     size_t scratch_bytes, void* stream);

int unet_morph_apply(int w, int h, int d, uint16_t* labels, const uint64_t* bits, int value, int mode,
                     int64_t* changed /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
