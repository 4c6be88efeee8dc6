/* C ABI of the starts of a registration, exported by libunet_hip.so: where an affine pattern search over two tissue maps begins.
 * The register module's search (unet_register.h) is local: from its default start (the voxel-size ratio on the diagonal, the two
 * centre voxels on each other) it stalls on a subject rotated by more than a few degrees or off the middle of its field of view.
 * Here: the image moments of the two foregrounds (translation and scale), a small grid of rotated starts ranked by the register
 * module's joint histograms at a coarse stride, and up to four full searches advancing in lock-step inside the same launches, the
 * winner chosen by its FINAL score.  Everything is this project's definition (parity with the reference's TIPL registration NOT
 * pinned, as in unet_register.h).  All device work is integer counting, or fp32 with every operation rounded and no fused
 * multiply-add, so the device is pinned to numpy restatements bit for bit (tests/start_ref.py).
 *
 * Grids, tissue values, maps, the nearest sample, the counted voxels, the score and the search (state, candidates, stages, levels,
 * the limit, map_out, trace, info) are those of unet_register.h, word for word; they are not repeated here.
 *
 * unet_start_moments -- PINNED (integer adds only): the raw moments of a volume's foreground, from ONE pass.
 *   volume   device, uint8 or uint16 (vbytes 1 or 2), any alignment, x fastest, w x h x d, fewer than 2^31 voxels, every dimension
 *            <= 65535.  A voxel is foreground when lo <= v <= hi (0 <= lo, hi <= 65535; lo > hi: an empty range, every sum 0).
 *            A tissue map: lo = 1, hi = T - 1.  An image of intensity codes over `bins` bins: lo = 1, hi = bins - 1 (the darkest bin
 *            and "none" dropped).
 *   sums     device uint64[10], 8-byte aligned, OVERWRITTEN (no memset by the caller): n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz over
 *            the foreground voxels' integer coordinates.  Under the limits above every sum stays below 2^63.
 *   A thread sums its voxels in registers, a wave reduces by lane shuffles, a block through LDS, and one 64-bit integer add per sum
 *   per block reaches memory; no loop waits on another block.
 *
 * unet_start_pick -- PINNED: the scores of S joint histograms and the n starts a search should run from.  One block.
 *   hist     device uint32[S*T*T], read only, 1 <= S <= 125: what the register module's histogram call leaves for S maps (in passes
 *            of at most 25 maps).
 *   scores   device int64[S], filled completely: agree - disagree of every table, background agreement not counted.
 *   picked   device int32[n], 1 <= n <= min(S, 4): the n best scores in descending order, the lowest index first among equal scores.
 *            always in [0, S): when that index is not among them it replaces the last.  always = -1: nothing is forced.
 *   maps     device float[S*12], read only; inits: device float[n*12], inits[j] = maps[picked[j]].
 *
 * unet_start_search -- n searches (1 <= n <= 4) over the same two tissue maps, one per entry of inits.
 *   inits    DEVICE float[n*12] (unet_start_pick's, nothing read back).  step, stages: HOST, as in unet_register.h.
 *   State s ends with exactly the maps_out[s] (device float[n*12]), trace[s] (device int64[n*max_iterations*4], optional, NULL) and
 *   info[s] (device int64[n*4]) that the register module's search produces alone from inits[s] with the same step, stages and
 *   max_iterations: state by state, bit for bit.
 *   best     device int32[1]: the state with the greatest key (converged, stage of the last iteration, score of the last iteration's
 *            winner), compared in that order, the lowest index among equal keys.  (A score taken at a coarser stride is not
 *            comparable with one taken at stride 1: the stage comes first.)  best_map: device float[12] = maps_out[best].
 *   impl     UNET_START_IMPL_BATCHED     one init launch, then max_iterations pairs of (histogram, step) launches however many
 *                                        states there are: a histogram block handles the live states one after another, each at
 *                                        its own stride, through one LDS table of K*T*T <= 6400 counters flushed between states;
 *                                        the step launch has one block per state; one closing launch writes best and best_map.
 *                                        Once every state is done the remaining launches return at once.  No host synchronisation.
 *            UNET_START_IMPL_SEQUENTIAL  the n searches one after another through the register module's own entry point, then the
 *                                        same closing launch: the yardstick and the second witness of the bits.  That entry point
 *                                        takes its start from the host, so this implementation copies inits to the host and WAITS
 *                                        for the stream once, before the first search.
 *            UNET_START_IMPL_DEFAULT     the faster of the two as measured.
 *   scratch  the caller's, unet_start_scratch_bytes(n_tissues, n), any alignment.
 *
 * Apart from IMPL_SEQUENTIAL's one wait no call synchronises with the host: everything is ordered on the caller's stream, so calls
 * on different streams with different scratch may run concurrently.  Outputs are filled completely by the call.  Argument errors (a
 * null pointer, a bad size, vbytes / sbytes / tbytes other than 1 or 2, lo, hi, S, n, always, T, a stage, a step or max_iterations
 * out of range, a misaligned output, a scratch that is too small, an unknown impl) are found before any device call, with a message
 * naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_START_H
#define UNET_START_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_START_IMPL_DEFAULT = 0, UNET_START_IMPL_BATCHED = 1, UNET_START_IMPL_SEQUENTIAL = 2 };

#define UNET_START_MAX_STATES 4
#define UNET_START_MAX_STARTS 125
#define UNET_START_MAX_DIM 65535

int unet_start_scratch_bytes(int n_tissues, int n, size_t* bytes);

int unet_start_moments(const void* volume, int vbytes, int w, int h, int d, int lo, int hi, uint64_t* sums, void* stream);

int unet_start_pick(const uint32_t* hist, int S, int n_tissues, const float* maps /* device, S x 12 */, int n, int always,
                    int64_t* scores, float* inits, int32_t* picked, void* stream);

int unet_start_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                      int n_tissues, const float* inits /* device, n x 12 */, int n, const float* step /* host, 12 */,
                      const int* stages /* host, n_stages x 3 */, int n_stages, int max_iterations, float* maps_out, int64_t* trace,
                      int64_t* info, int32_t* best, float* best_map, int impl, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
