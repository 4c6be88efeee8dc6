/* C ABI of the co-registration of two intensity images, exported by libunet_hip.so: an affine search that maximises the mutual
 * information of a fixed and a moving image.  It is what puts a second image of one subject (a T2 / FLAIR beside a T1, an FA or SUV
 * map beside the scan) on the scan's grid: the map it finds is the 12-float map of unet_space.h, and resampling the moving image
 * through it yields the co-registered channel.  The search of unet_register.h aligns two tissue label maps; its score means nothing
 * between modalities.  The reference declares linear_cuda (evaluate.cpp:19-26), TIPL's affine registration; TIPL is not in the
 * reference tree and nothing there calls it, so everything below is this project's definition (parity with TIPL NOT pinned).  Every
 * choice is made on integers, the score included, so the device is pinned to a numpy restatement bit for bit (tests/coreg_ref.py).
 *
 * Grids      x fastest, fewer than 2^31 voxels.  fixed: the destination grid fw x fh x fd (the role of unet_register.h's subject);
 *            moving: the source grid mw x mh x md (the role of its template).
 * Map        12 floats, m[9] (row-major) then t[3]: a fixed voxel (x, y, z) -> a moving position in voxel units,
 *                px = ((m0*x + m1*y) + m2*z) + t0     py = ((m3*x + m4*y) + m5*z) + t1     pz = ((m6*x + m7*y) + m8*z) + t2
 *            in fp32, every product and every sum rounded, no fused multiply-add (the layout and the arithmetic of unet_space.h's map).
 * Nearest    q = p + 0.5f per axis (one fp32 add).  The position is inside when 0 <= q < (float)dim on every axis; a NaN is
 *            outside.  The index is (int)floorf(q) per axis.
 * Code       a voxel's intensity as uint8 in [0, bins], bins in {8, 16, 32}; the code `bins` means "none".
 *            unet_coreg_code: scale = (float)bins / (hi - lo) in fp32 (one subtraction, one division, formed on the host);
 *            t = (v - lo) * scale, one subtraction and one multiplication, each rounded to nearest, never fused (as unet_stats.h's
 *            code); the code is 0 for t < 0, bins - 1 for t >= bins - 1, otherwise (int)t.  A NaN becomes `bins`.  -inf reads 0,
 *            +inf reads bins - 1.  Codes handed to the calls below are uint8 at any alignment, read only; a value above bins reads
 *            as `bins`.
 * Counted    with stride s in {1, 2, 4, 8}: the fixed voxels with x % s == 0 && y % s == 0 && z % s == 0 (unet_register.h's rule).
 * hist       hist[(k*bins + a)*(bins+1) + b], a < bins, b <= bins: under map k, the counted fixed voxels whose code is a and
 *            whose nearest moving voxel has the code b; b = bins when the position is outside or the moving code is `bins`.  A
 *            counted fixed voxel whose own code is `bins` is skipped.  So every map counts the same N voxels: leaving the overlap
 *            moves counts into the column `bins`, which is penalised (below), not rewarded.
 * L          the integer logarithm.  L(0) = 0.  For 1 <= n < 2^31: e = 31 - clz(n), x = n << (31 - e) as a uint32, f = 0; 16
 *            times: y = ((uint64)x * x) >> 31; if y >= 2^32 then f = 2f + 1, x = y >> 1, else f = 2f, x = y.  L = (e << 16) | f:
 *            65536 * log2(n), truncated, in fixed point.  L(3) = 103872, L(2^31 - 1) = 2031615.
 * Score      int64 of one histogram: with r_a its row sums (over b <= bins), c_b its column sums, N its total,
 *                the sum over a < bins, b < bins of n_ab * (L(n_ab) + L(N) - L(r_a) - L(c_b)).
 *            The column b = bins counts toward r_a and N and adds no term.  This is N times the mutual information in units of
 *            2^-16 bit; it is signed and its magnitude stays below 2^54.  Defined for N < 2^31, which every histogram of
 *            unet_coreg_hist satisfies; the sums of a hand-made table are taken modulo 2^32.
 *
 * unet_coreg_code -- PINNED: image (device fp32, voxels entries, 1 <= voxels < 2^31) -> codes (device uint8, any alignment).
 *
 * unet_coreg_hist -- PINNED (integer adds only): K joint histograms, one per map, from ONE pass over the fixed image.
 *   maps   HOST, K x 12 floats, 1 <= K <= 25, consumed before the call returns: they travel in the launch arguments.
 *   hist   device uint32[K*bins*(bins+1)], filled completely (no memset by the caller).
 *   impl   UNET_COREG_IMPL_LDS      a block gathers whole maps' counters in its LDS table and flushes one global add per non-zero
 *                                   counter.  The table holds 25 maps at 8 and 16 bins (6800 counters at 16); at 32 bins it
 *                                   holds 13, and a block walks its voxels once per group of 13 maps.  The bits do not depend on it
 *          UNET_COREG_IMPL_GLOBAL   global adds only: the measured baseline and the second witness of the bits
 *          UNET_COREG_IMPL_DEFAULT  the faster of the two as measured
 *          Both merge runs of equal (map, a, b) keys along x in registers before adding: without it the background cell (0, 0)
 *          takes every add.
 *   scratch  reserved: not used today, may be NULL.
 *
 * unet_coreg_score -- PINNED: scores[k] (device int64[K]) = the score of hist[k] (device uint32[K*bins*(bins+1)], read only).
 *
 * unet_coreg_search -- the centred pattern search of unet_register.h over the 12 map parameters, entirely on the device; only the
 * histogram and the score differ.
 *   State    12 fp32 parameters c: c0..c8 the map's matrix, c9..c11 = u, the moving position of the fixed grid's centre voxel
 *            (cx, cy, cz) = (fw/2, fh/2, fd/2) (integer division).  init (HOST, a map) is converted once:
 *                u_r = ((m[3r]*cx + m[3r+1]*cy) + m[3r+2]*cz) + t_r
 *   Map of a state: the matrix unchanged, t_r = u_r - ((c[3r]*cx + c[3r+1]*cy) + c[3r+2]*cz), every operation rounded to fp32 in
 *            that order.
 *   step     HOST, 12 floats, each finite and >= 0, at least one > 0.  step[i] == 0 freezes parameter i; nine zeros in front give
 *            a translation-only search.
 *   stages   HOST, n_stages x {stride, first_level, last_level} ints, 1 <= n_stages <= 4, 0 <= first_level <= last_level <= 20.
 *   One iteration at stage g, level l: candidate 0 is the state; for the j-th parameter with step[i] > 0, in ascending i, candidate
 *            1 + 2j has c_i + ldexpf(step[i], -l) and candidate 2 + 2j has c_i - ldexpf(step[i], -l) (one fp32 add each).  All
 *            K = 1 + 2P <= 25 joint histograms are taken in one pass at the stage's stride.  The best score wins, the lowest
 *            candidate index among equal scores.  Candidate 0 wins: l += 1, and when l passes last_level the next stage begins at
 *            its first_level; after the last stage the search is done (converged = 1).  Another candidate wins: it becomes the state.
 *   Limit    the search also ends after max_iterations iterations (1..1024; converged = 0): the state is then exactly that after
 *            max_iterations iterations.  An iteration that finishes the last stage reports converged = 1 also when it is the last
 *            one allowed.
 *   map_out  device, 12 floats: the map of the final state.
 *   trace    device int64[max_iterations * 4], optional (NULL): per iteration {stage, level, winning candidate, its score}; the
 *            rows never reached hold -1.
 *   info     device int64[4] = {iterations run, converged, score of the last iteration's winner, stage of the last iteration}.
 *   The host enqueues max_iterations pairs of launches (histograms, then one block that scores, picks, advances and writes the
 *   next candidates) and reads nothing back; both return at once when the state says done.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's
 * (unet_coreg_scratch_bytes), so calls on different streams with different scratch may run concurrently.  Outputs are filled
 * completely by the call.  No kernel loop waits for another thread, and every loop has a fixed bound.  Argument errors (a null
 * pointer, a bad size, a grid of 2^31 voxels or more, bins, K, stride, a stage, a step or max_iterations out of range, a range that
 * is not finite or has lo >= hi, a misaligned output, a scratch that is too small, an unknown impl) are found before any device
 * call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_COREG_H
#define UNET_COREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_COREG_IMPL_DEFAULT = 0, UNET_COREG_IMPL_LDS = 1, UNET_COREG_IMPL_GLOBAL = 2 };

#define UNET_COREG_MAX_BINS 32
#define UNET_COREG_MAX_MAPS 25
#define UNET_COREG_MAX_STAGES 4
#define UNET_COREG_MAX_LEVEL 20
#define UNET_COREG_MAX_ITERATIONS 1024

int unet_coreg_scratch_bytes(int64_t fixed_voxels, int bins, int max_iterations, size_t* bytes);

int unet_coreg_code(const float* image, int64_t voxels, float lo, float hi, int bins, uint8_t* codes, void* stream);

int unet_coreg_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                    const float* maps /* host, K x 12 */, int K, int stride, uint32_t* hist, int impl, void* scratch, size_t scratch_bytes,
                    void* stream);

int unet_coreg_score(const uint32_t* hist, int K, int bins, int64_t* scores, void* stream);

int unet_coreg_search(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                      const float* init /* host, 12 */, const float* step /* host, 12 */, const int* stages /* host, n_stages x 3 */,
                      int n_stages, int max_iterations, float* map_out, int64_t* trace, int64_t* info, int impl, void* scratch,
                      size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
