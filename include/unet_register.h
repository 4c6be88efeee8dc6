/* C ABI of the parcellation of a subject, exported by libunet_hip.so: an affine registration of two tissue maps and the carrying of
 * an atlas through the map it finds.  This is what `--template ... --atlas ...` exists for: the corrected atlas of unet_atlas.h
 *  lives on the template grid, an evaluation's label output is a tissue map on the subject's grid (classes 0-4, the
 * five the template image carries, evaluate.hpp:26-38).  The reference declares linear_cuda (evaluate.cpp:19-26), TIPL's affine
 * registration (cuda.cu:1); TIPL is not in the reference tree and nothing there calls it, so everything below is this project's
 * definition (parity with TIPL NOT pinned).  Every choice is made on integers, so the device is
 * pinned to a numpy restatement bit for bit (tests/test_register_host.py).
 *
 * Grids      x fastest, fewer than 2^31 voxels.  subject: the destination grid sw x sh x sd; template: the source grid tw x th x td.
 * Tissue     uint8 or uint16 on either side (sbytes, tbytes: 1 or 2), read only, any alignment.  T = n_tissues, 2 <= T <= 16; a
 *            value >= T reads as 0 on both sides (load_template's replace_if(v >= 5, 0), evaluate.hpp:38, on the fly).
 * Map        12 floats, m[9] (row-major) then t[3]: a subject voxel (x, y, z) -> a template position in voxel units,
 *                px = ((m0*x + m1*y) + m2*z) + t0     py = ((m3*x + m4*y) + m5*z) + t1     pz = ((m6*x + m7*y) + m8*z) + t2
 *            in fp32, every product and every sum rounded, no fused multiply-add (the layout and the arithmetic of unet_space.h's map).
 * Nearest    q = p + 0.5f per axis (one fp32 add).  The position is inside when 0 <= q < (float)dim on every axis; a NaN is
 *            outside.  The index is (int)floorf(q) per axis.  An outside position reads template tissue 0.
 * hist       hist[a*T + b] = the counted subject voxels whose tissue reads a and whose nearest template sample reads b.
 * Counted    with stride s in {1, 2, 4, 8}: the voxels with x % s == 0 && y % s == 0 && z % s == 0.
 * Score      int64, agree - disagree: agree = the sum over t >= 1 of hist[t][t], disagree = the sum over a != b of hist[a][b].
 *
 * unet_reg_hist -- PINNED (integer adds only): K joint histograms, one per map, from ONE pass over the subject.
 *   maps   HOST, K x 12 floats, 1 <= K <= 25, consumed before the call returns: they travel in the launch arguments.
 *   hist   device uint32[K*T*T], filled completely (no memset by the caller).
 *   impl   UNET_REG_IMPL_LDS      a block gathers its K*T*T <= 6400 counters in LDS and flushes one global add per non-zero counter
 *          UNET_REG_IMPL_GLOBAL   global adds only: the measured baseline and the second witness of the bits
 *          UNET_REG_IMPL_DEFAULT  the faster of the two as measured
 *          Both merge runs of equal (map, a, b) keys along x in registers before adding.
 *   scratch  reserved: not used today, may be NULL.
 *
 * unet_reg_search -- a centred pattern search over the 12 map parameters, entirely on the device.
 *   State    12 fp32 parameters c: c0..c8 the map's matrix, c9..c11 = u, the template position of the subject's centre voxel
 *            (cx, cy, cz) = (sw/2, sh/2, sd/2) (integer division).  init (HOST, a map) is converted once:
 *                u_r = ((m[3r]*cx + m[3r+1]*cy) + m[3r+2]*cz) + t_r
 *   Map of a state: the matrix unchanged, t_r = u_r - ((c[3r]*cx + c[3r+1]*cy) + c[3r+2]*cz), every operation rounded to fp32 in
 *            that order.
 *   step     HOST, 12 floats, each finite and >= 0, at least one > 0.  step[i] == 0 freezes parameter i.
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
 * unet_reg_carry -- the atlas (device uint16 on the template grid, read only) carried onto the subject grid through map (HOST).
 *   For a subject voxel whose tissue reads a, in this order:
 *   a == 0    0.
 *   direct    the centre is the nearest template voxel, if the position is inside.  When it exists, its tissue reads a and its
 *             atlas value is non-zero: that value.
 *   rescued   otherwise the 3x3x3 cube around the nearest index, taken even when that index is outside (an index below -2 or above
 *             dim + 1, or that of a NaN, reaches no voxel: it is read as -2); of the cube voxels inside the template, those whose
 *             tissue reads a and whose atlas value is non-zero are eligible; the most frequent value among them, the smallest among
 *             equal counts.
 *   left      no eligible voxel: 0.
 *   out       device uint16 on the subject grid.  counts: device uint32[3*T], optional (NULL), filled completely: direct, rescued
 *             and left per tissue in [0, T), [T, 2T) and [2T, 3T).
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's
 * (unet_reg_scratch_bytes), so calls on different streams with different scratch may run concurrently.  Report arrays are filled
 * completely by the call.  Argument errors (a null pointer, a bad size, sbytes / tbytes other than 1 or 2, T, K, stride, a stage, a
 * step or max_iterations out of range, a misaligned report, a scratch that is too small, an unknown impl) are found before any
 * device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_REGISTER_H
#define UNET_REGISTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_REG_IMPL_DEFAULT = 0, UNET_REG_IMPL_LDS = 1, UNET_REG_IMPL_GLOBAL = 2 };

#define UNET_REG_MAX_TISSUES 16
#define UNET_REG_MAX_MAPS 25
#define UNET_REG_MAX_STAGES 4
#define UNET_REG_MAX_LEVEL 20
#define UNET_REG_MAX_ITERATIONS 1024

int unet_reg_scratch_bytes(int64_t subject_voxels, int n_tissues, int max_iterations, size_t* bytes);

int unet_reg_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                  int n_tissues, const float* maps /* host, K x 12 */, int K, int stride, uint32_t* hist, int impl, void* scratch,
                  size_t scratch_bytes, void* stream);

int unet_reg_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    int n_tissues, const float* init /* host, 12 */, const float* step /* host, 12 */,
                    const int* stages /* host, n_stages x 3 */, int n_stages, int max_iterations, float* map_out, int64_t* trace,
                    int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_reg_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                   const uint16_t* atlas, int n_tissues, const float* map /* host, 12 */, uint16_t* out, uint32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
