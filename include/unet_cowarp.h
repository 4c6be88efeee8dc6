/* C ABI of the non-linear refinement of a co-registration, exported by libunet_hip.so: a displacement field on a lattice, fitted on
 * the device after the affine search of the co-registration header ("the coreg header" below: its test lets no other header spell
 * its file name) and scored by mutual information, and the resampling of the moving image through map + field.  It is to that
 * header what unet_warp.h is to unet_register.h: an EPI-distorted FA or b0 map is off by several voxels against the T1 in a way no
 * affine map removes, and `stats` of such a map is wrong at every region's boundary.  TIPL's non-linear stage is not in the
 * reference tree: everything below is this project's definition (parity with TIPL NOT pinned).  Every choice is made on integers,
 * so the device is pinned to a numpy restatement bit for bit (tests/cowarp_ref.py).
 *
 * The idea.  Mutual information is not a sum over voxels, so a lattice node cannot score its own support with it.  The term of each
 * cell of the joint histogram, L(n_ab) + L(N) - L(r_a) - L(c_b), can be frozen into a table W[a][b] at the start of a sweep: a node's
 * local score is then the sum of W[fixed code][moving code at the candidate position] over its support, which is unet_warp.h's
 * sweep with a weight table in place of +1 / -1.
 *
 * Grids, codes, Nearest    those of the coreg header: x fastest, fewer than 2^31 voxels; fixed fw x fh x fd, moving mw x mh x md; uint8
 *            codes at any alignment, read only, bins in {8, 16, 32}, a code above bins reads as `bins` = "none"; a position
 *            q = p + 0.5f is inside when 0 <= q < (float)dim on every axis (a NaN is outside), its index is (int)floorf(q).
 * Map, lattice, field, warped position, refine, admissibility, colours, supports, candidates 0..6    those of unet_warp.h, word for
 *            word, with the fixed grid in the subject's role and the moving grid in the template's: map = 12 HOST floats; nodes at
 *            (i*g, j*g, k*g), nx = (fw + g - 1) / g + 1; the field D is device int32 {nz, ny, nx, 3} in Q8 MOVING voxels,
 *            |D| <= UNET_COWARP_MAX_DISP; p' = p + ldexpf((float)n, -(8 + 3*lg)), n the 8-corner sum; q = p' + 0.5f.
 *            EXCEPT: g in {4, 8, 16} only.  A support then holds at most 31^3 = UNET_COWARP_MAX_SUPPORT voxels, which the bound
 *            below needs.  A field fitted here is a valid argument of unet_warp.h's refine (the lattices are the same); there is no
 *            second refine.
 * hist       uint32[bins * (bins + 1)], hist[a * (bins + 1) + b]: every fixed voxel (stride 1) whose own code is a < bins, b the
 *            code of its nearest moving voxel at the warped position; b = bins when the position is outside or the moving code is
 *            "none".  With a zero field it is the coreg header's hist of the one map at stride 1, bit for bit.
 * weights    int16[bins * (bins + 1)] from one hist.  With r_a the row sums (over b <= bins), c_b the column sums over a, N the
 *            total, and L the integer logarithm of the coreg header (L(0) = 0):
 *                W[a][b]    = (L(n_ab) + L(N) - L(r_a) - L(c_b)) >> 8     (arithmetic shift)   for b < bins
 *                W[a][bins] = min(0, the minimum over b < bins of W[a][b])
 *            leaving the image is never better than the worst match inside.  Defined for N < 2^31, which every hist of this
 *            header satisfies (the sums of a hand-made table are taken modulo 2^32 and W is cut to its low 16 bits).
 *            Bound: n_ab <= r_a, n_ab <= c_b <= N < 2^31 and 0 <= L < 2^21 give -2^21 < L(n) - L(r) <= 0 <= L(N) - L(c) < 2^21,
 *            so |W| <= 2^13.  Over a support of at most UNET_COWARP_MAX_SUPPORT = 29791 voxels every local sum stays below
 *            29791 * 2^13 < 2^28 < 2^29: seven int32 sums per node suffice.
 * Score      the coreg header's Score of a hist: N times the mutual information in units of 2^-16 bit, int64.
 *
 * One sweep at (g, step, limit): the hist of the current field, its weights, then the 8 colour passes of unet_warp.h with W frozen.
 *   Choice       the local score of a candidate: the sum of W[a][b] over the support's voxels whose code a is < bins, under the field
 *                with this node set to the candidate.  A fixed "none" voxel adds nothing and belongs to no support.  The best
 *                admissible score wins, the lowest index among equals.  A node whose support holds no voxel with a code stays and
 *                is not visited.
 *   info         device int64[2] = {nodes changed, nodes visited}, summed over the 8 passes.
 *   Within a sweep the frozen-W total, the sum over a, b of hist[a][b] * W[a][b], never decreases across a pass.  The true Score is
 *   NOT guaranteed to rise from sweep to sweep; the report carries it.
 *
 * Fit: unet_warp.h's schedule, limits and report layout.  levels = HOST, n_levels x {g, first_step, last_step, max_sweeps, limit}
 *   ints, 1 <= n_levels <= UNET_COWARP_MAX_LEVELS; g strictly halves from level to level; steps are powers of two,
 *   UNET_COWARP_MAX_STEP >= first_step >= last_step >= 1; 1 <= max_sweeps <= UNET_COWARP_MAX_SWEEPS; limit >= 0; at most
 *   UNET_COWARP_MAX_ROWS (level, step) pairs in all.  The field starts at zero on the first level's lattice.  Per level, for step =
 *   first_step, first_step/2, .., last_step: up to max_sweeps sweeps, ending early after a sweep that changed no node; then refine to
 *   the next level.  The early end is carried on the device: the host enqueues every launch of the schedule and reads nothing back; a
 *   sweep's hist, weights and pass kernels return at once when the preceding sweep of the same (level, step) changed nothing, which
 *   is bit-identical to not ending early (the same field gives the same hist, the same W and again no change).
 *   D_out    device, the field on the LAST level's lattice.
 *   report   device int64[UNET_COWARP_MAX_ROWS * 5], filled completely: per (level, step), in order, {g, step, sweeps run, nodes
 *            changed in the last sweep run, the Score after it (one hist pass)}; the rows past the schedule hold -1.
 *
 * Resample: out (device fp32 on the fixed grid) = the moving volume (device fp32) at p' (no + 0.5f) under unet_space.h's LINEAR
 *   rule: inside when 0 <= p' <= dim - 1 on every axis (a NaN is outside); the lower corner floorf(p'), the upper one clamped to
 *   dim - 1; lerp a + t * (b - a) along x, then y, then z, every operation rounded, no fused multiply-add; outside -> 0.  With a zero
 *   field it is unet_space.h's resample (LINEAR, one channel) bit for bit.
 *
 * impl   UNET_COWARP_IMPL_NODE     a block per node of the active colour (64 threads at g = 4, 256 at g = 8, 1024 at g = 16): W and the
 *                                  node's 3x3x3 neighbourhood of D staged in LDS, seven int32 sums in registers, reduced by lane
 *                                  shuffles and then LDS; one thread chooses
 *        UNET_COWARP_IMPL_VOXEL    a thread per voxel, int32 atomic adds into 8 counters per node in the scratch (the seven sums and the
 *                                  voxels with a code), then a pick kernel that zeroes them again: the second witness of the bits and
 *                                  the measured baseline
 *        UNET_COWARP_IMPL_DEFAULT  the faster of the two as measured
 * scratch   unet_cowarp_scratch_bytes(fixed grid, bins, levels): what a fit of these levels needs; a sweep at g needs what a
 *           one-level list {g, ..} needs.  Any alignment.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Outputs are filled completely by the call.  No kernel loop waits
 * for another thread, and every loop has a fixed bound; every atomic is an integer add.  Argument errors (a null pointer, a bad size,
 * bins, g (32 included), a level, a step, max_sweeps or a limit out of range, a misaligned array, a scratch that is too small, an
 * unknown impl) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_COWARP_H
#define UNET_COWARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_COWARP_IMPL_DEFAULT = 0, UNET_COWARP_IMPL_NODE = 1, UNET_COWARP_IMPL_VOXEL = 2 };

#define UNET_COWARP_MAX_BINS 32
#define UNET_COWARP_MAX_DISP 32767
#define UNET_COWARP_MAX_STEP 16384
#define UNET_COWARP_MAX_LEVELS 3
#define UNET_COWARP_MAX_SWEEPS 16
#define UNET_COWARP_MAX_ROWS 32
#define UNET_COWARP_MAX_SUPPORT 29791
#define UNET_COWARP_MAX_WEIGHT 8192

int unet_cowarp_scratch_bytes(int fw, int fh, int fd, int bins, const int* levels /* host, n_levels x 5 */, int n_levels, size_t* bytes);

int unet_cowarp_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                     const float* map /* host, 12 */, const int32_t* D, int g, uint32_t* hist, void* stream);

int unet_cowarp_weights(const uint32_t* hist, int bins, int16_t* weights, void* stream);

int unet_cowarp_sweep(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                      const float* map /* host, 12 */, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch,
                      size_t scratch_bytes, void* stream);

int unet_cowarp_fit(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                    const float* map /* host, 12 */, const int* levels /* host, n_levels x 5 */, int n_levels, int32_t* D_out,
                    int64_t* report, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_cowarp_resample(const float* moving, int mw, int mh, int md, int fw, int fh, int fd, const float* map /* host, 12 */,
                         const int32_t* D, int g, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
