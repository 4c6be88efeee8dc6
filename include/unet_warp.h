/* C ABI of the non-linear refinement of a parcellation, exported by libunet_hip.so: a displacement field on a lattice, fitted on the
 * device after the affine registration of unet_register.h, and the carrying of an atlas through the warped map.  The reference's
 * template path assumes TIPL's non-linear stage (cdm_cu.hpp), which is not in the reference tree: everything below is this
 * project's definition (parity with TIPL NOT pinned).  Every choice is made on integer counts, so the device
 * is pinned to a numpy restatement bit for bit (tests/warp_ref.py).
 *
 * Grids, tissue, map, Nearest    those of unet_register.h: x fastest, fewer than 2^31 voxels; uint8 or uint16 tissue at any
 *            alignment, 2 <= T <= 16, a value >= T reads as 0; map = 12 HOST floats, a subject voxel (x, y, z) ->
 *                p_r = ((m[3r]*x + m[3r+1]*y) + m[3r+2]*z) + t_r
 *            in fp32, every product and every sum rounded, no fused multiply-add; a position q = p + 0.5f is inside when
 *            0 <= q < (float)dim on every axis (a NaN is outside), its index is (int)floorf(q), an outside position reads tissue 0.
 * Lattice    spacing g in {4, 8, 16, 32} subject voxels, lg = log2 g.  Nodes sit at (i*g, j*g, k*g); nx = (sw + g - 1) / g + 1
 *            along x, likewise ny, nz.  The field D is device int32 {nz, ny, nx, 3}, x fastest then component: a displacement in
 *            TEMPLATE voxels in units of 1/256 (Q8), |D| <= UNET_WARP_MAX_DISP.
 * Warped position   of voxel (x, y, z), cell (x >> lg, y >> lg, z >> lg), offsets fx = x & (g - 1), fy, fz:
 *                n_r  = the sum over the cell's 8 corners of (wx*wy*wz) * D_r,  wx in {g - fx, fx}, likewise wy, wz
 *                p'_r = p_r + ldexpf((float)n_r, -(8 + 3*lg))
 *            n_r is exact in int32 (g^3 * 32767 < 2^31); the rest is one int -> float conversion (round to nearest even), an exact
 *            scaling and one fp32 add.  q = p' + 0.5f.  A zero field gives q the bits of the affine map alone.
 * hist, Score   unet_register.h's at stride 1 under the warped positions: hist[a*T + b] over every subject voxel; the score is
 *            int64 agree - disagree, agree = the sum over t >= 1 of hist[t][t], disagree = the sum over a != b of hist[a][b].
 *
 * One sweep at (g, step, limit): 8 colour passes, colour c = (i&1) | (j&1)<<1 | (k&1)<<2 of node (i, j, k), c = 0..7 in order.
 *   Support      of node (i, j, k): the subject voxels with (i-1)g < x < (i+1)g, likewise y and z, clipped to the grid.  Supports
 *                of one colour are disjoint and no node reads a node of its own colour (every corner of its 8 cells differs from
 *                it in parity somewhere): a pass updates the field in place and does not depend on the order.
 *   Candidates   0 = stay; 1..6 = D + step*e for e = +x, -x, +y, -y, +z, -z.  step: Q8, 1 <= step <= UNET_WARP_MAX_DISP.
 *   Admissible   candidate 0 always; a moved one when every component stays within +-UNET_WARP_MAX_DISP and
 *                |D_cand[a] - D_n[a]| <= limit for every axis a and each of the up to 6 lattice neighbours n that exist.
 *   Choice       the local score of a candidate: agree - disagree over the support's voxels under the field with this node set to
 *                the candidate.  The best admissible score wins, the lowest index among equals.  A node with an empty support stays.
 *   info         device int64[2] = {nodes changed, nodes visited (those with a support that is not empty)}, summed over the 8 passes.
 *   The global score never decreases across a pass.
 *
 * Refine (g -> g/2): fine node (i, j, k) = (S + 4) >> 3 (arithmetic shift) per component, S the sum over the 8 combinations of the
 *   coarse indices {i>>1, min((i>>1) + (i&1), nx_c - 1)} x the same for j, k: the rounded mean of the 1, 2, 4 or 8 coarse nodes
 *   around it.  sw, sh, sd, g: the subject grid and the COARSE spacing, g in {8, 16, 32}.
 *
 * Fit: levels = HOST, n_levels x {g, first_step, last_step, max_sweeps, limit} ints, 1 <= n_levels <= UNET_WARP_MAX_LEVELS; g
 *   strictly halves from level to level; steps are powers of two, UNET_WARP_MAX_STEP >= first_step >= last_step >= 1;
 *   1 <= max_sweeps <= UNET_WARP_MAX_SWEEPS; limit >= 0; at most UNET_WARP_MAX_ROWS (level, step) pairs in all.  The field starts
 *   at zero on the first level's lattice.  Per level, for step = first_step, first_step/2, .., last_step: up to max_sweeps sweeps,
 *   ending early after a sweep that changed no node; then refine to the next level.  The early end is carried on the device: the
 *   host enqueues every launch of the schedule and reads nothing back; a sweep's kernels return at once when the preceding sweep of
 *   the same (level, step) changed nothing, which is bit-identical to not ending early.
 *   D_out    device, the field on the LAST level's lattice.
 *   report   device int64[UNET_WARP_MAX_ROWS * 5], filled completely: per (level, step), in order, {g, step, sweeps run, nodes
 *            changed in the last sweep run, the global score after it (one hist pass)}; the rows past the schedule hold -1.
 *
 * Carry: the carry of unet_register.h (direct, rescued, left, and the -2 rule for an index that reaches no voxel) evaluated at q =
 *   p' + 0.5f.  out: device uint16 on the subject grid; counts: device uint32[3*T], optional (NULL), filled completely.
 *
 * impl   UNET_WARP_IMPL_NODE     a block (a wave for g = 4) per node of the active colour: the node's 3x3x3 neighbourhood of D staged
 *                                in LDS, seven int32 sums in registers, reduced by lane shuffles and then LDS; one thread chooses
 *        UNET_WARP_IMPL_VOXEL    a thread per voxel, integer atomic adds into 7 counters per node in the scratch, then a pick kernel:
 *                                the second witness of the bits and the measured baseline
 *        UNET_WARP_IMPL_DEFAULT  the faster of the two as measured
 * scratch   unet_warp_scratch_bytes(subject grid, T, levels): what a fit of these levels needs; a sweep at g needs what a one-level
 *           list {g, ..} needs.  Any alignment.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Report arrays are filled completely by the call.  Argument errors
 * (a null pointer, a bad size, sbytes / tbytes other than 1 or 2, T, g, a level, a step, max_sweeps or a limit out of range, a
 * misaligned array, a scratch that is too small, an unknown impl) are found before any device call, with a message naming the
 * argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_WARP_H
#define UNET_WARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_WARP_IMPL_DEFAULT = 0, UNET_WARP_IMPL_NODE = 1, UNET_WARP_IMPL_VOXEL = 2 };

#define UNET_WARP_MAX_TISSUES 16
#define UNET_WARP_MAX_DISP 32767
#define UNET_WARP_MAX_STEP 16384
#define UNET_WARP_MAX_LEVELS 4
#define UNET_WARP_MAX_SWEEPS 16
#define UNET_WARP_MAX_ROWS 32

int unet_warp_lattice(int sw, int sh, int sd, int g, int* nx, int* ny, int* nz);

int unet_warp_scratch_bytes(int sw, int sh, int sd, int n_tissues, const int* levels /* host, n_levels x 5 */, int n_levels, size_t* bytes);

int unet_warp_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                   int n_tissues, const float* map /* host, 12 */, const int32_t* D, int g, uint32_t* hist, void* stream);

int unet_warp_sweep(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    int n_tissues, const float* map /* host, 12 */, int32_t* D, int g, int step, int limit, int64_t* info, int impl,
                    void* scratch, size_t scratch_bytes, void* stream);

int unet_warp_refine(const int32_t* D_coarse, int sw, int sh, int sd, int g, int32_t* D_fine, void* stream);

int unet_warp_fit(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                  int n_tissues, const float* map /* host, 12 */, const int* levels /* host, n_levels x 5 */, int n_levels, int32_t* D_out,
                  int64_t* report, int impl, void* scratch, size_t scratch_bytes, void* stream);

int unet_warp_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    const uint16_t* atlas, int n_tissues, const float* map /* host, 12 */, const int32_t* D, int g, uint16_t* out,
                    uint32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
