/* C ABI of the intensity-inhomogeneity correction, exported by libunet_hip.so: the smooth multiplicative shading of an MR scan
 * fitted as a field on a lattice, over the voxels whose tissue a label map says is uniform, and removed.  Everything below is this
 * project's definition (parity with any outside tool NOT pinned).  The device works on integers, apart from one
 * rounded fp32 multiply in apply, so it is pinned to a numpy restatement bit for bit (tests/bias_ref.py).
 *
 * Grid       x fastest, fewer than 2^31 voxels.  The volume v is device float32; labels is device uint8 or uint16 (lbytes 1 or 2)
 *            at any byte alignment; classes = HOST, 1 <= K <= UNET_BIAS_MAX_CLASSES distinct label values in [0, 65535] whose tissue
 *            is taken to be uniform.  A voxel's class t is the index of its label in classes; a label that is not listed has none.
 * Log code   q, device int32 on the grid, Q12: for a finite, normal v > 0 with unbiased exponent e and x = (mantissa | 1 << 23) << 8,
 *            f = the 16 fraction bits that DESIGN.md §32's L forms from x (16 times: y = (x * x) >> 31 in 64 bits; when y >= 2^32
 *            the bit is 1 and x = y >> 1, else the bit is 0 and x = y), and
 *                q = (e * 65536 + f) >> 4          (arithmetic shift: 4096 * log2 v, truncated towards minus infinity)
 *            q(1) = 0, q(2) = 4096, q(3) = 6492; |q| <= 2^19.  Zero, negative, subnormal, infinite and NaN values give
 *            UNET_BIAS_NONE.
 * Lattice    that of unet_warp.h: spacing g in {4, 8, 16, 32}, lg = log2 g, nodes at (i*g, j*g, k*g), nx = (sw + g - 1) / g + 1
 *            (ny, nz alike).  The field B is device int32 {nz, ny, nx} in Q12 log2 units, |B| <= UNET_BIAS_MAX (a factor of 4).
 *            At voxel (x, y, z), cell (x >> lg, y >> lg, z >> lg), fx = x & (g - 1) (fy, fz alike):
 *                n = the sum over the cell's 8 corners of (wx*wy*wz) * B,   wx in {g - fx, fx}, likewise wy, wz
 *            exactly as unet_warp.h's n_r; |n| <= g^3 * 8192 = 2^28.  The field's value is n / g^3; b = n >> 3*lg (arithmetic).
 * Levels     device int64 {UNET_BIAS_MAX_CLASSES, 3}, filled completely, row t = {m_t, count, sum}: over the voxels of class t with
 *            a valid q, sum = the sum of (q - b) (below 2^51), count their number, m_t = floor(sum / count) (floor division, also of
 *            a negative sum).  A class without such a voxel, and every row t >= K, holds {UNET_BIAS_NONE, 0, 0}.
 * Residual   r, device int16 on the grid, 16-byte aligned: r = q - m_t when the voxel has a class t, m_t is not UNET_BIAS_NONE, q is
 *            valid and |q - m_t| <= clip; otherwise UNET_BIAS_SKIP.  0 <= clip <= UNET_BIAS_MAX.  A voxel outside the clip is left
 *            out, not clamped: that is the outlier rule.  The sweeps read only this 2-byte volume.
 *
 * One sweep at (g, lam): 8 colour passes, colours and supports as in unet_warp.h (a pass updates B in place and does not depend on
 *   the order: supports of a colour are disjoint, and no node reads a node of its own colour).  For node i of the colour, over the
 *   voxels of its support with r != UNET_BIAS_SKIP:
 *       W = (g - |x - i_x g|) * (g - |y - i_y g|) * (g - |z - i_z g|)     the node's own corner weight at the voxel
 *       e = r * g^3 - n          S1 = the sum of W * e          S2 = the sum of W * W
 *   and with L = lam * g^6 (a link to a lattice neighbour weighs as lam voxels sitting on the node), over the up to 6 lattice
 *   neighbours that exist:
 *       num = S1 + L * the sum of (B_nbr - B_i)          den = S2 + L * (the number of neighbours)
 *       d   = floor((2 * num + den) / (2 * den)) when den > 0, else 0          B_i <- clamp(B_i + d, +-UNET_BIAS_MAX)
 *   d is the rounded minimiser of the convex quadratic that the exact energy, the sum of e^2 over the voxels that count plus L * the
 *   sum over the lattice's links of (B_i - B_j)^2, is in B_i: the energy does not rise across a node update, clamped or not.
 *   A node with den = 0 (no voxel that counts and lam = 0) stays and is not visited.
 *   info     device int64[2] = {nodes changed (B_i differs afterwards), nodes visited (den > 0)}, summed over the 8 passes.
 *   int64    |r| <= 2^13 and g^3 <= 2^15, so |e| <= 2^28 + 2^28 = 2^29.  The sum of W over a support is at most (g^2)^3 = g^6 <=
 *            2^30, so |S1| <= 2^59; S2 <= g^3 * g^6 <= 2^45.  0 <= lam <= UNET_BIAS_MAX_LAM = 2^12 bounds L by 2^42, L * the sum of
 *            the differences by 2^42 * 6 * 2^14 < 2^59 and den by 2^45 + 6 * 2^42 < 2^46: |2 * num + den| < 2^61 + 2^46 and
 *            2 * den < 2^47 fit.
 * Cost       device int64[2] = {the sum of (r - b)^2 over the voxels with r != UNET_BIAS_SKIP (each below 2^30), their number}: the
 *            reduced cost, in Q12 squared.
 * Refine (g -> g/2): fine node (i, j, k) = (S + 4) >> 3 (arithmetic), S the sum over the 8 combinations of the coarse indices of
 *            unet_warp.h's refine: the rounded mean.  sw, sh, sd, g: the grid and the COARSE spacing, g in {8, 16, 32}.
 *
 * Fit: levels = HOST, n_levels x {g, sweeps, lam} ints, 1 <= n_levels <= UNET_BIAS_MAX_LEVELS, g strictly halving, 1 <= sweeps <=
 *   UNET_BIAS_MAX_SWEEPS; 1 <= outer <= UNET_BIAS_MAX_OUTER.  B starts at zero on the first level's lattice.  Per level, per outer
 *   round: the levels under the field as it stands, the residual from them, then up to `sweeps` sweeps, ending early after a sweep
 *   that changed no node; after the level's rounds, refine to the next level.  The early end is carried on the device as in
 *   unet_warp.h's fit: the host enqueues every launch of the schedule and reads nothing back, and a sweep's kernels return at once
 *   when the preceding sweep of the same round changed nothing, which is bit-identical to not ending early.
 *   B_out    device, the field on the LAST level's lattice.
 *   report   device int64[UNET_BIAS_MAX_ROWS * 6], filled completely: per (level, outer round), in order, {g, outer round, sweeps
 *            run, nodes changed in the last sweep run, cost, count of the cost} after the round's sweeps, under the round's
 *            residual; the rows past the schedule hold -1.
 *
 * Apply: c = (-n + (1 << (3*lg - 1))) >> 3*lg (arithmetic; Q12, |c| <= 8192), k = c >> 12, j = c & 4095;
 *            out = ldexpf(v * T[j], k)
 *   with T[j] the float32 nearest to 2^(j / 4096) (the table belongs to the definition: csrc/bias_table.h): one rounded fp32
 *   multiply and one scaling.  Where c = 0 (a zero field everywhere) out has the bits of v.  Elsewhere a NaN result is stored as the
 *   quiet NaN 0x7FC00000; an infinity stays one.  gain: device float32 on the grid or NULL, ldexpf(T[j], k) itself; v may be NULL
 *   when only the gain is wanted (then out must be NULL too).
 *
 * impl   UNET_BIAS_IMPL_NODE     a block (a wave for g = 4) per node of the active colour: the node's 3x3x3 neighbourhood of B staged
 *                                in LDS, the int16 residual read in aligned 16-byte runs along x, S1 and S2 as int64 in registers,
 *                                reduced by lane shuffles and then LDS; one thread updates the node
 *        UNET_BIAS_IMPL_VOXEL    a thread per voxel, 64-bit integer atomic adds into two counters per node in the scratch, then an
 *                                update kernel: the second witness of the bits and the measured baseline
 *        UNET_BIAS_IMPL_DEFAULT  the faster of the two as measured
 * scratch   unet_bias_scratch_bytes(grid, levels): what a fit of these levels needs (any outer).  A sweep at g needs only the two
 *           counters per node: 256 + 16 * nx * ny * nz bytes rounded up to a multiple of 256, which the size of any list with g
 *           as its last level covers.  Any alignment.
 * range     sweep, levels, cost, refine and apply take the field as given: they do not check |B| <= UNET_BIAS_MAX, and their int32
 *           arithmetic (n, e) is only defined inside it.  A field of fit, of sweep or of refine from fields inside it stays inside.
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and all scratch is the caller's, so calls on
 * different streams with different scratch may run concurrently.  Outputs and reports are filled completely by the call.  Every
 * atomic is an integer add: the results do not depend on the schedule.  Argument errors (a null pointer, a bad size, lbytes other
 * than 1 or 2, K, a class, g, lam, clip, sweeps, outer or a level out of range, a misaligned array, a scratch that is too small, an
 * unknown impl) are found before any device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_BIAS_H
#define UNET_BIAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_BIAS_IMPL_DEFAULT = 0, UNET_BIAS_IMPL_NODE = 1, UNET_BIAS_IMPL_VOXEL = 2 };

#define UNET_BIAS_NONE (-2147483647 - 1)
#define UNET_BIAS_SKIP (-32768)
#define UNET_BIAS_MAX 8192
#define UNET_BIAS_MAX_CLASSES 16
#define UNET_BIAS_MAX_LAM 4096
#define UNET_BIAS_MAX_LEVELS 4
#define UNET_BIAS_MAX_SWEEPS 16
#define UNET_BIAS_MAX_OUTER 8
#define UNET_BIAS_MAX_ROWS 32

int unet_bias_lattice(int sw, int sh, int sd, int g, int* nx, int* ny, int* nz);

int unet_bias_scratch_bytes(int sw, int sh, int sd, const int* levels /* host, n_levels x 3 */, int n_levels, size_t* bytes);

int unet_bias_logcode(const float* v, int64_t voxels, int32_t* q, void* stream);

int unet_bias_levels(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes /* host, K */, int K,
                     const int32_t* B, int g, int64_t* levels_out, void* stream);

int unet_bias_residual(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes /* host, K */, int K,
                       const int64_t* levels_in, int clip, int16_t* r, void* stream);

int unet_bias_sweep(const int16_t* r, int sw, int sh, int sd, int32_t* B, int g, int lam, int64_t* info, int impl, void* scratch,
                    size_t scratch_bytes, void* stream);

int unet_bias_refine(const int32_t* B_coarse, int sw, int sh, int sd, int g, int32_t* B_fine, void* stream);

int unet_bias_cost(const int16_t* r, int sw, int sh, int sd, const int32_t* B, int g, int64_t* cost, void* stream);

int unet_bias_fit(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes /* host, K */, int K,
                  int clip, const int* levels /* host, n_levels x 3 */, int n_levels, int outer, int32_t* B_out, int64_t* report, int impl,
                  void* scratch, size_t scratch_bytes, void* stream);

int unet_bias_apply(const float* v /* or NULL */, int sw, int sh, int sd, const int32_t* B, int g, float* out /* or NULL */,
                    float* gain /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
