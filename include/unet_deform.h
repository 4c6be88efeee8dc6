/* C ABI of the geometry of a fitted lattice warp, exported by libunet_hip.so: the Jacobian determinant of map + field at every subject
 * voxel, and a subject-grid volume brought onto the template grid through the inverse of map + field.  The two lattice warps
 * (unet_warp.h: tissue maps; unet_cowarp.h: intensity codes) fit a field that pulls template things onto the subject grid; this
 * header is the way back, and the report of what the field did to volume.  The inverse of "affine + trilinear lattice field" has no
 * closed form: it is a fixed-point iteration per template voxel.  Everything below is this project's definition (parity with TIPL
 * NOT pinned).  All arithmetic is fp32, one rounding per operation, no fused multiply-add, left to right as written, so the device
 * is pinned to a numpy restatement bit for bit (tests/deform_ref.py).
 *
 * Grids, map, lattice, field    those of unet_warp.h, unchanged: x fastest, fewer than 2^31 voxels; subject sw x sh x sd, template
 *            tw x th x td; map = 12 HOST floats (m[0..8] a row-major matrix, m[9..11] a translation) taking subject voxel centres
 *            to template voxel centres; spacing g in {4, 8, 16, 32}, lg = log2 g, nodes at (i*g, j*g, k*g), nx = (sw + g - 1) / g + 1
 *            (ny, nz alike); the field D is device int32 {nz, ny, nx, 3} in Q8 TEMPLATE voxels, |D| <= UNET_DEFORM_MAX_DISP (a field
 *            of either warp).  At an integer voxel the displacement is ldexpf((float)n_r, -(8 + 3*lg)), n_r the 8-corner sum of
 *            unet_warp.h.
 *
 * Jacobian   for subject voxel (x, y, z) in cell (x >> lg, y >> lg, z >> lg) with fx = x & (g - 1) (fy, fz alike) the derivative of
 *            n_r along x is the exact integer
 *                G[r][0] = the sum over the cell's 8 corners c of (c & 1 ? +1 : -1) * wy * wz * D_r[corner],
 *            wy = (c & 2 ? fy : g - fy), wz = (c & 4 ? fz : g - fz); G[r][1] and G[r][2] are the same along y (sign by c & 2, weights
 *            wx * wz) and z (sign by c & 4, weights wx * wy).  |G| <= g^2 * 65534 fits int32.  Then
 *                J[r][c] = m[3r + c] + ldexpf((float)G[r][c], -(8 + 3*lg))
 *                det     = (a*(e*i - f*h) - b*(d*i - f*g)) + c*(d*h - e*g)      with a..i = J[0][0]..J[2][2]
 *            It is the derivative of the cell's own trilinear piece: on a cell face the piece of the cell the voxel belongs to.
 *   det      device float32 on the subject grid, or NULL: then only info is formed.  A NaN is stored as the quiet NaN 0x7FC00000,
 *            whatever sign and payload the arithmetic gave it (pos below alike).
 *   info     device int64[4] = {voxels, voxels with !(det > 0) (folded, or NaN), the smallest det, the largest det}.  The two
 *            extremes are carried as the order-preserving keys unet_stats.h's exact float extremes use: with b the bits of the
 *            float, key = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), an unsigned 32-bit number in an int64.  A NaN det counts as
 *            folded and enters neither extreme; when no det entered, the two hold their start values 0xFFFFFFFF and 0.
 *
 * Field at a position    the continuous field e(s) at a subject position s = (s_x, s_y, s_z), along x:
 *                t = s_x * (1 / g);  t = t > 0 ? t : 0  (a NaN becomes 0);  t = t < (float)(nx - 1) ? t : (float)(nx - 1);
 *                c = min((int)floorf(t), nx - 2);  f = t - (float)c
 *            and the same along y and z.  Per component r the 8 corners of cell (c_x, c_y, c_z) are taken as (float)D_r and
 *            interpolated a + f * (b - a) along x, then y, then z; the result times 2^-8 is e_r(s) in template voxels.  Positions
 *            outside the lattice take the field of its border.  At an integer voxel e equals the displacement above exactly.
 *
 * Pull       inv = 12 HOST floats, the inverse of map (subject position of a template position).  The ABI does NOT check that inv
 *            inverts map: whatever is given is iterated with.  For template voxel u = (u_x, u_y, u_z), integers taken as floats:
 *                s0_r = ((inv[3r]*u_x + inv[3r+1]*u_y) + inv[3r+2]*u_z) + inv[9+r];    s = s0
 *                iters times:  e = e(s);  s_r = s0_r - ((inv[3r]*e_0 + inv[3r+1]*e_1) + inv[3r+2]*e_2)
 *            0 <= iters <= UNET_DEFORM_MAX_ITERS: a fixed count, no data-dependent loop.  D may be NULL: then s = s0, e = 0, and g
 *            and iters are still checked.
 *   sample   UNET_DEFORM_KIND_F32: the volume (device float32 on the subject grid) at s under unet_space.h's LINEAR rule (inside when
 *            0 <= s <= dim - 1 on every axis, the lower corner floorf(s), the upper one clamped, a + t * (b - a) along x, y, z),
 *            0 outside.  UNET_DEFORM_KIND_U8 / _U16 (labels, tissue maps): the voxel (int)floorf(q), q = s + 0.5f, when
 *            0 <= q < (float)dim on every axis (a NaN is outside), else 0.
 *   out      device, on the template grid, in the volume's type.  The volume and out may sit at any multiple of their element size.
 *   pos      device float32 {3, td, th, tw} or NULL: s of every template voxel (the dense inverse).
 *   info     device int64[2] = {template voxels whose s is inside the subject grid under the U8 rule, whatever the kind; of those,
 *            the voxels NOT converged}: with p_r = ((m[3r]*s_x + m[3r+1]*s_y) + m[3r+2]*s_z) + m[9+r], a voxel is not converged
 *            when !(fabsf((p_r + e_r(s)) - u_r) <= 1/16) on some axis.  A folded or wild field shows here, never as a hang.
 *
 * impl   UNET_DEFORM_IMPL_GLOBAL   a thread per template voxel, every corner of every round gathered from global memory
 *        UNET_DEFORM_IMPL_TILE     per 16 x 4 x 4 brick of template voxels a block stages the lattice window the brick's s0 can reach (its
 *                                  8 corners under inv, two nodes of margin) in LDS; a thread whose cell leaves the window reads
 *                                  global memory for that round; a window above UNET_DEFORM_MAX_WINDOW = 1536 nodes sends the whole
 *                                  brick down the global path.  The arithmetic is the same: the bits are the same
 *        UNET_DEFORM_IMPL_DEFAULT  the faster of the two as measured
 *
 * No call synchronises with the host: everything is ordered on the caller's stream, and there is no scratch, so calls on different
 * streams may run concurrently.  Outputs are filled completely by the call.  No kernel loop waits for another thread, and every loop
 * has a fixed bound; every atomic is an integer add, min or max.  Argument errors (a null pointer other than the optional ones, a
 * bad size, g, iters, kind or impl, a misaligned D, det, pos or info, a volume or out off its element size) are found before any
 * device call, with a message naming the argument.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_DEFORM_H
#define UNET_DEFORM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNET_DEFORM_IMPL_DEFAULT = 0, UNET_DEFORM_IMPL_GLOBAL = 1, UNET_DEFORM_IMPL_TILE = 2 };
enum { UNET_DEFORM_KIND_F32 = 0, UNET_DEFORM_KIND_U8 = 1, UNET_DEFORM_KIND_U16 = 2 };

#define UNET_DEFORM_MAX_DISP 32767
#define UNET_DEFORM_MAX_ITERS 32
#define UNET_DEFORM_MAX_WINDOW 1536

int unet_deform_jacobian(int sw, int sh, int sd, const float* map /* host, 12 */, const int32_t* D, int g, float* det /* or NULL */,
                         int64_t* info, void* stream);

int unet_deform_pull(const void* volume, int kind, int sw, int sh, int sd, int tw, int th, int td, const float* map /* host, 12 */,
                     const float* inv /* host, 12 */, const int32_t* D /* or NULL */, int g, int iters, void* out,
                     float* pos /* or NULL */, int64_t* info, int impl, void* stream);

#ifdef __cplusplus
}
#endif
#endif
