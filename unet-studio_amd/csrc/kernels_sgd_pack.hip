// The optimizer update that also writes the next forward's filter packs (unet_sgd_step_packed).
//
// k_sgd holds every updated parameter in a register when it stores it, and a filter pack (kernels_mfma_conv.hip, pack_unit_t) is a bf16
// rounding and a permutation of exactly those values.  k_sgd_pack therefore walks the flat parameter buffer in the plan's update tiles
// (SgdTile, kernels.h) instead of linearly: one block loads p, g, m of a tile over its contiguous source runs, applies sgd_update.h's
// arithmetic, stores p, m and g = 0, keeps the new values as bf16 in LDS and writes every fragment of every pack unit of the tile, the
// all-zero ones included, in pack_unit_t's layout.  Elements no pack job reads (biases, norm parameters, heads, the Cin = 1 conv, layers
// on other kernels) are plain ranges of the same table.  The parameters are read once and written once; the separate pack launches of
// the next training forward, their two re-reads of the parameters and their stretch beside the forward's first kernels go away.
#include "mfma_util.h"
#include "sgd_update.h"

namespace unet {

constexpr int SGDP_THREADS = 512;
constexpr int SGDP_LDS_ELEMS = SGD_TILE_MAX * (SGD_TILE_MAX * 27 + 1);   // [r0][r1][tap] bf16, rows padded by one element (54 KB: 2 blocks per CU)

// four consecutive elements at the 16-B aligned index qb, of which those in [lo, hi) belong to the run
struct SgdQuad {
    float4 p, g, m;
    int64_t qb;
    int kind;   // 0: nothing, 1: all four inside (16-B accesses), 2: some inside (4-B accesses)
};
__device__ __forceinline__ void quad_load(SgdQuad& q, const float* p, const float* g, const float* m, int64_t qb, int64_t lo, int64_t hi, bool on) {
    q.qb = qb;
    q.kind = !on ? 0 : (qb >= lo && qb + 4 <= hi) ? 1 : 2;
    q.p = q.g = q.m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q.kind == 1) {
        q.p = *(const float4*)(p + qb); q.g = *(const float4*)(g + qb); q.m = *(const float4*)(m + qb);
    } else if (q.kind == 2) {
        float* pv = &q.p.x; float* gv = &q.g.x; float* mv = &q.m.x;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (qb + e >= lo && qb + e < hi) { pv[e] = p[qb + e]; gv[e] = g[qb + e]; mv[e] = m[qb + e]; }
    }
}
// update, store, and (row != nullptr) leave the new values as bf16 at row[index - lo]
__device__ __forceinline__ void quad_finish(SgdQuad& q, float* p, float* g, float* m, int64_t lo, int64_t hi, const SgdUpdate& upd, float wd,
                                            __bf16* row) {
    if (q.kind == 0) return;
    upd(q.p.x, q.g.x, q.m.x, wd); upd(q.p.y, q.g.y, q.m.y, wd); upd(q.p.z, q.g.z, q.m.z, wd); upd(q.p.w, q.g.w, q.m.w, wd);
    const float* pv = &q.p.x; const float* mv = &q.m.x;
    if (q.kind == 1) {
        *(float4*)(p + q.qb) = q.p; *(float4*)(m + q.qb) = q.m; *(float4*)(g + q.qb) = q.g;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q.qb + e >= lo && q.qb + e < hi) { p[q.qb + e] = pv[e]; m[q.qb + e] = mv[e]; g[q.qb + e] = 0.f; }
    }
    if (row) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q.qb + e >= lo && q.qb + e < hi) row[q.qb + e - lo] = (__bf16)pv[e];
    }
}

// every fragment of every pack unit of `jb` inside tile `t`, from the tile's bf16 values lds[r0][r1][tap] (row stride RS)
__device__ __forceinline__ void tile_pack(const SgdTile& t, const PackJob& jb, const __bf16* lds, int RS, char* ws) {
    const int CK = jb.CK, T = jb.T, mode = jb.mode;
    const int KSTEPS = CK == 32 ? T : (T + 1) / 2;
    const int NTT = jb.Co / 16;
    const bool row0 = mode == PK_CONV_FWD || mode == PK_CONVT_DGRAD;     // rows run along the tensor's first dimension
    const int P = (mode == PK_CONVT_FWD || mode == PK_CONV_S2_DGRAD) ? 8 : 1;   // row planes: conv_trans taps / output parities
    const int nq = (row0 ? t.n1 : t.n0) / CK, nr = (row0 ? t.n0 : t.n1) / 16;
    const int q0 = (row0 ? t.d1 : t.d0) / CK;
    const int plane = mode == PK_CONV_S2_DGRAD ? jb.A : jb.B;            // rows per plane (P == 8 only)
    __bf16* out = (__bf16*)(ws + jb.dst_off);
    const int items = P * nq * nr * KSTEPS * 64;
    for (int it = threadIdx.x; it < items; it += SGDP_THREADS) {
        const int lane = it & 63, row = lane & 15;
        int x = it >> 6;
        const int ks = x % KSTEPS; x /= KSTEPS;
        const int ri = x % nr; x /= nr;
        const int qi = x % nq, pp = x / nq;
        int tap, c0;
        if (CK == 32) { tap = ks; c0 = 8 * (lane >> 4); }
        else { tap = 2 * ks + (lane >> 5); c0 = 8 * ((lane >> 4) & 1); }
        const int rr = ri * 16 + row, cc = qi * CK + c0;                 // row and first k-channel, relative to the tile
        int base = -1, step = 0;                                         // LDS index of element 0 and the stride between k-channels
        if (tap < T) {
            if (row0) { base = rr * RS + cc * t.T + tap; step = t.T; }
            else if (mode == PK_CONV_DGRAD) { base = cc * RS + rr * 27 + 26 - tap; step = RS; }
            else if (mode == PK_CONVT_FWD) { base = cc * RS + rr * 8 + pp; step = RS; }
            else {                                                       // PK_CONV_S2_DGRAD: parity pp, taps k in {0,1}^3
                const int pk[3] = {(pp >> 2) & 1, (pp >> 1) & 1, pp & 1}, kk[3] = {(tap >> 2) & 1, (tap >> 1) & 1, tap & 1};
                int ft[3];
                bool ok = true;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    if (pk[d] == 0) { ok = ok && kk[d] == 0; ft[d] = 1; }
                    else ft[d] = kk[d] == 0 ? 2 : 0;
                }
                if (ok) { base = cc * RS + rr * 27 + ft[0] * 9 + ft[1] * 3 + ft[2]; step = RS; }
            }
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = base >= 0 ? lds[base + e * step] : (__bf16)0.f;
        const int q = q0 + qi;
        const int nt = (row0 ? t.d0 : (P == 8 ? pp * plane : 0) + t.d1) / 16 + ri;
        *(bf16x8*)(out + ((((int64_t)q * KSTEPS + ks) * NTT + nt) * 64 + lane) * 8) = o;
    }
}

__global__ void __launch_bounds__(SGDP_THREADS) k_sgd_pack(float* p, float* g, float* m, const SgdTile* __restrict__ tiles,
                                                           const PackJob* __restrict__ jobs, char* ws, int with_dgrad,
                                                           int* __restrict__ zero, int nzero, const float* __restrict__ partial, int nblk,
                                                           float lr, float momentum, int nesterov, float wdecay, float clip_norm,
                                                           float grad_scale, float* norm_out) {
    __shared__ double red[256];
    __shared__ float s_coef;
    __shared__ __bf16 lds[SGDP_LDS_ELEMS];
    // the deep levels' arrival counters, as the first pack launch of a forward clears them (kernels_mfma_conv.hip, k_mfma_pack_batched)
    if (zero && blockIdx.x == 0)
        for (int i = threadIdx.x; i < nzero; i += SGDP_THREADS) zero[i] = 0;
    const SgdUpdate upd{sgd_clip_coef(partial, nblk, clip_norm, norm_out, red, &s_coef) * grad_scale, lr, momentum, nesterov};
    const SgdTile t = tiles[blockIdx.x];
    const float wd = t.wd * wdecay;
    const bool filter = t.job_fwd >= 0;
    // runs: n0 rows of n1 * T contiguous elements (filter tile) or the one range (plain); all runs of a tile start at the same offset
    // from a 16-B boundary (row pitch and d1 * T are multiples of 4), so they cover the same number of aligned quads
    const int nrun = filter ? t.n0 : 1;
    const int64_t len = filter ? (int64_t)t.n1 * t.T : t.count, pitch = filter ? (int64_t)t.D1 * t.T : 0;
    const int64_t first = filter ? t.off + ((int64_t)t.d0 * t.D1 + t.d1) * t.T : t.off;
    const int qr = (int)(((first + len + 3) >> 2) - (first >> 2));
    const int RS = SGD_TILE_MAX * t.T + 1;
    const int items = nrun * qr;
    for (int it = threadIdx.x; it < items; it += 2 * SGDP_THREADS) {      // two quads in flight per thread
        SgdQuad a, b;
        const int ib = it + SGDP_THREADS;
        const int ra = it / qr, rb = ib / qr;
        const int64_t la = first + ra * pitch, lb = first + rb * pitch;
        quad_load(a, p, g, m, (la & ~(int64_t)3) + 4 * (it - ra * qr), la, la + len, true);
        quad_load(b, p, g, m, (lb & ~(int64_t)3) + 4 * (ib - rb * qr), lb, lb + len, ib < items);
        quad_finish(a, p, g, m, la, la + len, upd, wd, filter ? lds + ra * RS : nullptr);
        quad_finish(b, p, g, m, lb, lb + len, upd, wd, filter ? lds + rb * RS : nullptr);
    }
    if (!filter) return;
    __syncthreads();
    tile_pack(t, jobs[t.job_fwd], lds, RS, ws);
    if (with_dgrad && t.job_dgrad >= 0) tile_pack(t, jobs[t.job_dgrad], lds, RS, ws);
}

int64_t sgd_tile_units(const SgdTile& t, const PackJob& jb) {
    const bool row0 = jb.mode == PK_CONV_FWD || jb.mode == PK_CONVT_DGRAD;
    const int P = (jb.mode == PK_CONVT_FWD || jb.mode == PK_CONV_S2_DGRAD) ? 8 : 1;
    const int ni = row0 ? t.n1 : t.n0, no = row0 ? t.n0 : t.n1;
    if (ni % jb.CK || no % 16 || t.d0 % SGD_TILE_MAX || t.d1 % SGD_TILE_MAX) return -1;
    return (int64_t)P * (ni / jb.CK) * (no / 16);
}

void launch_sgd_pack(float* p, float* g, float* m, const SgdTile* tiles_dev, int ntiles, const PackJob* jobs_dev, void* ws, int with_dgrad,
                     int* zero, int nzero, const float* partial, int nblk, float lr, float momentum, int nesterov, float wdecay,
                     float clip_norm, float grad_scale, float* norm_out, hipStream_t s) {
    if (ntiles <= 0) return;
    k_sgd_pack<<<(unsigned)ntiles, SGDP_THREADS, 0, s>>>(p, g, m, tiles_dev, jobs_dev, (char*)ws, with_dgrad, zero, nzero, partial, nblk, lr,
                                                         momentum, nesterov, wdecay, clip_norm, grad_scale, norm_out);
}

}  // namespace unet
