// The recalibration pass (include/unet_recal.h): one fused pass over the level-0 logits of a volume, the truth label and an optional
// mask into the negative log-likelihood under softmax(beta * x) and its slope in beta, for up to 8 candidate beta at once, as integer
// sums.
//
//   k_recal_init    the running table in the scratch: zeros
//   k_recal_eval    grid-stride over units of RC_UNIT voxels, one unit per thread at a time.  The mask and the label come first; sweep
//                   A over the channels finds M = max_c x_c, a NaN and x_t; sweep B forms d_c = x_c - M once per channel and, for each
//                   candidate, e_c = expf(beta * d_c), s += e_c, a += e_c * d_c.  The terms nll = logf(s) - beta * dt and g = a / s -
//                   dt are clamped, scaled by 2^20, rounded to integers and added to the thread's 2 K 64-bit sums; the six head counts
//                   stay in registers as well.  Up to RC_CACHE channels of the unit stay in registers between the sweeps (every index
//                   a compile-time one), beyond that they are read again (from L2: the same thread, a moment later).  At the end the
//                   sums reduce across the wave with shuffles, across the block's waves through LDS, and the block sends one 64-bit
//                   integer add per table entry into the running table.
//                   K is the candidate count rounded up to 1, 2, 4 or 8; the spare candidates repeat the first one (they can clamp
//                   nothing it does not) and are not added.
//   k_recal_finish  the running table -> int64 tables: stored, or added when accumulate
// Every atomic is an integer add: the results do not depend on the schedule.  No float atomics, no inline assembly.
#include "../../include/unet_recal.h"
#include "device_util.h"

#pragma clang fp contract(off)   // the header's expressions as written: no fused multiply-adds anywhere in this file

namespace unet {

namespace {

constexpr int RC_T = UNET_RECAL_BLOCK_UNITS;         // threads per block, a unit each
constexpr int RC_MAXB = 512;                         // grid cap, two blocks a CU
constexpr int RC_UNIT = UNET_RECAL_UNIT;
constexpr int RC_CACHE = UNET_RECAL_CACHE;
constexpr int RC_HEAD = UNET_RECAL_HEAD;
constexpr int RC_LEN = UNET_RECAL_TABLE_LEN;
constexpr int RC_KMAX = UNET_RECAL_MAX_BETAS;
constexpr float RC_CLAMP = (float)UNET_RECAL_CLAMP;
constexpr float RC_SCALE = (float)(1 << UNET_RECAL_SCALE_BITS);
static_assert(RC_UNIT == 4, "a unit is one float4 per plane");
static_assert(RC_T % 64 == 0 && RC_MAXB * RC_T == UNET_RECAL_GRID_UNITS, "the header states the grid's stride");
static_assert(RC_LEN == RC_HEAD + 2 * RC_KMAX && RC_LEN <= 64 && RC_CACHE == 8, "head, then (nll, g) per candidate");

typedef unsigned long long u64;

enum { RC_OUT = -1, RC_VALID = 0, RC_BAD = 1, RC_INVALID = 2, RC_SKIPPED = 3, RC_IMPOSSIBLE = 4 };   // RC_OUT: behind the volume's end

struct Args {
    const float* logits;
    const float* label;
    const uint8_t* mask;
    int C, nb;                  // nb: the candidates that are added
    int64_t S;
    bool mask_vec;              // 4-byte aligned: a unit is one 32-bit word
    float beta[RC_KMAX];
};

// the unit's values of one plane; VEC: S % 4 == 0 and the plane is 16-B aligned, so a unit is inside the volume
template <bool VEC> __device__ __forceinline__ void rc_load(const float* __restrict__ p, int64_t i0, int n, float (&x)[RC_UNIT]) {
    if constexpr (VEC) {
        const float4 q = *(const float4*)(p + i0);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j) x[j] = j < n ? p[i0 + j] : 0.f;
    }
}

__global__ void __launch_bounds__(64) k_recal_init(u64* __restrict__ tab) {
    if (threadIdx.x < RC_LEN) tab[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(64) k_recal_finish(const u64* __restrict__ tab, int accumulate, int64_t* __restrict__ out) {
    const int i = threadIdx.x;
    if (i < RC_LEN) out[i] = (accumulate ? out[i] : (int64_t)0) + (int64_t)tab[i];
}

template <int K, bool CACHED, bool VEC>
__global__ void __launch_bounds__(RC_T) k_recal_eval(const Args a, u64* tab) {
    __shared__ u64 part[RC_T / 64][RC_LEN];
    const int C = a.C;
    const int64_t S = a.S, units = (S + RC_UNIT - 1) / RC_UNIT, step = (int64_t)gridDim.x * RC_T;
    float beta[K];
#pragma unroll
    for (int k = 0; k < K; ++k) beta[k] = a.beta[k];
    long long nll[K], g[K];
    unsigned head[RC_HEAD];          // 32 bits: a thread takes a small share of fewer than 2^31 voxels
#pragma unroll
    for (int k = 0; k < K; ++k) { nll[k] = 0; g[k] = 0; }
#pragma unroll
    for (int h = 0; h < RC_HEAD; ++h) head[h] = 0u;
    for (int64_t u = (int64_t)blockIdx.x * RC_T + threadIdx.x; u < units; u += step) {
        const int64_t i0 = u * RC_UNIT;
        const int n = (int)min((int64_t)RC_UNIT, S - i0);
        // ---- the mask and the label
        float lab[RC_UNIT];
        rc_load<VEC>(a.label, i0, n, lab);
        unsigned mk[RC_UNIT];
        if (!a.mask) {
#pragma unroll
            for (int j = 0; j < RC_UNIT; ++j) mk[j] = 1u;
        } else if (VEC && a.mask_vec) {
            const unsigned w = *(const unsigned*)(a.mask + i0);
#pragma unroll
            for (int j = 0; j < RC_UNIT; ++j) mk[j] = (w >> (8 * j)) & 255u;
        } else {
#pragma unroll
            for (int j = 0; j < RC_UNIT; ++j) mk[j] = j < n ? (unsigned)a.mask[i0 + j] : 0u;
        }
        int t[RC_UNIT];
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j) {
            const float l = lab[j];
            t[j] = l > -1.0f && l < (float)C ? (int)l : -1;   // false for a NaN
        }
        // ---- sweep A: the max, a NaN, x_t
        float x[RC_UNIT], M[RC_UNIT], xt[RC_UNIT];
        float keep[CACHED ? RC_CACHE : 1][RC_UNIT];
        bool nan[RC_UNIT];
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j) { M[j] = -INFINITY; xt[j] = 0.f; nan[j] = false; }
        auto first = [&](const float (&y)[RC_UNIT], int c) {
#pragma unroll
            for (int j = 0; j < RC_UNIT; ++j) {
                nan[j] = nan[j] || y[j] != y[j];
                M[j] = fmaxf(M[j], y[j]);                    // a NaN is dropped here and kept in nan[j]
                xt[j] = c == t[j] ? y[j] : xt[j];
            }
        };
        if constexpr (CACHED) {
#pragma unroll
            for (int c = 0; c < RC_CACHE; ++c)
                if (c < C) rc_load<VEC>(a.logits, (int64_t)c * S + i0, n, keep[c]);
#pragma unroll
            for (int c = 0; c < RC_CACHE; ++c)
                if (c < C) first(keep[c], c);
        } else {
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                rc_load<VEC>(a.logits, (int64_t)c * S + i0, n, x);
                first(x, c);
            }
        }
        // ---- what each voxel is: the head counts
        bool valid[RC_UNIT], any = false;
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j) {
            const bool bad = nan[j] || !(fabsf(M[j]) < INFINITY);      // a NaN, a +inf, or all channels -inf
            const int kind = j >= n ? RC_OUT : mk[j] == 0u ? RC_SKIPPED : t[j] < 0 ? RC_INVALID : bad ? RC_BAD
                           : xt[j] == -INFINITY ? RC_IMPOSSIBLE : RC_VALID;
#pragma unroll
            for (int h = 0; h < 5; ++h) head[h] += kind == h ? 1u : 0u;
            valid[j] = kind == RC_VALID;
            any = any || valid[j];
        }
        if (!any) continue;
        // ---- sweep B: s and a of every candidate
        float s[RC_UNIT][K], w[RC_UNIT][K];
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) { s[j][k] = 0.f; w[j][k] = 0.f; }
        auto second = [&](const float (&y)[RC_UNIT]) {
#pragma unroll
            for (int j = 0; j < RC_UNIT; ++j) {
                const float d = y[j] - M[j];
                const bool fin = d != -INFINITY;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float e = expf(beta[k] * d);
                    s[j][k] += e;
                    w[j][k] += fin ? e * d : 0.f;
                }
            }
        };
        if constexpr (CACHED) {
#pragma unroll
            for (int c = 0; c < RC_CACHE; ++c)
                if (c < C) second(keep[c]);
        } else {
            for (int c = 0; c < C; ++c) {
                rc_load<VEC>(a.logits, (int64_t)c * S + i0, n, x);
                second(x);
            }
        }
        // ---- the terms, clamped and quantised
#pragma unroll
        for (int j = 0; j < RC_UNIT; ++j) {
            const float dt = xt[j] - M[j];
            bool sat = false;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float tn = logf(s[j][k]) - beta[k] * dt;
                float tg = w[j][k] / s[j][k] - dt;
                tn = valid[j] ? tn : 0.f;                    // a voxel that is not counted may hold anything
                tg = valid[j] ? tg : 0.f;
                sat = sat || fabsf(tn) > RC_CLAMP || fabsf(tg) > RC_CLAMP;
                tn = fminf(fmaxf(tn, -RC_CLAMP), RC_CLAMP);
                tg = fminf(fmaxf(tg, -RC_CLAMP), RC_CLAMP);
                nll[k] += llrintf(tn * RC_SCALE);
                g[k] += llrintf(tg * RC_SCALE);
            }
            head[5] += sat ? 1u : 0u;
        }
    }
    // ---- the thread's sums -> the wave's -> the block's -> one add per entry
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wave_sum = [&](long long v, int at) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][at] = (u64)v;
    };
#pragma unroll
    for (int h = 0; h < RC_HEAD; ++h) wave_sum((long long)head[h], h);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        wave_sum(nll[k], RC_HEAD + 2 * k);
        wave_sum(g[k], RC_HEAD + 2 * k + 1);
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (e < RC_HEAD + 2 * a.nb) {
        u64 v = 0ull;
#pragma unroll
        for (int wv = 0; wv < RC_T / 64; ++wv) v += part[wv][e];
        if (v) atomicAdd(tab + e, v);
    }
}

size_t rc_align(size_t b) { return (b + 255) & ~(size_t)255; }

template <int K>
void rc_launch(const Args& a, bool vec, int nb, u64* tab, hipStream_t s) {
    if (a.C <= RC_CACHE) {
        if (vec) k_recal_eval<K, true, true><<<nb, RC_T, 0, s>>>(a, tab);
        else k_recal_eval<K, true, false><<<nb, RC_T, 0, s>>>(a, tab);
    } else {
        if (vec) k_recal_eval<K, false, true><<<nb, RC_T, 0, s>>>(a, tab);
        else k_recal_eval<K, false, false><<<nb, RC_T, 0, s>>>(a, tab);
    }
}

}  // namespace

size_t recal_scratch_bytes() { return 256 + rc_align((size_t)RC_LEN * 8); }   // any scratch alignment: 256 B of slack

// every argument is checked (engine.cpp)
void launch_recal_eval(const float* logits, int C, int64_t S, const float* label, const uint8_t* mask, const float* betas, int n_betas,
                       int accumulate, int64_t* tables, void* scratch, hipStream_t s) {
    u64* tab = (u64*)rc_align((size_t)(uintptr_t)scratch);
    Args a;
    a.logits = logits; a.label = label; a.mask = mask; a.C = C; a.nb = n_betas; a.S = S;
    a.mask_vec = ((uintptr_t)mask & 3) == 0;
    for (int k = 0; k < RC_KMAX; ++k) a.beta[k] = betas[k < n_betas ? k : 0];
    // 16-B words need every plane to start 16-B aligned: S % 4 == 0 and aligned bases
    const bool vec = S % 4 == 0 && (((uintptr_t)logits | (uintptr_t)label) & 15) == 0;
    const int64_t units = (S + RC_UNIT - 1) / RC_UNIT, want = (units + RC_T - 1) / RC_T;
    const int nb = (int)(want > RC_MAXB ? RC_MAXB : want);
    k_recal_init<<<1, 64, 0, s>>>(tab);
    if (n_betas <= 1) rc_launch<1>(a, vec, nb, tab, s);
    else if (n_betas <= 2) rc_launch<2>(a, vec, nb, tab, s);
    else if (n_betas <= 4) rc_launch<4>(a, vec, nb, tab, s);
    else rc_launch<8>(a, vec, nb, tab, s);
    k_recal_finish<<<1, 64, 0, s>>>(tab, accumulate, tables);
}

}  // namespace unet
