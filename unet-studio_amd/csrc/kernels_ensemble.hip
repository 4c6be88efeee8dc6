// The model ensemble (include/unet_ensemble.h): every member's logits become softmax probabilities and are folded, weighted, into
// a running state {C + 2, S}; a closing pass reads the state into the outputs.
//
//   k_ens_accumulate   per voxel the online state (m, s, sf) of pp_acc over the member's channels, then p_c = expf(x_c - m) / s,
//                      fg = sf / s and H = logf(s) - (sum_c e_c d_c) / s, and state = first ? w * value : state + w * value
//   k_ens_finalize     label_prob / fg_prob copied out, label from the argmax of the mean foreground planes, the entropy of the
//                      mean and the mutual information (entropy - mean member entropy, clamped at 0)
//
// Both are streaming passes in the shape of k_pp_softmax (kernels_postproc.hip): a thread owns VEC consecutive voxels, VEC = 4 with
// 16-B loads and stores when S % 4 == 0 and every pointer is 16-B aligned, VEC = 1 otherwise; the grid is capped and strides over
// the rest.  The accumulate pass needs every logit twice (once for m, s, sf, once for p_c and e_c d_c): up to ENS_CACHE channels a
// voxel's logits stay in registers between the two, beyond that they are read again (from L2: the same thread, a moment later).
// Products and adds into the state are rounded one by one (contraction off); pp_acc keeps the mode it is compiled in everywhere.
// No LDS, no atomics, no scratch.
#include "../../include/unet_ensemble.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int ENS_T = 256;
constexpr int ENS_MAXB = 2048;   // 256 CUs x 8 blocks; the threads stride over the rest
constexpr int ENS_CACHE = 8;     // channels whose logits stay in registers between the two sweeps

// state plane `plane` at voxel v: written by the first member, added to by the later ones
template <int VEC, bool FIRST>
__device__ __forceinline__ void ens_fold(float* __restrict__ state, int64_t at, float w, const float (&val)[VEC]) {
#pragma clang fp contract(off)
    float r[VEC];
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) r[j] = w * val[j];
    } else {
        ldv<VEC>(state, at, r);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float t = w * val[j];
            r[j] = r[j] + t;
        }
    }
    stv<VEC>(state, at, r);
}

// channel c's second sweep: p_c into the state, e_c * d_c into ed
template <int VEC, bool FIRST>
__device__ __forceinline__ void ens_channel(const float (&x)[VEC], const float (&m)[VEC], const float (&s)[VEC], const bool (&bad)[VEC],
                                            float (&ed)[VEC], float* __restrict__ state, int64_t at, float w) {
#pragma clang fp contract(off)
    float p[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const float d = x[j] - m[j];
        const float e = expf(d);
        p[j] = bad[j] ? NAN : e / s[j];
        const float t = e * d;
        ed[j] = ed[j] + (x[j] == -INFINITY ? 0.f : t);      // 0 * -inf: such a channel contributes 0
    }
    ens_fold<VEC, FIRST>(state, at, w, p);
}

template <int VEC, bool FIRST, bool CACHED>
__global__ void __launch_bounds__(ENS_T) k_ens_accumulate(const float* __restrict__ lg, int C, int64_t S, float w,
                                                          float* __restrict__ state) {
    const int64_t step = (int64_t)gridDim.x * ENS_T * VEC;
    for (int64_t v = ((int64_t)blockIdx.x * ENS_T + threadIdx.x) * VEC; v < S; v += step) {   // VEC == 4 only when S % 4 == 0
        float m[VEC], s[VEC], sf[VEC], ed[VEC], x[VEC];
        float keep[CACHED ? ENS_CACHE : 1][VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) { m[j] = -INFINITY; s[j] = 0.f; sf[j] = 0.f; ed[j] = 0.f; }
        if constexpr (CACHED) {                                   // C <= ENS_CACHE: every index below is a compile-time one
#pragma unroll
            for (int c = 0; c < ENS_CACHE; ++c)
                if (c < C) ldv<VEC>(lg, (int64_t)c * S + v, keep[c]);
#pragma unroll
            for (int c = 0; c < ENS_CACHE; ++c)
                if (c < C) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) pp_acc(keep[c][j], m[j], s[j], sf[j], c ? 1.f : 0.f);
                }
        } else {
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                ldv<VEC>(lg, (int64_t)c * S + v, x);
#pragma unroll
                for (int j = 0; j < VEC; ++j) pp_acc(x[j], m[j], s[j], sf[j], c ? 1.f : 0.f);
            }
        }
        bool bad[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) bad[j] = !(fabsf(m[j]) < INFINITY) || s[j] != s[j];   // the rule of pp_voxels
        if constexpr (CACHED) {
#pragma unroll
            for (int c = 0; c < ENS_CACHE; ++c)
                if (c < C) ens_channel<VEC, FIRST>(keep[c], m, s, bad, ed, state, (int64_t)c * S + v, w);
        } else {
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                ldv<VEC>(lg, (int64_t)c * S + v, x);
                ens_channel<VEC, FIRST>(x, m, s, bad, ed, state, (int64_t)c * S + v, w);
            }
        }
        float f[VEC], h[VEC];
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                f[j] = bad[j] ? NAN : sf[j] / s[j];
                const float t = ed[j] / s[j];
                h[j] = bad[j] ? NAN : logf(s[j]) - t;
            }
        }
        ens_fold<VEC, FIRST>(state, (int64_t)C * S + v, w, f);
        ens_fold<VEC, FIRST>(state, (int64_t)(C + 1) * S + v, w, h);
    }
}

// need_all: the entropy or the mutual information is wanted (plane 0 and a logarithm per plane); need_top: the label is
template <int VEC>
__global__ void __launch_bounds__(ENS_T) k_ens_finalize(const float* __restrict__ state, int C, int64_t S, float thr,
                                                        float* __restrict__ lp, float* __restrict__ fg, uint16_t* __restrict__ lab,
                                                        float* __restrict__ ent, float* __restrict__ mi) {
    const bool need_all = ent || mi, need_planes = need_all || lp || lab;
    const int64_t step = (int64_t)gridDim.x * ENS_T * VEC;
    for (int64_t v = ((int64_t)blockIdx.x * ENS_T + threadIdx.x) * VEC; v < S; v += step) {
        float q[VEC], acc[VEC], best[VEC];
        int arg[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) { acc[j] = 0.f; best[j] = 0.f; arg[j] = 1; }
        if (need_planes) {
#pragma unroll 4
            for (int c = need_all ? 0 : 1; c < C; ++c) {
                ldv<VEC>(state, (int64_t)c * S + v, q);
                if (need_all) {
#pragma clang fp contract(off)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float t = q[j] * logf(q[j]);
                        acc[j] = acc[j] + (q[j] == 0.f ? 0.f : t);   // 0 ln 0 = 0
                    }
                }
                if (c >= 1) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j)
                        if (c == 1 || q[j] > best[j]) { best[j] = q[j]; arg[j] = c; }   // the first index wins a tie
                    if (lp) stv<VEC>(lp, (int64_t)(c - 1) * S + v, q);
                }
            }
        }
        if (fg || lab) {
            float f[VEC];
            ldv<VEC>(state, (int64_t)C * S + v, f);
            if (fg) stv<VEC>(fg, v, f);
            if (lab) {
                uint16_t l[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) l[j] = f[j] > thr ? (uint16_t)arg[j] : (uint16_t)0;   // NaN > thr is false
                if constexpr (VEC == 4) *(ushort4*)(lab + v) = make_ushort4(l[0], l[1], l[2], l[3]);
                else lab[v] = l[0];
            }
        }
        if (need_all) {
            float e[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) e[j] = -acc[j];
            if (ent) stv<VEC>(ent, v, e);
            if (mi) {
                float hm[VEC], t[VEC];
                ldv<VEC>(state, (int64_t)(C + 1) * S + v, hm);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float u = e[j] - hm[j];
                    t[j] = u < 0.f ? 0.f : u;                        // NaN < 0 is false: NaN stays
                }
                stv<VEC>(mi, v, t);
            }
        }
    }
}

int ens_blocks(int64_t items) {
    const int64_t nb = (items + ENS_T - 1) / ENS_T;
    return (int)(nb > ENS_MAXB ? ENS_MAXB : nb < 1 ? 1 : nb);
}

template <int VEC>
void accumulate_v(const float* lg, int C, int64_t S, float w, int first, float* state, hipStream_t s) {
    const int nb = ens_blocks(S / VEC);
    if (C <= ENS_CACHE) {
        if (first) k_ens_accumulate<VEC, true, true><<<nb, ENS_T, 0, s>>>(lg, C, S, w, state);
        else k_ens_accumulate<VEC, false, true><<<nb, ENS_T, 0, s>>>(lg, C, S, w, state);
    } else {
        if (first) k_ens_accumulate<VEC, true, false><<<nb, ENS_T, 0, s>>>(lg, C, S, w, state);
        else k_ens_accumulate<VEC, false, false><<<nb, ENS_T, 0, s>>>(lg, C, S, w, state);
    }
}

}  // namespace

size_t ens_state_bytes(int C, int64_t S) { return (size_t)(C + 2) * (size_t)S * 4; }

// every argument is checked (engine.cpp)
void launch_ens_accumulate(const float* logits, int C, int64_t S, float w, int first, float* state, hipStream_t s) {
    // 16-B words need every plane to start 16-B aligned: S % 4 == 0 and aligned bases (launch_postproc_softmax's rule)
    const bool v4 = S % 4 == 0 && ((uintptr_t)logits | (uintptr_t)state) % 16 == 0;
    if (v4) accumulate_v<4>(logits, C, S, w, first, state, s);
    else accumulate_v<1>(logits, C, S, w, first, state, s);
}

void launch_ens_finalize(const float* state, int C, int64_t S, float thr, float* lp, float* fg, uint16_t* lab, float* ent, float* mi,
                         hipStream_t s) {
    const bool v4 = S % 4 == 0 && ((uintptr_t)state | (uintptr_t)lp | (uintptr_t)fg | (uintptr_t)ent | (uintptr_t)mi) % 16 == 0 &&
                    (uintptr_t)lab % 8 == 0;
    if (v4) k_ens_finalize<4><<<ens_blocks(S / 4), ENS_T, 0, s>>>(state, C, S, thr, lp, fg, lab, ent, mi);
    else k_ens_finalize<1><<<ens_blocks(S), ENS_T, 0, s>>>(state, C, S, thr, lp, fg, lab, ent, mi);
}

}  // namespace unet
