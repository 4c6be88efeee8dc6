// The calibration tables (include/unet_calib.h): one fused pass over the probabilities of a volume (formed from logits on the fly, or
// read), the truth label and an optional mask into one table of integer counts and sums, and an optional correct / wrong byte map.
//
//   k_calib_init    the running table in the scratch: zeros
//   k_calib_tables  grid-stride over units of CB_UNIT voxels, one unit per thread at a time.  Sweep A over the channels decides which
//                   voxels are bad (LOGITS: the online state m, s of pp_acc; PROBS: any NaN); the mask and the label decide the rest.
//                   Sweep B forms p_c once more (LOGITS: expf(x_c - m) / s, the expressions of k_ens_accumulate; PROBS: as read),
//                   follows the argmax and p_t, and sends the cls updates of class c: the consecutive valid voxels of the unit whose
//                   code falls into the same bin are one update.  The head counts, the top rows and the logh keys of the unit are
//                   merged the same way.  Up to CB_CACHE channels of the unit stay in registers between the sweeps (every index a
//                   compile-time one), beyond that they are read again (from L2: the same thread, a moment later).
//                   LDS: head, top, the cls rows of the classes below UNET_CALIB_LDS_CLASSES and the uppermost
//                   UNET_CALIB_LDS_LOG_BINS keys are updated in the block's LDS table (64-bit entries, 21 KiB) and flushed with one
//                   global update per touched entry; everything else, and every update with LDS == false, goes to the scratch
//   k_calib_finish  the running table -> int64 tables: stored, or added when accumulate
// Every atomic is an integer add: the results do not depend on the schedule.  No inline assembly.
#include "../../include/unet_calib.h"
#include "device_util.h"

namespace unet {

namespace {

constexpr int CB_T = UNET_CALIB_BLOCK_UNITS;         // threads per block, a unit each
constexpr int CB_MAXB = 512;                         // grid cap, two blocks a CU: a block's table is flushed once, so fewer, longer blocks
constexpr int CB_UNIT = UNET_CALIB_UNIT;
constexpr int CB_CACHE = UNET_CALIB_CACHE;
constexpr int CB_BINS = UNET_CALIB_BINS;
constexpr int CB_LOGB = UNET_CALIB_LOG_BINS;
constexpr int CB_LC = UNET_CALIB_LDS_CLASSES;
constexpr int CB_LL = UNET_CALIB_LDS_LOG_BINS;
constexpr int CB_TOP = 4;                            // head[4]
constexpr int CB_CLS = CB_TOP + CB_BINS * 3;         // top[20][3]
constexpr int CB_ROW = CB_BINS * 5;                  // entries of a class
constexpr int CB_LDS = CB_CLS + CB_LC * CB_ROW + CB_LL;
static_assert(CB_UNIT == 8, "a unit is two float4 per plane");
static_assert(CB_T % 64 == 0 && CB_MAXB * CB_T == UNET_CALIB_GRID_UNITS, "the header states the grid's stride");
static_assert(CB_LDS * 8 <= 64 * 1024, "the LDS table of a block");
static_assert(CB_LL <= CB_LOGB && CB_CACHE == 8, "the held keys; the cached sweeps are unrolled over 8 channels");

typedef unsigned long long u64;

enum { CB_OUT = 0, CB_SKIPPED = 1, CB_INVALID = 2, CB_BAD = 3, CB_VALID = 4 };   // a voxel of a unit; CB_OUT: behind the volume's end

struct Args {
    const float* src;
    const float* label;
    const uint8_t* mask;
    uint8_t* wrong;
    int C;
    int64_t S;
    bool mask_vec, wrong_vec;   // 4-byte aligned: a half unit is one 32-bit word
};

// the unit's values of one plane; VEC: S % 4 == 0 and the plane is 16-B aligned, so a half unit is inside the volume or behind it
template <bool VEC> __device__ __forceinline__ void cb_load(const float* __restrict__ p, int64_t i0, int n, float (&x)[CB_UNIT]) {
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * h < n) q = *(const float4*)(p + i0 + 4 * h);
            x[4 * h] = q.x; x[4 * h + 1] = q.y; x[4 * h + 2] = q.z; x[4 * h + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CB_UNIT; ++j) x[j] = j < n ? p[i0 + j] : 0.f;
    }
}

__device__ __forceinline__ unsigned cb_code(float p) {
    const float u = p * 65536.0f;                     // exact
    return u < 0.f ? 0u : u >= 65535.0f ? 65535u : (unsigned)(int)u;
}
__device__ __forceinline__ unsigned cb_bin(unsigned q) { return (q * (unsigned)CB_BINS) >> 16; }
__device__ __forceinline__ unsigned cb_key(float p) { return p <= 0.f ? 0u : p >= 1.f ? (unsigned)(CB_LOGB - 1) : __float_as_uint(p) >> 18; }

__global__ void __launch_bounds__(CB_T) k_calib_init(u64* __restrict__ tab, int n) {
    for (int i = blockIdx.x * CB_T + threadIdx.x; i < n; i += gridDim.x * CB_T) tab[i] = 0ull;
}

__global__ void __launch_bounds__(CB_T) k_calib_finish(const u64* __restrict__ tab, int n, int accumulate, int64_t* __restrict__ out) {
    for (int i = blockIdx.x * CB_T + threadIdx.x; i < n; i += gridDim.x * CB_T)
        out[i] = (accumulate ? out[i] : (int64_t)0) + (int64_t)tab[i];
}

template <bool LOGITS, bool LDS, bool CACHED, bool VEC>
__global__ void __launch_bounds__(CB_T) k_calib_tables(const Args a, u64* tab) {
    __shared__ u64 lt[LDS ? CB_LDS : 1];
    const int C = a.C;
    const int held = CB_CLS + min(C, CB_LC) * CB_ROW;   // head, top and the held classes: the same index in lt and in tab
    const int logh0 = CB_CLS + C * CB_ROW;              // logh in tab
    constexpr int key0 = CB_LOGB - CB_LL;               // the first held key, at lt[held]
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < held + CB_LL; e += CB_T) lt[e] = 0ull;
        __syncthreads();
    }
    // an update of head, top or cls (idx < logh0), and one of logh; zero adds are never sent
    auto add = [&](int idx, u64 v) {
        if (LDS && idx < held) atomicAdd(&lt[idx], v);
        else atomicAdd(tab + idx, v);
    };
    auto add_key = [&](unsigned key, u64 n) {
        if (LDS && key >= (unsigned)key0) atomicAdd(&lt[held + (int)key - key0], n);
        else atomicAdd(tab + logh0 + (int)key, n);
    };
    const int64_t S = a.S, units = (S + CB_UNIT - 1) / CB_UNIT, step = (int64_t)gridDim.x * CB_T;
    for (int64_t u = (int64_t)blockIdx.x * CB_T + threadIdx.x; u < units; u += step) {
        const int64_t i0 = u * CB_UNIT;
        const int n = (int)min((int64_t)CB_UNIT, S - i0);
        float x[CB_UNIT], m[CB_UNIT], s[CB_UNIT], sf[CB_UNIT];
        float keep[CACHED ? CB_CACHE : 1][CB_UNIT];
        bool nan[CB_UNIT];
#pragma unroll
        for (int j = 0; j < CB_UNIT; ++j) { m[j] = -INFINITY; s[j] = 0.f; sf[j] = 0.f; nan[j] = false; }
        // ---- sweep A: which voxels are bad
        auto first = [&](const float (&y)[CB_UNIT], int c) {
#pragma unroll
            for (int j = 0; j < CB_UNIT; ++j) {
                if constexpr (LOGITS) pp_acc(y[j], m[j], s[j], sf[j], c ? 1.f : 0.f);
                else nan[j] = nan[j] || y[j] != y[j];
            }
        };
        if constexpr (CACHED) {
#pragma unroll
            for (int c = 0; c < CB_CACHE; ++c)
                if (c < C) cb_load<VEC>(a.src, (int64_t)c * S + i0, n, keep[c]);
#pragma unroll
            for (int c = 0; c < CB_CACHE; ++c)
                if (c < C) first(keep[c], c);
        } else {
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                cb_load<VEC>(a.src, (int64_t)c * S + i0, n, x);
                first(x, c);
            }
        }
        // ---- the mask, the label, the bad voxels: the head counts of the unit
        float lab[CB_UNIT];
        cb_load<VEC>(a.label, i0, n, lab);
        unsigned mk[CB_UNIT];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!a.mask) {
#pragma unroll
                for (int j = 0; j < 4; ++j) mk[4 * h + j] = 1u;
            } else if (VEC && a.mask_vec) {
                const unsigned w = 4 * h < n ? *(const unsigned*)(a.mask + i0 + 4 * h) : 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) mk[4 * h + j] = (w >> (8 * j)) & 255u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) mk[4 * h + j] = 4 * h + j < n ? (unsigned)a.mask[i0 + 4 * h + j] : 0u;
            }
        }
        int kind[CB_UNIT], t[CB_UNIT];
        unsigned cnt = 0u;                               // four counts of at most 8, a nibble each: valid, bad, invalid_label, skipped
#pragma unroll
        for (int j = 0; j < CB_UNIT; ++j) {
            const float l = lab[j];
            bool bad;
            if constexpr (LOGITS) bad = !(fabsf(m[j]) < INFINITY) || s[j] != s[j];   // the rule of pp_voxels
            else bad = nan[j];
            const bool lab_ok = l > -1.0f && l < (float)C;                          // false for a NaN
            t[j] = lab_ok ? (int)l : -1;
            kind[j] = j >= n ? CB_OUT : mk[j] == 0u ? CB_SKIPPED : !lab_ok ? CB_INVALID : bad ? CB_BAD : CB_VALID;
            cnt += kind[j] == CB_VALID ? 1u : kind[j] == CB_BAD ? 1u << 4 : kind[j] == CB_INVALID ? 1u << 8 : kind[j] == CB_SKIPPED ? 1u << 12 : 0u;
        }
        unsigned valid = 0u;                             // bit j: voxel j of the unit is counted in the tables
#pragma unroll
        for (int j = 0; j < CB_UNIT; ++j) valid |= (kind[j] == CB_VALID ? 1u : 0u) << j;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (const unsigned ck = (cnt >> (4 * k)) & 15u) add(k, (u64)ck);
        // ---- sweep B: p_c, the argmax over p, p_t, the cls updates of class c
        float best[CB_UNIT], pt[CB_UNIT];
        int arg[CB_UNIT];
#pragma unroll
        for (int j = 0; j < CB_UNIT; ++j) { best[j] = 0.f; pt[j] = 0.f; arg[j] = 0; }
        auto second = [&](const float (&y)[CB_UNIT], int c) {
            float p[CB_UNIT];
            if constexpr (LOGITS) {
#pragma clang fp contract(off)
#pragma unroll
                for (int j = 0; j < CB_UNIT; ++j) {   // the expressions of ens_channel (kernels_ensemble.hip)
                    const float d = y[j] - m[j];
                    const float e = expf(d);
                    p[j] = e / s[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < CB_UNIT; ++j) p[j] = y[j];
            }
            const int base = CB_CLS + c * CB_ROW;
            int rb = -1;                              // the open run: consecutive valid voxels whose code falls into bin rb
            unsigned rn = 0u, rpos = 0u, rq = 0u, rqp = 0u;
            u64 rqq = 0ull;
            auto flush = [&]() {
                const int at = base + rb * 5;
                add(at, (u64)rn);
                if (rpos) add(at + 1, (u64)rpos);
                if (rq) {
                    add(at + 2, (u64)rq);
                    add(at + 4, rqq);
                }
                if (rqp) add(at + 3, (u64)rqp);
            };
#pragma unroll
            for (int j = 0; j < CB_UNIT; ++j) {
                if (!((valid >> j) & 1u)) continue;
                if (c == 0 || p[j] > best[j]) { best[j] = p[j]; arg[j] = c; }   // the first index wins a tie
                const bool pos = t[j] == c;
                if (pos) pt[j] = p[j];
                const unsigned q = cb_code(p[j]);
                const int b = (int)cb_bin(q);
                if (b != rb) {
                    if (rn) flush();
                    rb = b; rn = 0u; rpos = 0u; rq = 0u; rqp = 0u; rqq = 0ull;
                }
                ++rn;
                rpos += pos ? 1u : 0u;
                rq += q;                              // 8 * 65535 < 2^32
                rqp += pos ? q : 0u;
                rqq += (u64)(q * q);                  // 65535^2 < 2^32
            }
            if (rn) flush();
        };
        if constexpr (CACHED) {
#pragma unroll
            for (int c = 0; c < CB_CACHE; ++c)
                if (c < C) second(keep[c], c);
        } else {
            for (int c = 0; c < C; ++c) {
                cb_load<VEC>(a.src, (int64_t)c * S + i0, n, x);
                second(x, c);
            }
        }
        // ---- top and logh, merged over the unit as well; the byte map
        {
            int rb = -1;
            unsigned rn = 0u, rc = 0u, rq = 0u, rk = 0u, kn = 0u;
            unsigned w8[CB_UNIT];
            auto flush = [&]() {
                const int at = CB_TOP + rb * 3;
                add(at, (u64)rn);
                if (rc) add(at + 1, (u64)rc);
                if (rq) add(at + 2, (u64)rq);
            };
#pragma unroll
            for (int j = 0; j < CB_UNIT; ++j) {
                w8[j] = 0u;
                if (!((valid >> j) & 1u)) continue;
                const bool correct = arg[j] == t[j];
                w8[j] = correct ? 1u : 2u;
                const unsigned q = cb_code(best[j]);
                const int b = (int)cb_bin(q);
                if (b != rb) {
                    if (rn) flush();
                    rb = b; rn = 0u; rc = 0u; rq = 0u;
                }
                ++rn;
                rc += correct ? 1u : 0u;
                rq += q;
                const unsigned k = cb_key(pt[j]);
                if (kn && k != rk) {
                    add_key(rk, (u64)kn);
                    kn = 0u;
                }
                rk = k;
                ++kn;
            }
            if (rn) flush();
            if (kn) add_key(rk, (u64)kn);
            if (a.wrong) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (VEC && a.wrong_vec) {
                        if (4 * h < n)
                            *(unsigned*)(a.wrong + i0 + 4 * h) = w8[4 * h] | (w8[4 * h + 1] << 8) | (w8[4 * h + 2] << 16) | (w8[4 * h + 3] << 24);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (4 * h + j < n) a.wrong[i0 + 4 * h + j] = (uint8_t)w8[4 * h + j];
                    }
                }
            }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < held; e += CB_T)
            if (const u64 v = lt[e]) atomicAdd(tab + e, v);
        for (int e = threadIdx.x; e < CB_LL; e += CB_T)
            if (const u64 v = lt[held + e]) atomicAdd(tab + logh0 + key0 + e, v);
    }
}

size_t cb_align(size_t b) { return (b + 255) & ~(size_t)255; }

template <bool LOGITS, bool LDS>
void cb_launch(const Args& a, bool vec, int nb, u64* tab, hipStream_t s) {
    if (a.C <= CB_CACHE) {
        if (vec) k_calib_tables<LOGITS, LDS, true, true><<<nb, CB_T, 0, s>>>(a, tab);
        else k_calib_tables<LOGITS, LDS, true, false><<<nb, CB_T, 0, s>>>(a, tab);
    } else {
        if (vec) k_calib_tables<LOGITS, LDS, false, true><<<nb, CB_T, 0, s>>>(a, tab);
        else k_calib_tables<LOGITS, LDS, false, false><<<nb, CB_T, 0, s>>>(a, tab);
    }
}

}  // namespace

size_t calib_table_len(int C) { return (size_t)CB_CLS + (size_t)C * CB_ROW + CB_LOGB; }

size_t calib_scratch_bytes(int C) { return 256 + cb_align(calib_table_len(C) * 8); }   // any scratch alignment: 256 B of slack

// every argument is checked (engine.cpp)
void launch_calib_tables(const float* src, int src_kind, int C, int64_t S, const float* label, const uint8_t* mask, int accumulate,
                         int64_t* tables, uint8_t* wrong, int impl, void* scratch, hipStream_t s) {
    u64* tab = (u64*)cb_align((size_t)(uintptr_t)scratch);
    const int len = (int)calib_table_len(C);
    Args a;
    a.src = src; a.label = label; a.mask = mask; a.wrong = wrong; a.C = C; a.S = S;
    a.mask_vec = ((uintptr_t)mask & 3) == 0;
    a.wrong_vec = ((uintptr_t)wrong & 3) == 0;
    // 16-B words need every plane to start 16-B aligned: S % 4 == 0 and aligned bases
    const bool vec = S % 4 == 0 && (((uintptr_t)src | (uintptr_t)label) & 15) == 0;
    const int64_t units = (S + CB_UNIT - 1) / CB_UNIT, want = (units + CB_T - 1) / CB_T;
    const int nb = (int)(want > CB_MAXB ? CB_MAXB : want);
    const int tb = (len + CB_T - 1) / CB_T;
    k_calib_init<<<tb, CB_T, 0, s>>>(tab, len);
    const bool lds = impl != UNET_CALIB_IMPL_GLOBAL;   // DEFAULT: LDS
    if (src_kind == UNET_CALIB_SRC_LOGITS) {
        if (lds) cb_launch<true, true>(a, vec, nb, tab, s);
        else cb_launch<true, false>(a, vec, nb, tab, s);
    } else {
        if (lds) cb_launch<false, true>(a, vec, nb, tab, s);
        else cb_launch<false, false>(a, vec, nb, tab, s);
    }
    k_calib_finish<<<tb, CB_T, 0, s>>>(tab, len, accumulate, tables);
}

}  // namespace unet
