// What the two carries share (kernels_register.hip: through the affine map, include/unet_register.h; kernels_warp.hip: through the
// map and a lattice field, include/unet_warp.h): a tissue as read, the index of a position, and the choice of one subject voxel's
// atlas value once its position is known.  Device code only, all inlined.
#pragma once
#include <stdint.h>

#include "affine_search.h"

namespace unet {

// a tissue as read: uint8 or uint16 at any alignment; a value >= T reads as 0
__device__ __forceinline__ unsigned reg_tissue(const void* __restrict__ p, int bytes, int64_t i, int T) {
    const unsigned v = bytes == 1 ? (unsigned)((const uint8_t*)p)[i]
                                  : (unsigned)((const uint8_t*)p)[2 * i] | ((unsigned)((const uint8_t*)p)[2 * i + 1] << 8);
    return v >= (unsigned)T ? 0u : v;
}

// floorf(q) as an index along an axis of `dim` voxels; below -2, above dim + 1 or NaN reads as -2: no cube voxel is inside there
__device__ __forceinline__ int reg_index(float q, int dim) {
    const float f = floorf(q);
    return f >= -2.f && f <= (float)(dim + 1) ? (int)f : -2;
}

// The atlas value of a subject voxel of tissue a != 0 whose position + 0.5 is p: the centre, or the mode of the eligible voxels of
// the 3x3x3 cube around the nearest index.  Returns the kind (0 direct, 1 rescued, 2 left) and the value in `result`
__device__ __forceinline__ unsigned reg_carry_at(const AffPos& p, unsigned a, const void* __restrict__ tmpl, int tbytes, int tw, int th, int td,
                                                 const uint16_t* __restrict__ atlas, int T, unsigned& result) {
    const int ix = reg_index(p.qx, tw), iy = reg_index(p.qy, th), iz = reg_index(p.qz, td);
    unsigned kind = 2u;   // left
    result = 0u;
    if (p.in) {
        const int o = (iz * th + iy) * tw + ix;
        const unsigned v = atlas[o];
        if (v && reg_tissue(tmpl, tbytes, o, T) == a) { result = v; kind = 0u; }   // direct
    }
    if (kind) {
        unsigned lab[27];
#pragma unroll
        for (int n = 0; n < 27; ++n) {
            const int xx = ix + n % 3 - 1, yy = iy + (n / 3) % 3 - 1, zz = iz + n / 9 - 1;
            const bool ok = xx >= 0 && xx < tw && yy >= 0 && yy < th && zz >= 0 && zz < td;
            const int o = ok ? (zz * th + yy) * tw + xx : 0;
            const unsigned v = atlas[o];
            lab[n] = ok && v && reg_tissue(tmpl, tbytes, o, T) == a ? v : 0u;
        }
        // the most frequent non-zero entry, the smallest among equal counts
        unsigned best = 0u, best_n = 0u;
#pragma unroll
        for (int j = 0; j < 27; ++j) {
            unsigned n = 0u;
#pragma unroll
            for (int k = 0; k < 27; ++k) n += lab[k] == lab[j] ? 1u : 0u;
            if (lab[j] && (n > best_n || (n == best_n && lab[j] < best))) { best_n = n; best = lab[j]; }
        }
        if (best) { result = best; kind = 1u; }   // rescued
    }
    return kind;
}

}  // namespace unet
