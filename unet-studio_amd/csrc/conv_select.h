// Which kernel family runs each direction of a conv / conv_trans layer.  The plan makes the choice once per layer
// (unet_plan::layout) and the single-op entry points once per call, both here; what depends on the run (the deep levels' counters, the
// statistics epilogues, the streams) is decided where the kernels are launched.
#pragma once
#include "kernels.h"

namespace unet {

// deep: the mfma path, tried first on the deep levels' split-K kernel (kernels_mfma_deep.hip) when the workspace allows it
enum class Fwd : unsigned char { deep, mfma, head, first_mfma, first_f32_mfma, f32_mfma, direct };
enum class Dgrad : unsigned char { mfma, f32_mfma, direct };
enum class Wgrad : unsigned char { first_mfma, mfma, f32_mfma, small, direct };

struct ConvChoice {
    Fwd fwd = Fwd::direct;
    Dgrad dgrad = Dgrad::direct;
    Wgrad wgrad = Wgrad::direct;
    // which filter form the forward reads: the bf16 MFMA pack, the fp32 torch-layout parameter itself, else the fp32 tap-major copy
    bool mfma_fwd() const { return fwd == Fwd::deep || fwd == Fwd::mfma; }
    bool param_fwd() const { return fwd == Fwd::head || fwd == Fwd::first_mfma || fwd == Fwd::first_f32_mfma; }
};

// src: the sources as the op reads them (channel counts; a norm + activation applied on read rules out the matrix-core kernels that take
// plain sources only).  is_head: the conv writes one of the network's results.  conv_trans has the mfma and direct families in every
// direction and the fp32 matrix-core forward.
inline ConvChoice choose_conv(int dtype, int impl, const ConvGeom& g, const SrcDesc* src, int nsrc, bool is_head, bool transposed) {
    ConvChoice c;
    if (impl != UNET_IMPL_AUTO) return c;
    if (transposed) {
        if (mfma_convt_supported(dtype, g, src, nsrc)) c.fwd = Fwd::mfma, c.dgrad = Dgrad::mfma;
        else if (convt_f32_mfma_supported(dtype, g, src, nsrc)) c.fwd = Fwd::f32_mfma;
        if (mfma_convt_wgrad_supported(dtype, g, src, nsrc)) c.wgrad = Wgrad::mfma;
        return c;
    }
    if (is_head) { if (head_supported(g, nsrc)) c.fwd = Fwd::head; }
    else if (mfma_conv_fwd_supported(dtype, g, src, nsrc))
        c.fwd = deep_conv_applies(dtype, (int64_t)g.Do * g.Ho * g.Wo, g.Cin, g.Cout) ? Fwd::deep : Fwd::mfma;
    else if (conv_first_mfma_supported(dtype, g, src, nsrc)) c.fwd = Fwd::first_mfma;
    else if (conv_first_f32_mfma_supported(dtype, g, src, nsrc)) c.fwd = Fwd::first_f32_mfma;
    else if (conv_f32_mfma_supported(dtype, g, src, nsrc)) c.fwd = Fwd::f32_mfma;

    DstGrad dst[2];
    for (int k = 0; k < nsrc; ++k) dst[k].C = src[k].C;
    if (!is_head && mfma_conv_dgrad_supported(dtype, g, src, nsrc)) c.dgrad = Dgrad::mfma;
    else if (conv_f32_mfma_dgrad_supported(dtype, g, dst, nsrc)) c.dgrad = Dgrad::f32_mfma;

    if (conv_first_wgrad_mfma_supported(dtype, g, src, nsrc)) c.wgrad = Wgrad::first_mfma;
    else if (mfma_wgrad_supported(dtype, g, src, nsrc)) c.wgrad = Wgrad::mfma;
    else if (wgrad_f32_mfma_supported(dtype, g, src, nsrc)) c.wgrad = Wgrad::f32_mfma;
    else if (wgrad_small_supported(g, nsrc)) c.wgrad = Wgrad::small;
    return c;
}

}  // namespace unet
