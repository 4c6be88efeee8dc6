// Launchers of the HIP kernels (gfx950).  Every function enqueues on `stream` and returns; errors are
// reported through hipGetLastError() by the caller.  dtype: 0 fp32, 1 bf16 element type of the
// channels-last activation/gradient tensors.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/unet_atlas.h"
#include "../../include/unet_augment.h"
#include "../../include/unet_bias.h"
#include "../../include/unet_calib.h"
#include "../../include/unet_recal.h"
#include "../../include/unet_components.h"
#include "../../include/unet_connectivity.h"
#include "../../include/unet_coreg.h"
#include "../../include/unet_cowarp.h"
#include "../../include/unet_deform.h"
#include "../../include/unet_distance.h"
#include "../../include/unet_ensemble.h"
#include "../../include/unet_feed.h"
#include "../../include/unet_hip.h"
#include "../../include/unet_instances.h"
#include "../../include/unet_morph.h"
#include "../../include/unet_patches.h"
#include "../../include/unet_postproc.h"
#include "../../include/unet_preproc.h"
#include "../../include/unet_qc.h"
#include "../../include/unet_register.h"
#include "../../include/unet_space.h"
#include "../../include/unet_start.h"
#include "../../include/unet_stats.h"
#include "../../include/unet_table.h"
#include "../../include/unet_mirror.h"
#include "../../include/unet_tiles.h"
#include "../../include/unet_warp.h"

namespace unet {

// A tensor as a consumer sees it: act(x * scale[c] + shift[c]) (scale == nullptr: identity affine).
struct SrcDesc {
    const void* ptr = nullptr;
    int C = 0;
    const float* scale = nullptr;
    const float* shift = nullptr;
    int act = 0;
};
// Gradient destination of one source: written (accumulate == 0) or added to (accumulate == 1).
struct DstGrad {
    void* ptr = nullptr;  // nullptr: this source needs no gradient
    int C = 0;
    int accumulate = 0;
};

struct ConvGeom {
    int Cin = 0, Cout = 0;
    int D = 0, H = 0, W = 0;     // input volume
    int Do = 0, Ho = 0, Wo = 0;  // output volume
    int ks = 3, stride = 1;
};

__host__ __device__ static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- weight repacking (fp32 torch layout -> kernel layouts), once per parameter update ----
// conv  [Cout][Cin][k3]  -> fwd  [k3][Cin][CoutP]   and dgrad [k3][Cout][CinP]   (P = padded to 8)
void launch_pack_conv_w(const float* w, float* w_fwd, float* w_dgrad, int Cin, int Cout, int k3, hipStream_t s);
// convT [Cin][Cout][8]   -> fwd  [8][Cin][CoutP]    and dgrad [8][Cout][CinP]
void launch_pack_convt_w(const float* w, float* w_fwd, float* w_dgrad, int Cin, int Cout, hipStream_t s);

// ---- layout ----
void launch_pack_input(int dtype, const float* x_ncdhw, void* y, int C, int64_t S, hipStream_t s);
void launch_export(int dtype, SrcDesc src, float* y_ncdhw, int64_t S, hipStream_t s);                // view -> fp32 NCDHW
void launch_import_grad(int dtype, const float* g_ncdhw, void* g, int C, int64_t S, int accumulate, hipStream_t s);

// ---- direct (non-MFMA) conv family ----
// out: channels-last element type, or (out_ncdhw != nullptr) fp32 NCDHW external output
void launch_conv_fwd_direct(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const float* w_fwd, const float* bias,
                            void* out, float* out_ncdhw, hipStream_t s);
void launch_conv_dgrad_direct(int dtype, const ConvGeom& g, const void* dy, const float* w_dgrad, const DstGrad* dst, int ndst,
                              hipStream_t s);
// dw/db in torch layout, accumulated (+=).  scratch (wgrad_direct_scratch_bytes, may be nullptr) lets the kernel split
// the voxel range over more blocks (partial slabs summed in a fixed order)
size_t wgrad_direct_scratch_bytes(const ConvGeom& g, int transposed);
void launch_conv_wgrad_direct(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, float* dw, float* db,
                              void* scratch, hipStream_t s);
void launch_convt_fwd_direct(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const float* w_fwd, const float* bias,
                             void* out, hipStream_t s);
void launch_convt_dgrad_direct(int dtype, const ConvGeom& g, const void* dy, const float* w_dgrad, const DstGrad* dst, int ndst,
                               hipStream_t s);
void launch_convt_wgrad_direct(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, float* dw, float* db,
                               void* scratch, hipStream_t s);

// ---- normalisation ----
// number of partial blocks the statistics kernels use for S voxels (plan-time constant)
int stats_blocks(int64_t S);
// per-block partial {sum, sumsq} of a raw tensor: partial[blk][c][2]
// block partials: float for bf16 tensors, DOUBLE for fp32 tensors (then pass dbl = true to the finalize / sum that reads them)
void launch_stats_partial(int dtype, const void* x, int C, int64_t S, float* partial, hipStream_t s);
// partials -> stat[0..C) mean, [C..2C) rstd, [2C..3C) scale = gamma*rstd, [3C..4C) shift = beta - mean*scale;
// running stats (bnorm, may be nullptr): rm = (1-m)*rm + m*mean, rv = (1-m)*rv + m*unbiased var
void launch_norm_finalize(const float* partial, int nblk, int C, int64_t S, const float* gamma, const float* beta, double eps,
                          float* stat, float* running_mean, float* running_var, double momentum, hipStream_t s, bool dbl = false);
// partials -> out[c][2] = {sum, sum of squares}
void launch_stats_sum(const float* partial, int nblk, int C, float* out, hipStream_t s, bool dbl = false);
// eval-mode bnorm: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale (mean := rm, rstd := 1/sqrt(rv+eps))
void launch_norm_eval(int C, const float* gamma, const float* beta, const float* rm, const float* rv, double eps, float* stat,
                      hipStream_t s);
// The predicates the norm launchers and the copy launcher of kernels_elem.hip branch on.  unet_op_norm_choice (engine.cpp) reports
// from the same functions, so the query and the launches cannot disagree.
// bf16 with C/8 a power of two <= 256: the 16-B (8-channel) statistics / apply kernels of the backward (and k_colsum8)
static inline bool vec8_ok(int dtype, int C) {
    if (dtype != 1 || C % 8) return false;
    int g8 = C / 8;
    return g8 <= 256 && (g8 & (g8 - 1)) == 0;
}
constexpr int STATS8_SHUFFLE_MAX_G8 = 32;   // k_norm_bwd_stats8 / k_colsum8: shuffle reduction up to this many 8-channel groups, LDS above
// few partial rows: the finalize runs in the prologue of the element-wise pass (k_norm_finalize_apply8, k_norm_bwd_finalize_apply8)
constexpr int FUSED_MAX_ROWS = 128, FUSED_MAX_C = 512;
static inline bool fused_norm_ok(int dtype, int C, int nblk) {
    return dtype == 1 && C % 8 == 0 && C <= FUSED_MAX_C && 256 % (C / 8) == 0 && nblk <= FUSED_MAX_ROWS;
}
// threads per channel of the separate finalize kernels (k_norm_finalize, k_norm_bwd_finalize, k_stats_sum)
static inline int finalize_threads(int nblk) { return nblk > 128 ? 256 : 64; }
// the copy launch_apply_view makes: k_apply_view8g (voxel-walking, four loads in flight), k_apply_view8, or k_materialize
enum class ViewCopy { vec8g, vec8, generic };
static inline ViewCopy apply_view_form(int dtype, int C, int64_t S) {
    if (dtype == 1 && C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0 && S * C >= (1 << 18)) return ViewCopy::vec8g;
    return dtype == 1 && C % 8 == 0 ? ViewCopy::vec8 : ViewCopy::generic;
}

// ---- view backward: g holds dL/d(act(norm(u))) on entry ----
// no norm: g *= act'(u)
void launch_act_bwd(int dtype, void* g, const void* u, int act, int64_t n, hipStream_t s);
// with norm: pass 1: g <- dv = g*act'(v), partial[blk][c] = {sum dv, sum dv*xhat}
void launch_norm_bwd_partial(int dtype, void* g, const void* u, int C, int64_t S, const float* stat, int act, float* partial,
                             hipStream_t s);
// pass 2: coef[0..C) = gamma*rstd, [C..2C) = mean(dv), [2C..3C) = mean(dv*xhat); dgamma += sum dv*xhat, dbeta += sum dv
void launch_norm_bwd_finalize(const float* partial, int nblk, int C, int64_t S, const float* gamma, const float* stat, float* coef,
                              float* dgamma, float* dbeta, hipStream_t s, bool dbl = false);
// finalize + activated copy in ONE launch where the partial rows are few (bf16, <= 128 rows, C <= 512): returns false when the
// shape does not qualify (the caller then uses launch_norm_finalize + launch_apply_view)
bool launch_norm_finalize_apply(int dtype, const float* partial, int nblk, int C, int64_t S, const float* gamma, const float* beta, double eps,
                                float* stat, float* running_mean, float* running_var, double momentum, const void* raw, int act, void* out,
                                hipStream_t s);
// the same for passes 2 + 3 of the backward
bool launch_norm_bwd_finalize_apply(int dtype, const float* partial, int nblk, int C, int64_t S, const float* gamma, const float* stat,
                                    float* coef, float* dgamma, float* dbeta, void* g, const void* u, int act, hipStream_t s);
// pass 3: g <- du = coef0 * (dv - m1 - xhat*m2)
void launch_norm_bwd_apply(int dtype, void* g, const void* u, int C, int64_t S, const float* stat, const float* coef, int act,
                           hipStream_t s);

// ---- pooling / resampling / copies ----
void launch_maxpool_fwd(int dtype, SrcDesc src, void* out, int D, int H, int W, hipStream_t s);
void launch_maxpool_bwd(int dtype, SrcDesc src, const void* gout, DstGrad dst, int D, int H, int W, hipStream_t s);
void launch_upsample_fwd(int dtype, SrcDesc src, void* out, int D, int H, int W, hipStream_t s);
void launch_upsample_bwd(int dtype, const void* gout, DstGrad dst, int D, int H, int W, hipStream_t s);
void launch_materialize(int dtype, const SrcDesc* src, int nsrc, void* out, int64_t S, hipStream_t s);
// out = act(src*scale+shift) for a whole tensor (vectorised for bf16): the activated copy that consumers read
void launch_apply_view(int dtype, SrcDesc src, void* out, int64_t S, hipStream_t s);
void launch_materialize_bwd(int dtype, const void* gout, const DstGrad* dst, int ndst, int64_t S, hipStream_t s);
void launch_export_bwd(int dtype, const float* g_ncdhw, DstGrad dst, int64_t S, hipStream_t s);
void launch_unpack_ncdhw(int dtype, const void* g, float* out_ncdhw, int C, int64_t S, hipStream_t s);

// ---- losses (train.cpp:501-552, 634-706) ----
void launch_target_half(const int64_t* t, int64_t* o, int D, int H, int W, hipStream_t s);
int loss_blocks(int64_t S);
// pass 1: per-block partials [blk][3 + 2*oc]: {ce, mse, nvalid, inter[oc], card[oc]}
void launch_loss_partial(const float* logits, const int64_t* target, int C, int64_t S, int collapse, float* partial, hipStream_t s);
// pass 2: level_out[0..2] = ce, dice, mse; level_out[3 ..] = n, inter[oc], card[oc]; totals[0] += weight*(selected), totals[1..3] = stats when set_stats
void launch_loss_finalize(const float* partial, int nblk, int oc, float level_weight, int cost_mask, float* level_out, float* totals,
                          int set_stats, hipStream_t s);
// pass 3: dlogits = level_weight * d(selected losses)/dlogits
void launch_loss_grad(const float* logits, const int64_t* target, int C, int64_t S, int collapse, const float* level_out,
                      float level_weight, int cost_mask, float* dlogits, hipStream_t s);

// out = ((b0 + b1) + b2) + ... element-wise in exactly that order (n <= UNET_SUM_MAX_BUFFERS, 16-B aligned); zero_inputs clears b* (not out)
void launch_sum_buffers(const float* const* bufs, int n, float* out, int64_t count, int zero_inputs, hipStream_t s);

// ---- step epilogue ----
struct SgdSeg { int64_t offset, count; float wd; };  // wd: 1 when weight decay applies to the tensor, else 0
void launch_sumsq_partial(const float* g, int64_t n, float scale, float* partial, int nblk, hipStream_t s);
void launch_sgd(float* p, float* g, float* m, int64_t n, const SgdSeg* segs_dev, int nseg, const float* partial, int nblk,
                float lr, float momentum, int nesterov, float weight_decay, float clip_norm, float grad_scale, float* norm_out,
                hipStream_t s);

// ---- update + filter packs in one pass (kernels_sgd_pack.hip) ----
// One block's share of the flat parameter buffer.  A filter tile (job_fwd >= 0) is the sub-block [d0, d0 + n0) x [d1, d1 + n1) x T of a
// weight tensor w[D0][D1][T] at `off` (conv: Cout, Cin, 27; conv_trans: Cin, Cout, 8); n0, n1 <= 32 and both starts are multiples of 32,
// so every pack unit of the tensor's forward job and of its dgrad job (job_dgrad, -1: none) draws its values from inside one tile.
// A plain range (job_fwd < 0) is `count` elements at `off` that no pack job reads.  wd as in SgdSeg.
struct PackJob;
struct SgdTile { int64_t off, count; float wd; int job_fwd, job_dgrad, D1, T, d0, n0, d1, n1, pad; };
constexpr int SGD_TILE_MAX = 32;
// the pack units of `job` that tile `t` holds (host side: the plan checks that its tiles hold every unit of every job exactly once)
int64_t sgd_tile_units(const SgdTile& t, const PackJob& job);
// the effect of launch_sgd followed by launch_mfma_pack_batched over the jobs [0, with_dgrad ? all : the forward jobs) of the table
void launch_sgd_pack(float* p, float* g, float* m, const SgdTile* tiles_dev, int ntiles, const PackJob* jobs_dev, void* ws, int with_dgrad,
                     int* zero, int nzero, const float* partial, int nblk, float lr, float momentum, int nesterov, float weight_decay,
                     float clip_norm, float grad_scale, float* norm_out, hipStream_t s);

// ---- MFMA implicit-GEMM family (kernels_mfma_conv.hip, kernels_mfma_wgrad.hip), bf16 only ----
// one filter pack of the batched pack kernel: fp32 parameter (src_off floats from the flat parameter base) ->
// bf16 fragments at dst_off bytes into the workspace; blk0 = first 256-thread block of the job in the launch
struct PackJob { int64_t src_off, dst_off, total, blk0; int Ci, Co, CK, T, mode, A, B, pad; };
// PackJob::mode: how a pack unit (16 rows o x CK k-channels i x T taps t) draws its values from the fp32 torch-layout filter w
enum PackMode {
    PK_CONV_FWD = 0,    // rows o = cout, k-channel i = cin, T taps:           w[(o*A + i)*T + t]              A = Cin
    PK_CONV_DGRAD = 1,  // rows o = cin,  i = cout, 27 taps flipped:           w[(i*A + o)*27 + 26 - t]        A = Cin
    PK_CONVT_DGRAD = 2, // rows o = cin,  i = cout, 8 taps:                    w[(o*B + i)*8 + t]              B = Cout
    PK_CONVT_FWD = 3,   // rows o = t*B + co, i = cin, 1 tap:                  w[(i*B + co)*8 + t]             B = Cout
    PK_CONV_S2_DGRAD = 4 // rows o = p*A + ci (p = output parity), i = cout, 8 taps k in {0,1}^3 over dy[m+k]:
                        //   per dim  p=0: k=0 -> filter tap 1 ;  p=1: k=0 -> tap 2, k=1 -> tap 0 ; else zero     A = Cin
};
int mfma_conv_pack_jobs(const ConvGeom& g, bool want_dgrad, PackJob* out2);
int mfma_convt_pack_jobs(const ConvGeom& g, PackJob* out2);
// one launch serves the pack units [blk_base, blk_base + nblocks) of the table (njobs = the whole table); max_grid > 0 bounds the
// number of blocks (a block then walks several units); zero / nzero: ints the launch also clears (the deep levels' arrival counters)
void launch_mfma_pack_batched(const float* params_base, void* ws, const PackJob* jobs_dev, int njobs, int64_t nblocks, hipStream_t s,
                              int64_t blk_base = 0, int max_grid = 0, int* zero = nullptr, int nzero = 0);
bool mfma_conv_fwd_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t mfma_conv_w_bytes(const ConvGeom& g);
void launch_mfma_pack_conv_w(const float* w, void* w_mfma_fwd, void* w_mfma_dgrad, const ConvGeom& g, hipStream_t s);
// returns the number of statistics partial rows written to stats_partial ([rows][Cout][2], one per persistent block)
int launch_mfma_conv_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out,
                         float* stats_partial, hipStream_t s);
// the first conv (Cin = 1, 3x3x3 stride 1, Cout 16 or 32, plain bf16 input) on the matrix cores, filter read as fp32 torch layout;
// returns the number of statistics partial rows (<= conv_first_mfma_blocks)
bool conv_first_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
int conv_first_mfma_blocks(const ConvGeom& g);
int launch_conv_first_mfma(const ConvGeom& g, const SrcDesc* src, const float* w, const float* bias, void* out, float* stats_partial,
                           hipStream_t s);
// upper bound of that row count (tiles of the geometry): sizes the partials buffer
int mfma_conv_blocks(const ConvGeom& g);
// wgrad (+ bias grad) of a 3x3x3 conv, stride 1 or 2; dw/db fp32 torch layout, accumulated (+=); db may be nullptr
// sliding-window wgrad of the 3x3x3 stride-1 convs (kernels_mfma_wgrad_z.hip): kernel only, returns the number of slab rows
// written at `scratch` ([rows][Cout][Cin][27], then [rows][Cout] bias partials when want_bias); 0 = shape not covered
bool mfma_wgrad_z_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t mfma_wgrad_z_scratch_bytes(const ConvGeom& g, int polite = 0);
int mfma_wgrad_z_splits(const ConvGeom& g, int polite = 0);
int launch_mfma_wgrad_z(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, bool want_bias, void* scratch, hipStream_t s,
                        int polite = 0);
// dw[i] += sum over rows of slab[row][i] (n % 4 == 0), db[c] += sum of bias_slab[row][c]; fixed order, no atomics
void wgrad_reduce(const float* slab, const float* bias_slab, int nsplit, int64_t n, int Cb, float* dw, float* db, hipStream_t s);
// one launch for many layers' slabs: offsets in floats from the workspace base (slab, bias partials; bias_off < 0: none) and
// from the flat gradient buffer (dw, db)
struct WgradReduceJob { long long slab_off, bias_off, dw_off, db_off, n; int nsplit, Cb, ly, blk0, nblk, op; };
int wgrad_reduce_job_blocks(WgradReduceJob& j, int blk0);
void launch_wgrad_reduce_batched(const WgradReduceJob* jobs_dev, int job0, int njobs, int blk_base, int nblocks, const void* ws, float* gflat,
                                 hipStream_t s);
bool mfma_wgrad_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
// polite = 1 (weight-gradient launches only): the layer's gradient runs on the side stream beside the caller's stream's latency-bound small
// levels -- one 4-wave block per CU (one wave per SIMD), so that the caller's kernels always find registers and LDS.  The slab row count
// depends on it: the same value must be given to *_scratch_bytes, *_splits and the launch (engine.cpp: Plan::side_polite).
size_t mfma_wgrad_scratch_bytes(const ConvGeom& g, int polite = 0);
// defer_reduce: only the slab ([rows][n] + [rows][Cout] bias partials at `scratch`) is written; rows = *_wgrad_splits(g)
int mfma_conv_wgrad_splits(const ConvGeom& g, int polite = 0);
int mfma_convt_wgrad_splits(const ConvGeom& g);
// small volumes: the launch ADDS its result into dw / db itself (output-stationary blocks; no slab, defer_reduce is ignored)
bool mfma_conv_wgrad_direct(const ConvGeom& g);
bool mfma_convt_wgrad_direct(const ConvGeom& g);
int conv_first_wgrad_splits(const ConvGeom& g);
void launch_mfma_conv_wgrad(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, float* dw, float* db, void* scratch,
                            hipStream_t s, bool defer_reduce = false, int polite = 0);
// wgrad of layers with <= 1024 weights (Cin = 1 first conv, 6-channel heads): row-staged, HBM-bound
// 1x1x1 heads (Cout <= 8, Cin = 16 * 2^k <= 256, one plain or viewed source): forward writes results[level] (fp32 NCDHW) and/or
// the channels-last tensor; backward = dL/dW (+=), dL/db (+=) and dL/d(source view) in one pass, dy as fp32 NCDHW or channels-last
bool head_supported(const ConvGeom& g, int nsrc);
size_t head_bwd_scratch_bytes(const ConvGeom& g);
void launch_head_fwd(int dtype, const ConvGeom& g, const SrcDesc& src, const float* w, const float* bias, void* y, float* out_ncdhw,
                     hipStream_t s);
// defer_reduce: only the slab is written (scratch must stay untouched until launch_head_bwd_reduce has run on a stream ordered after `s`)
void launch_head_bwd(int dtype, const ConvGeom& g, const SrcDesc& src, const float* dy_ncdhw, const void* dy_cl, const float* w,
                     DstGrad dst, float* dw, float* db, void* scratch, hipStream_t s, bool defer_reduce = false);
void launch_head_bwd_reduce(const ConvGeom& g, float* dw, float* db, const void* scratch, hipStream_t s);
// wgrad (+ bias grad) of the first conv (Cin = 1, 3x3x3 stride 1, Cout 16 or 32, plain bf16 input) on the matrix cores
bool conv_first_wgrad_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t conv_first_wgrad_mfma_scratch_bytes(const ConvGeom& g);
// nb_fuse: dy is dL/d(activated view); the norm backward's element-wise pass (k_norm_bwd_apply8's arithmetic with the coefficients
// k_norm_bwd_finalize left) is applied as the tiles are staged -- the same bits as running that pass first, without its 3 tensor transfers
struct NormBwdFuse { const void* u; const float* stat; const float* coef; int act; };
void launch_conv_first_wgrad_mfma(const ConvGeom& g, const SrcDesc* src, const void* dy, float* dw, float* db, void* scratch, hipStream_t s,
                                  bool defer_reduce = false, const NormBwdFuse* nb_fuse = nullptr);
bool wgrad_small_supported(const ConvGeom& g, int nsrc);
size_t wgrad_small_scratch_bytes(const ConvGeom& g);
void launch_conv_wgrad_small(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, float* dw, float* db,
                             void* scratch, hipStream_t s);
// conv_trans wgrad (single source); db (optional): the bias gradient rides along (sums of dy as the kernel stages it: [rows][Cout]
// partials behind the slab, or += db itself in the direct form) -- no pass of its own over dy
bool mfma_convt_wgrad_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t mfma_convt_wgrad_scratch_bytes(const ConvGeom& g);
void launch_mfma_convt_wgrad(const ConvGeom& g, const SrcDesc* src, const void* dy, float* dw, void* scratch, hipStream_t s,
                             bool defer_reduce = false, float* db = nullptr, int polite = 0);
// vectorised per-block column sums partial[blk][C] of a bf16 [S][C] tensor; returns #blocks (0: not applicable)
int launch_colsum_partial8(int dtype, const void* x, int C, int64_t S, float* partial, hipStream_t s);
size_t bias_grad_scratch_bytes(int C, int64_t S);
void launch_bias_grad(int dtype, const void* dy, int C, int64_t S, float* db, void* scratch, hipStream_t s);
// dgrad of a 3x3x3 conv, stride 1 or 2 (g = forward geometry)
bool mfma_conv_dgrad_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t mfma_conv_dgrad_w_bytes(const ConvGeom& g);
// What a dgrad launch does about the norm backward of its destination's view.  Every family below has an *_outcome function that
// launches nothing and answers from the forward geometry, the destinations (count, channels, accumulate flags, null or not), whether a
// norm is offered and the DeepScratch sizes; its launcher decides and sizes its grid by the same function and returns what it ran, so
// a caller can know before the launch (or without one: the dry replay of a backward in parts) who finishes that norm backward.
struct DgradOutcome {
    bool served = false;     // false: the family does not take the shape, nothing was launched
    bool norm_done = false;  // the destination's whole norm backward ran in the epilogue: dL/d(raw), coef, the affine gradients
    int rows = 0;            // norm-backward partial rows (what launch_norm_bwd_partial computes) left in the partials buffer
    bool operator==(const DgradOutcome& o) const { return served == o.served && norm_done == o.norm_done && rows == o.rows; }
};
// bn (optional): the norm whose view the destination is; the kernels with a statistics epilogue then leave its rows in bn->partial
// (else the caller runs launch_norm_bwd_partial as usual).  The stride-1 kernels only for a single destination that is written, not
// accumulated.  Always served.
struct BnBwdStats { const void* u; const float* stat; float* partial; int act, C; };
DgradOutcome mfma_conv_dgrad_outcome(const ConvGeom& g, const DstGrad* dst, int ndst, bool norm);
DgradOutcome launch_mfma_conv_dgrad(const ConvGeom& g, const void* dy, const void* w_mfma_dgrad, const DstGrad* dst, int ndst, hipStream_t s,
                                    const BnBwdStats* bn = nullptr);
// kernels_mfma_s2.hip: sliding-window / LDS-DMA kernels for the contractions that cross a resolution boundary, coarse grid >= 16 wide
// (the launchers below try them first; 0 / false = shape not served, the halo-tile kernel k_mfma_conv_p runs instead).
// launch_s2_conv_fwd returns the number of statistics rows; launch_s2_conv_dgrad leaves the norm-backward partial rows in bn->partial
// when bn is given (its destination may be ACCUMULATED into: the old values and the raw tensor travel by LDS-DMA too)
int launch_s2_conv_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out, float* stats_partial,
                       hipStream_t s);
DgradOutcome s2_conv_dgrad_outcome(const ConvGeom& g, const DstGrad* dst, int ndst, bool norm);
DgradOutcome launch_s2_conv_dgrad(const ConvGeom& g, const void* dy, const void* w_s2_dgrad, const DstGrad* dst, int ndst, hipStream_t s,
                                  const BnBwdStats* bn);
int s2_conv_dgrad_rows_max();
bool launch_s2_convt_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out, hipStream_t s);
bool launch_s2_convt_dgrad(const ConvGeom& g, const void* dy, const void* w_mfma_dgrad, const DstGrad* dst, int ndst, hipStream_t s);
// kernels_mfma_s2_wgrad.hip: sliding-window weight gradient of Conv3d(k3, s2) (ks = 3: fine = the input, a concat when fine2 != nullptr,
// coarse = dy) and ConvTranspose3d(k2, s2) (ks = 2: fine = dy, coarse = the input; bias_from_a: the bias partials are sums of the fine
// tensor).  Kernel only: slab [rows][Cb][Ca][ks^3] (+ [rows][Cb or Ca] bias partials behind it) at `scratch`; returns rows, 0 = not served
int s2_wgrad_splits(int Ca, int Cb, int cD, int cH, int cW);
int launch_s2_wgrad(int ks, const void* fine, const void* fine2, int C0, int Ca, int fD, int fH, int fW, const void* coarse, int Cb, int cD, int cH,
                    int cW, bool want_bias, int bias_from_a, void* scratch, hipStream_t s, int polite);
// kernels_mfma_deep.hip: the deep levels (output grids of DEEP_MAX_VOXELS voxels or fewer): split-K implicit GEMM straight from global
// memory, finished by the block that arrives last; with nf / nb the norm layer behind (forward) or in front of (backward) the conv runs
// in that epilogue too.  The launchers below are tried first by the engine; false / !served = shape not served.  DeepScratch: fp32 partial tiles
// and the arrival counters (ints, ZERO before the first launch; every launch leaves them zero) of one workspace.
constexpr int64_t DEEP_MAX_VOXELS = 512;
struct DeepScratch { float* part = nullptr; size_t part_bytes = 0; int* cnt = nullptr; int ncnt = 0; };
struct DeepNormFwd {      // the norm + activation on the conv's output: statistics of this launch (use_running == 0) or the running ones
    const float* gamma; const float* beta; double eps; float* stat; float* rm; float* rv; double momentum; int use_running; int act;
    void* act_out;        // the activated copy [voxel][Cout] bf16
};
struct DeepNormBwd {      // the norm + activation whose view the dgrad's destination is: u = the raw tensor, stat = {mean, rstd, scale, shift}
    const void* u; const float* stat; const float* gamma; float* coef; float* dgamma; float* dbeta; int act;
};
bool deep_conv_applies(int dtype, int64_t out_voxels, int cin, int cout);
bool launch_deep_conv_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out,
                          const DeepNormFwd* nf, const DeepScratch& sc, hipStream_t s);
bool launch_deep_convt_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out,
                           const DeepScratch& sc, hipStream_t s);
// dgrad of a conv k3 or (transposed) a conv_trans k2 s2: the gradient is written / accumulated; with nb and one destination that takes
// every row, its norm backward is done in place
DgradOutcome deep_dgrad_outcome(const ConvGeom& g, bool transposed, const DstGrad* dst, int ndst, bool norm, const DeepScratch& sc);
DgradOutcome launch_deep_dgrad(const ConvGeom& g, bool transposed, const void* dy, const void* w_mfma_dgrad, const DstGrad* dst, int ndst,
                               const DeepNormBwd* nb, const DeepScratch& sc, hipStream_t s);
// ConvTranspose3d 2x2x2 stride 2: forward (1x1 GEMM + depth-to-space scatter) and dgrad (2x2x2 stride-2 conv of dL/dy)
bool mfma_convt_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t mfma_convt_w_bytes(const ConvGeom& g);
size_t mfma_convt_dgrad_w_bytes(const ConvGeom& g);
void launch_mfma_pack_convt_w(const float* w, void* w_mfma_fwd, void* w_mfma_dgrad, const ConvGeom& g, hipStream_t s);
void launch_mfma_convt_fwd(const ConvGeom& g, const SrcDesc* src, int nsrc, const void* w_mfma, const float* bias, void* out, hipStream_t s);
void launch_mfma_convt_dgrad(const ConvGeom& g, const void* dy, const void* w_mfma_dgrad, const DstGrad* dst, int ndst, hipStream_t s);

// kernels_mfma_f32.hip: fp32 3x3x3 stride-1 conv on the fp32 matrix cores (the fp32 engine with impl == AUTO)
bool conv_f32_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
// stats_partial (optional): [rows][Cout][2] fp64 {sum, sum of squares} of the output per block, rows = the return value
// (= conv_f32_mfma_stat_rows): the norm layer's statistics without a pass of its own (read them with dbl = true)
int conv_f32_mfma_stat_rows(const ConvGeom& g, const SrcDesc* src);
int launch_conv_f32_mfma(const ConvGeom& g, const SrcDesc* src, int nsrc, const float* w_fwd, const float* bias, float* out,
                         hipStream_t s, double* stats_partial = nullptr);
// the fp32 engine's first conv (Cin = 1, 3x3x3 stride 1, Cout 16 or 32, plain fp32 input) on the fp32 matrix cores, filter read in torch
// layout; stats_partial (optional): fp64 {sum, sum of squares} rows, one per block (the return value)
bool conv_first_f32_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
int conv_first_f32_mfma_blocks(const ConvGeom& g);
int launch_conv_first_f32_mfma(const ConvGeom& g, const SrcDesc* src, const float* w, const float* bias, float* out, double* stats_partial,
                               hipStream_t s);
// fp32 ConvTranspose3d(k2, s2) forward on the fp32 matrix cores (w_fwd: launch_pack_convt_w's [8][Cin][CoutP])
bool convt_f32_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
void launch_convt_f32_mfma(const ConvGeom& g, const SrcDesc* src, const float* w_fwd, const float* bias, float* out, hipStream_t s);
bool wgrad_f32_mfma_supported(int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc);
size_t wgrad_f32_mfma_scratch_bytes(const ConvGeom& g);
void launch_wgrad_f32_mfma(const ConvGeom& g, const SrcDesc* src, int nsrc, const float* dy, float* dw, float* db, void* scratch,
                           hipStream_t s);
// out[i] += sum over the nsplit slabs of slab[k][i], fixed order, fp64 (kernels_direct.hip)
void slab_reduce_public(const float* slab, int nsplit, int64_t n, float* out, hipStream_t s);
bool conv_f32_mfma_dgrad_supported(int dtype, const ConvGeom& g, const DstGrad* dst, int ndst);
void launch_conv_f32_mfma_dgrad(const ConvGeom& g, const float* dy, const float* w_dgrad, const DstGrad* dst, int ndst, hipStream_t s);

// kernels_augment.hip: on-GPU sample augmentation (include/unet_augment.h)
size_t augment_scratch_bytes(const UnetAugmentRecipe& r);
void launch_augment(const UnetAugmentRecipe& r, float* image, float* label, void* scratch, hipStream_t st);
size_t simulate_scratch_bytes(const UnetSimulateRecipe& r);
void launch_simulate_modality(const UnetSimulateRecipe& r, float* t1w, const float* label, void* scratch, hipStream_t st);

// kernels_qc.hip: per-class voxel / wrong counts of quality control (include/unet_qc.h)
size_t qc_scratch_bytes(int out_c, int64_t S, int collapse);
void launch_qc_counts(const float* logits, const float* label, const float* image0, int out_c, int64_t S, int collapse, int shift,
                      uint64_t* counts, void* scratch, hipStream_t s);

// kernels_feed.hip: label max / normalize / subject shift / int64 target of the training feed (include/unet_feed.h)
size_t feed_scratch_bytes(int64_t S);
void launch_feed_label_max(const float* label, int64_t S, int* out_max, void* scratch, hipStream_t s);
void launch_feed_prepare(const float* image0, float* label, int64_t S, int normalize, int shift, int* label_max, void* scratch,
                         hipStream_t s);
void launch_feed_target(const float* label, int64_t S, int normalize, int64_t* target, void* scratch, hipStream_t s);

// kernels_patches.hip: the per-class index of a canvas label, the pick of a window and its crop (include/unet_patches.h); K = the
// number of classes (2 for classes == 0); picks: n host entries, read before the return
int64_t patches_segments(int64_t voxels);
size_t patches_index_bytes(int64_t voxels, int K);
void launch_patches_index(const float* label, int64_t voxels, int classes, int32_t* index, hipStream_t s);
void launch_patches_pick(const float* label, const int32_t* index, int classes, int W, int H, int D, int tw, int th, int td,
                         const UnetPatchPick* picks, int n, int32_t* origins, hipStream_t s);
void launch_patches_crop(const float* image, int channels, const float* label, int W, int H, int D, int tw, int th, int td,
                         const int32_t* origin, float* x, float* lab, hipStream_t s);

// kernels_postproc.hip: the inference post-processing chain (include/unet_postproc.h)
size_t postproc_scratch_bytes(int planes, int64_t S);
void launch_postproc_softmax(const float* logits, int C, int64_t S, float thr, float* lp, float* fg, uint16_t* lab, hipStream_t s);
void launch_postproc_argmax_planes(const float* lp, int np, int64_t S, const float* fg, float thr, uint16_t* lab, hipStream_t s);
void launch_postproc_defragment(int W, int H, int D, int each, float thr, double ratio, float* fg, float* lp, int np, uint16_t* lab,
                                void* scratch, hipStream_t s);
void launch_postproc_plane_op(int op, float t, int W, int H, int D, float* lp, int np, void* scratch, hipStream_t s);

// kernels_space.hip: resampling between a scan's grid and the model's, and the fused pass on the native grid (include/unet_space.h)
int64_t space_bricks(int w, int h, int d);
size_t space_scratch_bytes(int64_t dst_voxels, int channels);
void launch_space_resample(const float* src, int sw, int sh, int sd, float* dst, int dw, int dh, int dd, int channels,
                           const UnetSpaceMap& map, int mode, int normalize, void* scratch, hipStream_t s);
void launch_space_postproc(const float* logits, int C, int mw, int mh, int md, const UnetSpaceMap& map, int nw, int nh, int nd, float thr,
                           float* lp, float* fg, uint16_t* lab, hipStream_t s);

// kernels_tiles.hip: the blend of overlapping tiles onto the canvas, alone and inside the fused pass (include/unet_tiles.h)
void launch_tiles_blend(const float* tiles, int C, int tw, int th, int td, const UnetTilePlan& plan, int cw, int ch, int cd, float* canvas,
                        hipStream_t s);
void launch_tiles_postproc(const float* tiles, int C, int tw, int th, int td, const UnetTilePlan& plan, int cw, int ch, int cd, float thr,
                           float* lp, float* fg, uint16_t* lab, hipStream_t s);

// kernels_mirror.hip: the combine of mirrored members' logits, alone and inside the fused pass (include/unet_mirror.h); the arguments
// are checked by the caller (n_members 1, 2, 4 or 8; masks and pairs in host memory)
void launch_mirror_combine(const float* stack, int C, int W, int H, int D, int n_members, const int* masks, int swap_axis, const int* pairs,
                           int n_pairs, float* mean, uint8_t* agreement, hipStream_t s);
void launch_mirror_postproc(const float* stack, int C, int W, int H, int D, int n_members, const int* masks, int swap_axis,
                            const int* pairs, int n_pairs, float thr, float* lp, float* fg, uint16_t* lab, uint8_t* agreement,
                            hipStream_t s);

// kernels_ensemble.hip: one member's probabilities folded into the running state, and the closing pass (include/unet_ensemble.h);
// the arguments are checked by the caller
size_t ens_state_bytes(int C, int64_t S);
void launch_ens_accumulate(const float* logits, int C, int64_t S, float w, int first, float* state, hipStream_t s);
void launch_ens_finalize(const float* state, int C, int64_t S, float thr, float* lp, float* fg, uint16_t* lab, float* ent, float* mi,
                         hipStream_t s);

// kernels_preproc.hip: the pre-processing commands of a model (include/unet_preproc.h); w, h, d are the source's dimensions
int64_t preproc_filter_blocks(int w, int h, int d, int channels);
size_t preproc_scratch_bytes(int64_t values);
void launch_preproc_filter(const float* src, float* dst, int w, int h, int d, int channels, int kind, int impl, hipStream_t s);
void launch_preproc_downsample(const float* src, float* dst, int w, int h, int d, int channels, hipStream_t s);
void launch_preproc_upsample(const float* src, float* dst, int w, int h, int d, int channels, hipStream_t s);
void launch_preproc_permute(const float* src, float* dst, int w, int h, int d, int channels, int op, hipStream_t s);
void launch_preproc_normalize(float* buf, int64_t values, void* scratch, hipStream_t s);

// kernels_components.hip: a model's single_component_label (include/unet_components.h); classes: sorted distinct host entries;
// connectivity: 6, 18 or 26 (include/unet_connectivity.h), here and in the launches below that take one
size_t components_scratch_bytes(int64_t S, int n_classes);
void launch_components_keep_largest(int W, int H, int D, uint16_t* label, int n_classes, const uint32_t* classes, int n,
                                    uint32_t* removed, int impl, int connectivity, void* scratch, hipStream_t s);
// the labelling stage alone (shared with kernels_instances.hip and kernels_morph.hip): parent[v] = the smallest linear index of v's component or -1,
// count[r] = the component's voxels at a root r; both live in the scratch.  end: the first byte behind what
// components_scratch_bytes covers from the scratch's 256-B aligned base (itself 256-B aligned); best: keep_largest's per-class table
struct ComponentsForest {
    int* parent;
    unsigned* count;
    char* end;
    unsigned long long* best;
};
ComponentsForest launch_components_label(int W, int H, int D, const uint16_t* label, int n_classes, const uint32_t* classes, int n,
                                         int impl, int connectivity, void* scratch, hipStream_t s);

// kernels_instances.hip: the instances of a label map (include/unet_instances.h); classes as above
size_t inst_scratch_bytes(int64_t S, int n_classes, int64_t max_instances);
void launch_inst_label(int W, int H, int D, const uint16_t* label, int n_classes, const uint32_t* classes, int n, int32_t* inst,
                       int64_t* rows, int64_t max_instances, int64_t* info, int impl, int connectivity, void* scratch, hipStream_t s);
size_t inst_match_scratch_bytes(int64_t max_pairs);
void launch_inst_match(const int32_t* ia, const int32_t* ib, int64_t voxels, unsigned long long* keys, int64_t* counts, int64_t max_pairs,
                       int64_t* info, int impl, void* scratch, hipStream_t s);
void launch_inst_remove_small(uint16_t* label, const int32_t* inst, int64_t voxels, const int64_t* rows, int64_t max_instances,
                              int64_t min_voxels, uint32_t* removed, int n_classes, hipStream_t s);

// kernels_morph.hip: binary morphology on bit-packed masks (include/unet_morph.h); a mask is uint64[D][H][ceil(W / 64)].  classes: host
// entries in (0, n_classes), read before the return; step's impl is LDS or GLOBAL, holes' labelling one of UNET_COMPONENTS_IMPL_*
size_t morph_scratch_bytes(int W, int H, int D);
void launch_morph_pack(int W, int H, int D, const void* labels, int label_bytes, int n_classes, const uint32_t* classes, int n,
                       uint64_t* bits, void* scratch, hipStream_t s);
void launch_morph_unpack(int W, int H, int D, const uint64_t* bits, uint8_t* mask, hipStream_t s);
void launch_morph_count(int W, int H, int D, const uint64_t* bits, int64_t* count, hipStream_t s);
void launch_morph_step(int W, int H, int D, const uint64_t* in, uint64_t* out, int op, int connectivity, int iterations, int border,
                       int impl, void* scratch, hipStream_t s);
void launch_morph_holes(int W, int H, int D, const uint64_t* in, uint64_t* out, int64_t* info, int labelling, int connectivity,
                        void* scratch, hipStream_t s);
void launch_morph_apply(int W, int H, int D, uint16_t* labels, const uint64_t* bits, int value, int mode, int64_t* changed, hipStream_t s);

// kernels_atlas.hip: the atlas preparation of load_atlas (include/unet_atlas.h); grow: n_tissues host flags, read before the return.
// reclassify uses the tables of the scratch only: atlas_scratch_bytes(1, R, T, 0) serves it
size_t atlas_scratch_bytes(int64_t S, int n_regions, int n_tissues, int max_rounds);
void launch_atlas_reclassify(int64_t S, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_regions, int n_tissues, int flags,
                             uint32_t* votes, uint32_t* total, uint32_t* covered, uint8_t* majority, uint32_t* erased, int impl,
                             void* scratch, hipStream_t s);
void launch_atlas_grow(int W, int H, int D, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_tissues, int flags,
                       const uint8_t* grow, int max_rounds, int smooth_rounds, uint32_t* filled, uint32_t* relabelled, uint32_t* info,
                       void* scratch, hipStream_t s);

// kernels_register.hip: the parcellation of a subject (include/unet_register.h); maps, init, step, stages, map: host arrays, read
// before the return.  Only the search uses scratch
size_t reg_scratch_bytes(int n_tissues);
void launch_reg_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                     int n_tissues, const float* maps, int K, int stride, uint32_t* hist, int impl, hipStream_t s);
void launch_reg_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                       int n_tissues, const float* init, const float* step, const int* stages, int n_stages, int max_iterations,
                       float* map_out, int64_t* trace, int64_t* info, int impl, void* scratch, hipStream_t s);
void launch_reg_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                      const uint16_t* atlas, int n_tissues, const float* map, uint16_t* out, uint32_t* counts, hipStream_t s);

// kernels_coreg.hip: the co-registration of two intensity images (include/unet_coreg.h); fixed and moving are codes; scale =
// (float)bins / (hi - lo), formed by the caller; maps, init, step, stages: host arrays, read before the return.  Only the search uses
// scratch
size_t coreg_scratch_bytes(int bins);
void launch_coreg_code(const float* image, int64_t voxels, float lo, float scale, int bins, uint8_t* codes, hipStream_t s);
void launch_coreg_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                       const float* maps, int K, int stride, uint32_t* hist, int impl, hipStream_t s);
void launch_coreg_score(const uint32_t* hist, int K, int bins, int64_t* scores, hipStream_t s);
void launch_coreg_search(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                         const float* init, const float* step, const int* stages, int n_stages, int max_iterations, float* map_out,
                         int64_t* trace, int64_t* info, int impl, void* scratch, hipStream_t s);

// kernels_start.hip: the starts of a registration (include/unet_start.h); inits and maps: device arrays; step, stages: host arrays,
// read before the return.  start_seq_scratch: the scratch of state s's own search under UNET_START_IMPL_SEQUENTIAL
size_t start_scratch_bytes(int n_tissues, int n);
void* start_seq_scratch(void* scratch, int n_tissues, int n, int s);
size_t start_seq_scratch_bytes(int n_tissues);
void launch_start_moments(const void* vol, int vbytes, int w, int h, int d, int lo, int hi, uint64_t* sums, hipStream_t s);
void launch_start_pick(const uint32_t* hist, int S, int n_tissues, const float* maps, int n, int always, int64_t* scores, float* inits,
                       int32_t* picked, hipStream_t s);
void launch_start_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                         int n_tissues, const float* inits, int n, const float* step, const int* stages, int n_stages, int max_iterations,
                         float* maps_out, int64_t* trace, int64_t* info, int32_t* best, float* best_map, void* scratch, hipStream_t s);
void launch_start_close(const int64_t* info, const float* maps_out, int n, int32_t* best, float* best_map, hipStream_t s);

// kernels_warp.hip: the non-linear refinement of a parcellation (include/unet_warp.h); map and levels (n_levels x 5): host arrays,
// read before the return.  warp_scratch_bytes: the scratch of a fit of these levels; a sweep at g uses that of the one-level list {g}
size_t warp_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels);
void launch_warp_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                      int n_tissues, const float* map, const int32_t* D, int g, uint32_t* hist, hipStream_t s);
void launch_warp_sweep(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                       int n_tissues, const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch,
                       hipStream_t s);
void launch_warp_refine(const int32_t* coarse, int sw, int sh, int sd, int g, int32_t* fine, hipStream_t s);
void launch_warp_fit(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                     int n_tissues, const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl,
                     void* scratch, hipStream_t s);
void launch_warp_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes, int tw, int th, int td,
                       const uint16_t* atlas, int n_tissues, const float* map, const int32_t* D, int g, uint16_t* out, uint32_t* counts,
                       hipStream_t s);

// kernels_cowarp.hip: the non-linear refinement of a co-registration (include/unet_cowarp.h); fixed and moving are codes; map and
// levels (n_levels x 5): host arrays, read before the return.  cowarp_scratch_bytes: the scratch of a fit of these levels; a sweep at
// g uses that of the one-level list {g}.  A fit refines with launch_warp_refine
size_t cowarp_scratch_bytes(int fw, int fh, int fd, const int* levels, int n_levels);
void launch_cowarp_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                        const float* map, const int32_t* D, int g, uint32_t* hist, hipStream_t s);
void launch_cowarp_weights(const uint32_t* hist, int bins, int16_t* weights, hipStream_t s);
void launch_cowarp_sweep(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                         const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch, hipStream_t s);
void launch_cowarp_fit(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                       const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                       hipStream_t s);
void launch_cowarp_resample(const float* moving, int mw, int mh, int md, int fw, int fh, int fd, const float* map, const int32_t* D, int g,
                            float* out, hipStream_t s);

// kernels_deform.hip: the geometry of a fitted lattice warp (include/unet_deform.h); map and inv: host arrays, read before the return;
// det, D (pull) and pos may be null
void launch_deform_jacobian(int sw, int sh, int sd, const float* map, const int32_t* D, int g, float* det, int64_t* info, hipStream_t s);
void launch_deform_pull(const void* volume, int kind, int sw, int sh, int sd, int tw, int th, int td, const float* map, const float* inv,
                        const int32_t* D, int g, int iters, void* out, float* pos, int64_t* info, int impl, hipStream_t s);

// kernels_bias.hip: the intensity-inhomogeneity correction (include/unet_bias.h); classes (K) and levels (n_levels x 3): host arrays,
// read before the return.  bias_scratch_bytes: the scratch of a fit of these levels; bias_sweep_scratch_bytes: that of one sweep at g
// (the counters of IMPL_VOXEL alone)
size_t bias_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels);
size_t bias_sweep_scratch_bytes(int sw, int sh, int sd, int g);
void launch_bias_logcode(const float* v, int64_t voxels, int32_t* q, hipStream_t s);
void launch_bias_levels(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, const int32_t* B,
                        int g, int64_t* levels_out, hipStream_t s);
void launch_bias_residual(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K,
                          const int64_t* levels_in, int clip, int16_t* r, hipStream_t s);
void launch_bias_sweep(const int16_t* r, int sw, int sh, int sd, int32_t* B, int g, int lam, int64_t* info, int impl, void* scratch,
                       hipStream_t s);
void launch_bias_refine(const int32_t* coarse, int sw, int sh, int sd, int g, int32_t* fine, hipStream_t s);
void launch_bias_cost(const int16_t* r, int sw, int sh, int sd, const int32_t* B, int g, int64_t* cost, hipStream_t s);
void launch_bias_fit(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, int clip,
                     const int* levels, int n_levels, int outer, int32_t* B_out, int64_t* report, int impl, void* scratch, hipStream_t s);
void launch_bias_apply(const float* v, int sw, int sh, int sd, const int32_t* B, int g, float* out, float* gain, hipStream_t s);

// kernels_table.hip: the tables of a label map (include/unet_table.h); the running table lives in the scratch
size_t table_scratch_bytes(int n_labels);
void launch_table_regions(const void* labels, int label_bytes, int w, int h, int d, int n_labels, int64_t* rows, int impl, void* scratch,
                          hipStream_t s);
void launch_table_overlap(const void* a, int a_bytes, const void* b, int b_bytes, int64_t voxels, int n_labels, int64_t* rows, int impl,
                          void* scratch, hipStream_t s);

// kernels_stats.hip: the per-region intensity statistics (include/unet_stats.h); labels may be null (one region, n_labels 0); scale =
// 65536.0f / (hi - lo), formed by the caller; permille: n_quantiles host ints, read before the return; the running tables live in the
// scratch
size_t stats_scratch_bytes(int n_labels, int n_quantiles);
void launch_stats_moments(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi, float scale,
                          int64_t* rows, int impl, void* scratch, hipStream_t s);
void launch_stats_hist(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi, float scale,
                       int64_t* rows, int impl, void* scratch, hipStream_t s);
void launch_stats_quantiles(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                            float scale, const int* permille, int n_quantiles, int32_t* out, int impl, void* scratch, hipStream_t s);

// kernels_calib.hip: the calibration tables (include/unet_calib.h); mask and wrong may be null; the running table lives in the scratch
size_t calib_table_len(int C);
size_t calib_scratch_bytes(int C);
void launch_calib_tables(const float* src, int src_kind, int C, int64_t S, const float* label, const uint8_t* mask, int accumulate,
                         int64_t* tables, uint8_t* wrong, int impl, void* scratch, hipStream_t s);

// kernels_recal.hip: the recalibration pass (include/unet_recal.h); mask may be null; betas: n_betas host floats, read before the
// return; the running table lives in the scratch
size_t recal_scratch_bytes();
void launch_recal_eval(const float* logits, int C, int64_t S, const float* label, const uint8_t* mask, const float* betas, int n_betas,
                       int accumulate, int64_t* tables, void* scratch, hipStream_t s);

// kernels_distance.hip: the exact squared distance transform and the surface lists (include/unet_distance.h); the volume between
// the passes lives in the scratch
size_t dist_scratch_bytes(int64_t voxels);
void launch_dist_transform(const void* labels, int label_bytes, int w, int h, int d, int label, int of, int wx, int wy, int wz, int32_t* out,
                           int impl, void* scratch, hipStream_t s);
void launch_dist_surface_counts(const void* a, int a_bytes, const void* b, int b_bytes, int w, int h, int d, int n_labels, int64_t* rows,
                                hipStream_t s);
void launch_dist_gather(const void* at, int at_bytes, int w, int h, int d, int label, const int32_t* dist, int32_t* values, int64_t capacity,
                        unsigned long long* cursor, hipStream_t s);

}  // namespace unet
