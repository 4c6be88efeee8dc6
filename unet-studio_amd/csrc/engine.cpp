// Plan + executor + C ABI (include/unet_hip.h).  The plan is immutable after creation; every call
// works on caller-owned device memory (parameters, gradients, workspace) and a caller-owned stream,
// so concurrent calls on one plan are safe when they use different workspaces (qc.cpp:273-297).
// What a call has to remember between its launches (which gradient buffers hold a value, which dgrad
// epilogue left or finished a norm backward) lives in the call: a backward issued in parts rebuilds it
// from the graph and the launchers' outcome queries (kernels.h: DgradOutcome), never from an earlier call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <mutex>
#include <random>
#include <unordered_map>
#include <vector>

#include "../../include/unet_hip.h"
#include "conv_select.h"
#include "graph.hpp"
#include "kernels.h"

using namespace unet;

namespace {

thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return 1; }

#define HIP_OK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        HIP_OK(hipGetDevice(&prev));
        if (prev != dev) HIP_OK(hipSetDevice(dev));
        else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// f(stream) with the device that owns `any` current: how every call on caller-owned device pointers that has no plan reaches its
// launcher.  What f throws and a failed launch become the call's error (0 or 1, as the C ABI returns)
int run_on_device_of(const void* any, void* stream, const std::function<void(hipStream_t)>& f) {
    try {
        {
            hipPointerAttribute_t at;
            HIP_OK(hipPointerGetAttributes(&at, any));
            DeviceGuard guard(at.device);
            f((hipStream_t)stream);
        }
        HIP_OK(hipGetLastError());
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// the switches of DESIGN.md §9 that this file reads, once per process.  UNET_OP_POLITE: unet_op_conv3d_bwd_weight launches as the engine's
// side stream does (one 4-wave block per CU, single (ca, cb) pairs), for micro-benchmarks and counters of the kernel as the step runs it
struct EnvSwitches {
    bool no_side_stream = getenv("UNET_NO_SIDE_STREAM"), no_first_wgrad_fuse = getenv("UNET_NO_FIRST_WGRAD_FUSE"), op_polite = getenv("UNET_OP_POLITE");
};
const EnvSwitches& env() { static const EnvSwitches e; return e; }

// ---- per-op timing (unet_profile_begin / unet_profile_end) ----
// While a host thread has a profile open, every forward / backward it issues runs on the caller's stream alone (no side
// stream) and each op's launches are bracketed by a pair of HIP events on that stream, tagged (op index, category).
struct ProfRec { int op, cat; hipEvent_t e0, e1; };
struct ProfSink { std::vector<ProfRec> recs; };
thread_local ProfSink* g_prof = nullptr;
struct ProfScope {
    ProfRec r{};
    hipStream_t s = nullptr;
    bool on = false;
    ProfScope(int op, int cat, hipStream_t st) {
        if (!g_prof) return;
        on = true; s = st; r.op = op; r.cat = cat;
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(r.e0, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.e1, s);
        g_prof->recs.push_back(r);
    }
};

}  // namespace

struct unet_plan {
    Graph g;
    int dtype = 0, device = 0, impl = 0;
    size_t elsize = 4;
    // workspace layout (byte offsets)
    std::vector<size_t> t_off, g_off;        // tensor storage / gradient storage (SIZE_MAX: none)
    std::vector<size_t> a_off;               // activated copy act(norm(tensor)) that consumers read (SIZE_MAX: none)
    std::vector<size_t> n_stat, n_coef;      // per norm: 4C / 3C floats
    std::vector<size_t> w_fwd, w_dgrad;      // per op (conv / conv_trans): packed fp32 weights
    std::vector<size_t> wm_fwd, wm_dgrad;    // per op: MFMA fragment-order bf16 filters (SIZE_MAX: op not on the MFMA path)
    std::vector<int> n_consumers;            // per tensor: ops that read it
    // per tensor: lowest op index that reads it (-1: none) -- in the backward its LAST gradient writer, the only dgrad that is offered the
    // tensor's norm (Exec::backward: its epilogue may leave that norm backward's partial rows in partial(), or run all of it)
    std::vector<int> first_consumer;
    std::vector<ConvChoice> conv;            // per op: the kernel family of each direction (conv / conv_trans; conv_select.h)
    size_t wgrad_off = 0;
    // sliding-window wgrads keep their slabs until ONE batched reduce per backward (part): per-op slab regions + the job table
    std::vector<size_t> wz_off;              // per op: slab region (SIZE_MAX: op does not use k_mfma_wgrad_z)
    std::vector<int> wz_job_of_op;           // per op: index into wz_jobs or -1
    std::vector<WgradReduceJob> wz_jobs;     // ascending op index
    WgradReduceJob* wz_jobs_dev = nullptr;
    size_t partial_off = 0, partial_bytes = 0;
    size_t ws_bytes = 0;
    // loss scratch layout
    size_t loss_bytes = 0;
    // batched MFMA filter pack (used when the caller's parameters are one flat contiguous buffer)
    std::vector<int64_t> p_off;              // element offset of parameter i in a flat buffer
    std::vector<PackJob> pack_jobs;
    int64_t pack_blocks = 0;
    PackJob* jobs_dev = nullptr;
    // update tiles of unet_sgd_step_packed (kernels_sgd_pack.hip): a partition of the flat parameter buffer in which every pack unit of
    // pack_jobs lies inside one tile; empty when there is no batched pack (then that entry point runs the plain update)
    std::vector<SgdTile> sgd_tiles;
    SgdTile* tiles_dev = nullptr;
    // sgd
    SgdSeg* segs_dev = nullptr;
    int nseg = 0;
    int64_t n_param_elems = 0;

    // backward side stream: the parameter-gradient kernels (wgrad, its reduce, bias grad) of a layer run beside the
    // dgrad -> norm-backward chain of the next one (they only share read-only inputs); forked / joined with events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pack = nullptr, ev_packd = nullptr;
    // the training forward packs the filters in three launches on the side stream.  The job table holds every op's FORWARD pack first
    // (op order), then every DGRAD pack: [0, pack_split_blocks) = forward packs of the ops before pack_split_op (the encoder's top
    // levels: a few hundred KB), [pack_split_blocks, pack_fwd_blocks) = the other forward packs (the deep levels and the decoder; only
    // awaited by the first op that reads one of them, ~0.3 ms into the forward), [pack_fwd_blocks, pack_blocks) = the dgrad packs (half
    // of the bytes): nothing reads them before the backward, which waits for ev_packd.  An inference forward packs [0, pack_fwd_blocks) only.
    int pack_split_op = 0;
    int64_t pack_split_blocks = 0, pack_fwd_blocks = 0;
    size_t head_off = 0;                     // scratch of the fused head backward (stays on the main stream)
    // the deep levels' split-K kernels (kernels_mfma_deep.hip): fp32 partial tiles + arrival counters, used on the caller's stream only
    size_t deep_part_off = 0, deep_part_bytes = 0, deep_cnt_off = 0;
    static constexpr int deep_ncnt = 4096;
    std::vector<size_t> head_op_off;         // per op: a head's own slab region (its reduce runs on the side stream, later) or SIZE_MAX

    ~unet_plan() {
        if (segs_dev) (void)hipFree(segs_dev);
        if (wz_jobs_dev) (void)hipFree(wz_jobs_dev);
        if (jobs_dev) (void)hipFree(jobs_dev);
        if (tiles_dev) (void)hipFree(tiles_dev);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_pack) (void)hipEventDestroy(ev_pack);
        if (ev_packd) (void)hipEventDestroy(ev_packd);
        if (side) (void)hipStreamDestroy(side);
    }

    ConvGeom op_geom_of(const Op& op) const {
        const Tensor& a = g.tensors[op.src[0]];
        const Tensor& o = g.tensors[op.dst];
        ConvGeom cg;
        cg.Cin = op.cin; cg.Cout = op.cout; cg.D = a.D; cg.H = a.H; cg.W = a.W; cg.Do = o.D; cg.Ho = o.H; cg.Wo = o.W;
        cg.ks = op.ks; cg.stride = op.stride;
        return cg;
    }
    // the sources by their channel counts: what the kernel choice and the scratch sizes read
    void src_chans(const Op& op, SrcDesc* sd) const {
        for (int k = 0; k < op.nsrc; ++k) sd[k].C = g.tensors[op.src[k]].C;
    }
    // the pointers of the caller's parameters (or their gradients) form one flat buffer in parameter order: both hosts allocate them
    // so, and the batched launches (filter packs, slab reduce) address everything from ptrs[0]
    bool is_flat(const float* const* ptrs) const {
        for (size_t i = 0; i < g.params.size(); ++i)
            if (ptrs[i] != ptrs[0] + p_off[i]) return false;
        return true;
    }
    // Which weight-gradient launches are "polite" (one 4-wave block per CU: mfma_util.h polite_lds): every one that runs on the side
    // stream.  The backward walks the ops from the last to the first -- the decoder's top levels (their gradients are HELD, see
    // backward()), then the small levels, then the encoder's top levels; polite launches for the tail of the step as well measured as
    // fast or faster than giving those the whole chip (profiles/r10e_ab_polite_policy.txt: 2.915-2.93 vs 2.94 ms).
    std::vector<int> side_polite;
    // Weight gradients that run on the CALLER's stream (full occupancy, slab summed there too): the stride-2 convs above 32^3 (the top of
    // the encoder).  Such a kernel becomes ready together with its own dgrad at the tail of the backward, where nothing latency-bound is
    // left to hide it behind, and the two side by side took longer than one after the other (154 us against 55 + 49: both stream the same
    // 64-MB tensors through the same L2s; profiles/r10h_ab_tail_on_main.txt: step 2.92 -> 2.88 ms; the stride-1 layer after it loses 0.03 ms).
    std::vector<char> wgrad_on_main;
    void choose_polite() {
        side_polite.assign(g.ops.size(), 0);
        wgrad_on_main.assign(g.ops.size(), 0);
        bool first = true, any_deep = false;
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind != OP_CONV && op.kind != OP_CONVT) continue;
            if (g.tensors[op.dst].voxels() <= (int64_t)32 * 32 * 32) { any_deep = true; break; }
            if (!first && op.kind == OP_CONV && op.stride == 2) wgrad_on_main[i] = 1;
            first = false;
        }
        if (!any_deep) return;      // a network without small levels has nothing latency-bound to be polite to
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind == OP_CONV || op.kind == OP_CONVT) side_polite[i] = wgrad_on_main[i] ? 0 : 1;
        }
    }

    // tensor t is read by fused heads only (bf16): see layout()
    bool head_only(size_t t) const {
        if (dtype != UNET_DTYPE_BF16 || g.tensors[t].norm < 0 || g.tensors[t].C % 16) return false;
        int readers = 0;
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind == OP_NORM) continue;
            for (int k = 0; k < op.nsrc; ++k) {
                if (op.src[k] != (int)t) continue;
                if (conv[i].fwd != Fwd::head) return false;
                ++readers;
            }
        }
        return readers > 0;
    }
    void layout() {
        choose_polite();
        // The kernel of every direction of every conv / conv_trans.  The sources are described by their channel counts alone: in the AUTO
        // engine a consumer reads a tensor with a norm or an activation through its activated copy (a_off below), except a tensor that
        // only fused heads read, and a head's choice does not depend on its source.
        conv.assign(g.ops.size(), ConvChoice());
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind != OP_CONV && op.kind != OP_CONVT) continue;
            SrcDesc sd[2];
            src_chans(op, sd);
            conv[i] = choose_conv(dtype, impl, op_geom_of(op), sd, op.nsrc, op.out_level >= 0, op.kind == OP_CONVT);
        }
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
        t_off.assign(g.tensors.size(), SIZE_MAX);
        g_off.assign(g.tensors.size(), SIZE_MAX);
        n_consumers.assign(g.tensors.size(), 0);
        first_consumer.assign(g.tensors.size(), -1);
        for (size_t oi = 0; oi < g.ops.size(); ++oi) {
            const Op& op = g.ops[oi];
            for (int k = 0; k < op.nsrc && op.kind != OP_NORM; ++k)     // (a norm op names the tensor it normalises: not a reader of the view)
                if (op.src[k] >= 0) { ++n_consumers[op.src[k]]; if (first_consumer[op.src[k]] < 0) first_consumer[op.src[k]] = (int)oi; }
        }
        a_off.assign(g.tensors.size(), SIZE_MAX);
        for (size_t i = 0; i < g.tensors.size(); ++i) {
            t_off[i] = take((size_t)g.tensors[i].numel() * elsize);
            if (g.tensors[i].needs_grad) g_off[i] = take((size_t)g.tensors[i].numel() * elsize);
            // Activated copy act(norm(u)): one extra write + the consumers read it as is.  Measured on the 32->16 conv at
            // 128^3: transforming in the conv's staging loop costs +85 % of the kernel (VALU-bound, repeated for the
            // 2.5x halo re-reads), the separate 2-pass copy ~0.03 ms.  288 GB of HBM makes the extra tensor free.
            // ... except for a tensor whose only readers are fused heads (the decoder's last tensor at full resolution): the head kernels are
            // bandwidth-bound element-wise passes that transform as they load, so the copy (read + write of 64 MB at 128^3) is never made.
            if (impl == UNET_IMPL_AUTO && (g.tensors[i].norm >= 0 || g.tensors[i].act != ACT_NONE) && !head_only(i))
                a_off[i] = take((size_t)g.tensors[i].numel() * elsize);
        }
        n_stat.resize(g.norms.size()); n_coef.resize(g.norms.size());
        size_t pmax = 0;
        for (size_t i = 0; i < g.norms.size(); ++i) {
            n_stat[i] = take(4 * (size_t)g.norms[i].C * 4);
            n_coef[i] = take(3 * (size_t)g.norms[i].C * 4);
            size_t pb = (size_t)stats_blocks(g.tensors[g.norms[i].tensor].voxels()) * g.norms[i].C * 2 * (dtype == UNET_DTYPE_F32 ? 8 : 4);
            if (pb > pmax) pmax = pb;
        }
        w_fwd.assign(g.ops.size(), SIZE_MAX); w_dgrad.assign(g.ops.size(), SIZE_MAX);
        wm_fwd.assign(g.ops.size(), SIZE_MAX); wm_dgrad.assign(g.ops.size(), SIZE_MAX);
        auto grow = [](size_t& m, size_t b) { if (b > m) m = b; };
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind != OP_CONV && op.kind != OP_CONVT) continue;
            const ConvChoice& c = conv[i];
            const ConvGeom cg = op_geom_of(op);
            int k3 = op.kind == OP_CONV ? op.ks * op.ks * op.ks : 8;
            w_fwd[i] = take((size_t)k3 * op.cin * round_up(op.cout, 8) * 4);
            w_dgrad[i] = take((size_t)k3 * op.cout * round_up(op.cin, 8) * 4);
            if (op.kind == OP_CONVT) {
                if (c.mfma_fwd()) { wm_fwd[i] = take(mfma_convt_w_bytes(cg)); wm_dgrad[i] = take(mfma_convt_dgrad_w_bytes(cg)); }
                continue;
            }
            const bool stats = g.tensors[op.dst].norm >= 0;   // statistics partial rows of the forward's epilogue
            SrcDesc sd[2];
            src_chans(op, sd);
            if (c.mfma_fwd()) {
                wm_fwd[i] = take(mfma_conv_w_bytes(cg));
                if (stats) grow(pmax, (size_t)mfma_conv_blocks(cg) * op.cout * 2 * 4);
            }
            if (c.fwd == Fwd::first_f32_mfma && stats) grow(pmax, (size_t)conv_first_f32_mfma_blocks(cg) * op.cout * 2 * 8);
            if (c.fwd == Fwd::f32_mfma && stats) grow(pmax, (size_t)conv_f32_mfma_stat_rows(cg, sd) * op.cout * 2 * 8);   // fp64 rows
            if (c.dgrad == Dgrad::mfma) {
                wm_dgrad[i] = take(mfma_conv_dgrad_w_bytes(cg));
                // norm-backward partial rows of the stride-2 dgrad's epilogue (kernels_mfma_s2.hip)
                if (op.stride == 2) grow(pmax, (size_t)s2_conv_dgrad_rows_max() * op.cin * 2 * 4);
            }
        }
        partial_bytes = pmax ? pmax : 256;
        partial_off = take(partial_bytes);
        // weight gradients: one shared slab scratch (ops run one after another on the stream)
        size_t wmax = 0, hmax = 0;
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            if (op.kind != OP_CONV && op.kind != OP_CONVT) continue;
            const ConvChoice& c = conv[i];
            const ConvGeom cg = op_geom_of(op);
            grow(wmax, wgrad_direct_scratch_bytes(cg, op.kind == OP_CONVT));   // (for every layer, whichever kernel it runs)
            if (op.kind == OP_CONVT) {
                if (c.wgrad == Wgrad::mfma) {
                    grow(wmax, mfma_convt_wgrad_scratch_bytes(cg));
                    grow(wmax, bias_grad_scratch_bytes(cg.Cout, (int64_t)cg.Do * cg.Ho * cg.Wo));
                }
                continue;
            }
            if (c.wgrad == Wgrad::mfma) grow(wmax, mfma_wgrad_scratch_bytes(cg, side_polite[i]));
            if (c.wgrad == Wgrad::f32_mfma) grow(wmax, wgrad_f32_mfma_scratch_bytes(cg));
            if (wgrad_small_supported(cg, op.nsrc)) grow(wmax, wgrad_small_scratch_bytes(cg));   // (also where another kernel runs)
            if (cg.Cin == 1 && (cg.Cout == 16 || cg.Cout == 32)) grow(wmax, conv_first_wgrad_mfma_scratch_bytes(cg));   // (at any dtype)
            if (head_supported(cg, op.nsrc)) grow(hmax, head_bwd_scratch_bytes(cg));   // (also for a conv that is no head)
        }
        wgrad_off = take(wmax ? wmax : 256);
        head_off = take(hmax ? hmax : 256);
        if (dtype == UNET_DTYPE_BF16 && impl == UNET_IMPL_AUTO) {
            deep_part_bytes = (size_t)8 << 20;
            deep_part_off = take(deep_part_bytes);
            deep_cnt_off = take((size_t)deep_ncnt * 4);
        }
        head_op_off.assign(g.ops.size(), SIZE_MAX);
        for (size_t i = 0; i < g.ops.size(); ++i)
            if (conv[i].fwd == Fwd::head) head_op_off[i] = take(head_bwd_scratch_bytes(op_geom_of(g.ops[i])));
        // every matrix-core weight gradient keeps a slab region of its own until the batched reduce of the backward (part)
        wz_off.assign(g.ops.size(), SIZE_MAX);
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            const Wgrad w = conv[i].wgrad;
            if (op.out_level >= 0 || (w != Wgrad::first_mfma && w != Wgrad::mfma)) continue;
            const ConvGeom cg = op_geom_of(op);
            if (w == Wgrad::first_mfma) wz_off[i] = take(conv_first_wgrad_mfma_scratch_bytes(cg));
            else if (op.kind == OP_CONV) { if (!mfma_conv_wgrad_direct(cg)) wz_off[i] = take(mfma_wgrad_scratch_bytes(cg, side_polite[i])); }
            else if (!mfma_convt_wgrad_direct(cg)) wz_off[i] = take(mfma_convt_wgrad_scratch_bytes(cg));
        }
        ws_bytes = off;
        // batched filter pack: one job per MFMA filter pack, sources as offsets into a flat parameter buffer
        p_off.assign(g.params.size() + 1, 0);
        for (size_t i = 0; i < g.params.size(); ++i) {
            int64_t n = 1;
            for (auto d : g.params[i].shape) n *= d;
            p_off[i + 1] = p_off[i] + n;
        }
        wz_jobs.clear();
        wz_job_of_op.assign(g.ops.size(), -1);
        int wz_blk = 0;
        for (size_t i = 0; i < g.ops.size(); ++i) {
            if (wz_off[i] == SIZE_MAX) continue;
            const Op& op = g.ops[i];
            ConvGeom cg = op_geom_of(op);
            WgradReduceJob j;
            j.op = (int)i;
            j.slab_off = (long long)(wz_off[i] / 4);
            j.dw_off = p_off[op.weight];
            j.Cb = op.cout;
            if (op.kind == OP_CONVT) {   // the bias partials (sums of dy over the fine grid) sit behind the slab, [nsplit][Cout]
                j.nsplit = mfma_convt_wgrad_splits(cg);
                j.n = (long long)8 * op.cin * op.cout;
                j.bias_off = op.bias >= 0 ? j.slab_off + (long long)j.nsplit * j.n : -1;
                j.db_off = op.bias >= 0 ? p_off[op.bias] : -1;
            } else {
                j.nsplit = conv[i].wgrad == Wgrad::first_mfma ? conv_first_wgrad_splits(cg) : mfma_conv_wgrad_splits(cg, side_polite[i]);
                j.n = (long long)27 * op.cin * op.cout;
                j.bias_off = op.bias >= 0 ? j.slab_off + (long long)j.nsplit * j.n : -1;
                j.db_off = op.bias >= 0 ? p_off[op.bias] : -1;
            }
            wz_blk += wgrad_reduce_job_blocks(j, wz_blk);
            wz_job_of_op[i] = (int)wz_jobs.size();
            wz_jobs.push_back(j);
        }
        pack_jobs.clear();
        pack_blocks = 0;
        pack_split_op = -1; pack_split_blocks = 0; pack_fwd_blocks = 0;
        for (int which = 0; which < 2; ++which) {          // forward packs first, then the dgrad packs
            for (size_t i = 0; i < g.ops.size(); ++i) {
                const Op& op = g.ops[i];
                if (!conv[i].mfma_fwd()) continue;
                // first matrix-core op whose output is 16^3 voxels or smaller: its forward pack and the later ops' go into the second launch
                if (which == 0 && pack_split_op < 0 && g.tensors[op.dst].voxels() <= (int64_t)16 * 16 * 16) { pack_split_op = (int)i; pack_split_blocks = pack_blocks; }
                PackJob jb[2];
                int n = op.kind == OP_CONV ? mfma_conv_pack_jobs(op_geom_of(op), conv[i].dgrad == Dgrad::mfma, jb) : mfma_convt_pack_jobs(op_geom_of(op), jb);
                if (which >= n) continue;
                jb[which].src_off = p_off[op.weight];
                jb[which].dst_off = (int64_t)(which == 0 ? wm_fwd[i] : wm_dgrad[i]);
                jb[which].blk0 = pack_blocks;
                pack_blocks += jb[which].total;
                pack_jobs.push_back(jb[which]);
            }
            if (which == 0) pack_fwd_blocks = pack_blocks;
        }
        build_sgd_tiles();
    }

    // The tile table is derived from pack_jobs (job indices, not copies of their offsets), next to it: filter tiles of up to 32 x 32
    // channels x all taps for every weight with pack jobs, plain ranges for everything else.  Largest first: the launch has one block
    // per tile, so the short ones fill the tail.
    void build_sgd_tiles() {
        sgd_tiles.clear();
        if (pack_jobs.empty()) return;
        const size_t np = g.params.size();
        std::vector<int> jf(np, -1), jd(np, -1), d0(np, 0), d1(np, 0), taps(np, 0);
        {
            size_t j = 0;
            for (int which = 0; which < 2; ++which)
                for (size_t i = 0; i < g.ops.size(); ++i) {
                    const Op& op = g.ops[i];
                    if (!conv[i].mfma_fwd()) continue;
                    const bool convt = op.kind != OP_CONV;
                    if (which >= (convt ? 2 : (conv[i].dgrad == Dgrad::mfma ? 2 : 1))) continue;
                    const ConvGeom cg = op_geom_of(op);
                    int& slot = which == 0 ? jf[op.weight] : jd[op.weight];
                    if (j >= pack_jobs.size() || pack_jobs[j].src_off != p_off[op.weight] || slot >= 0) return;   // (a weight two ops share: no table)
                    slot = (int)j++;
                    d0[op.weight] = convt ? cg.Cin : cg.Cout; d1[op.weight] = convt ? cg.Cout : cg.Cin; taps[op.weight] = convt ? 8 : 27;
                }
            if (j != pack_jobs.size()) return;
        }
        std::vector<int64_t> units(pack_jobs.size(), 0);
        bool ok = true;
        for (size_t i = 0; i < np && ok; ++i) {
            SgdTile t{};
            t.wd = g.params[i].decay ? 1.f : 0.f;
            t.job_fwd = jf[i]; t.job_dgrad = jd[i];
            const int64_t n = p_off[i + 1] - p_off[i];
            if (jf[i] < 0) {
                if (jd[i] >= 0) { ok = false; break; }
                constexpr int64_t chunk = 8192;
                for (int64_t o = 0; o < n; o += chunk) { t.off = p_off[i] + o; t.count = std::min(chunk, n - o); sgd_tiles.push_back(t); }
                continue;
            }
            if ((int64_t)d0[i] * d1[i] * taps[i] != n) { ok = false; break; }
            t.off = p_off[i]; t.D1 = d1[i]; t.T = taps[i];
            for (int a = 0; a < d0[i] && ok; a += SGD_TILE_MAX)
                for (int b = 0; b < d1[i] && ok; b += SGD_TILE_MAX) {
                    t.d0 = a; t.n0 = std::min(SGD_TILE_MAX, d0[i] - a); t.d1 = b; t.n1 = std::min(SGD_TILE_MAX, d1[i] - b);
                    t.count = (int64_t)t.n0 * t.n1 * t.T;
                    for (int j : {jf[i], jd[i]}) {
                        if (j < 0) continue;
                        const int64_t u = sgd_tile_units(t, pack_jobs[j]);
                        if (u < 0) ok = false; else units[j] += u;
                    }
                    sgd_tiles.push_back(t);
                }
        }
        // every unit of every job exactly once (the tiles of a tensor are disjoint): else the forward would read fragments nobody wrote
        for (size_t j = 0; j < pack_jobs.size() && ok; ++j) ok = units[j] == pack_jobs[j].total;
        if (!ok) { sgd_tiles.clear(); return; }
        std::stable_sort(sgd_tiles.begin(), sgd_tiles.end(), [](const SgdTile& a, const SgdTile& b) { return a.count > b.count; });
    }
};

namespace {

// The separate launches of a norm layer, shared by the executor (OP_NORM, view_backward) and the single-op surface.  Forward: the
// statistics from `rows` partial rows in `partial` (0: a statistics pass over `raw` first; dbl: fp64 rows) or, in eval mode, the
// running ones; then the activated copy into act_out (may be nullptr), in one launch with the finalize where the rows are few.
// unet_op_norm_choice (below) restates which launch each step of these two functions ends in, for rows = 0 in training mode with an
// activated copy: whoever changes how the predicates are combined here (fused only when !dbl && act_out; the backward's vec8_ok) changes
// it there as well.
void norm_fwd_passes(int dtype, const void* raw, int C, int64_t S, float* partial, int rows, bool dbl, bool eval, const float* gamma,
                     const float* beta, double eps, float* stat, float* rm, float* rv, int act, void* act_out, hipStream_t s) {
    if (eval) launch_norm_eval(C, gamma, beta, rm, rv, eps, stat, s);
    else {
        if (!rows) {
            launch_stats_partial(dtype, raw, C, S, partial, s);
            rows = stats_blocks(S);
            dbl = dtype == UNET_DTYPE_F32;
        }
        // few partial rows (32^3 and deeper): finalize + activated copy in one launch
        if (!dbl && act_out && launch_norm_finalize_apply(dtype, partial, rows, C, S, gamma, beta, eps, stat, rm, rv, 0.1, raw, act, act_out, s))
            return;
        launch_norm_finalize(partial, rows, C, S, gamma, beta, eps, stat, rm, rv, 0.1, s, dbl);
    }
    if (act_out) {
        SrcDesc d;
        d.ptr = raw; d.C = C; d.act = act; d.scale = stat + 2 * C; d.shift = stat + 3 * C;
        launch_apply_view(dtype, d, act_out, S, s);
    }
}
// Backward: g holds dL/d(view of u) and becomes dL/d(raw u); coef and the affine gradients (+=) are written.  rows > 0: the statistics
// rows a dgrad epilogue left in `partial`.  no_apply: stop after the finalize (the element-wise pass is fused into the consumer).
void norm_bwd_passes(int dtype, void* g, const void* u, int C, int64_t S, const float* stat, int act, const float* gamma, float* coef,
                     float* dgamma, float* dbeta, float* partial, int rows, bool no_apply, hipStream_t s) {
    if (rows <= 0) {
        launch_norm_bwd_partial(dtype, g, u, C, S, stat, act, partial, s);
        rows = stats_blocks(S);
    }
    if (!no_apply && launch_norm_bwd_finalize_apply(dtype, partial, rows, C, S, gamma, stat, coef, dgamma, dbeta, g, u, act, s)) return;
    launch_norm_bwd_finalize(partial, rows, C, S, gamma, stat, coef, dgamma, dbeta, s, dtype == UNET_DTYPE_F32);
    if (!no_apply) launch_norm_bwd_apply(dtype, g, u, C, S, stat, coef, act, s);
}
// The input gradient of a conv / conv_trans on the matrix cores (Dgrad::mfma), shared by the executor and the single-op surface: the
// deep levels' split-K kernel where its outcome query says it takes the shape, else the halo-tile / sliding-window family.  nb
// (optional): the norm whose view the one destination is, offered to the kernel's epilogue; partial: where its statistics rows go.
// Returns who finishes that norm backward -- known BEFORE the launch (launch == false: nothing is enqueued, the answer alone: the dry
// replay of a backward in parts), and what a launcher then reports must be that prediction.
DgradOutcome mfma_dgrad(const ConvGeom& g, bool transposed, const void* dy, const void* wm, const DstGrad* dst, int ndst, const DeepNormBwd* nb,
                        float* partial, const DeepScratch& deep, hipStream_t s, bool launch = true) {
    const bool norm = nb != nullptr;
    DgradOutcome want = deep_dgrad_outcome(g, transposed, dst, ndst, norm, deep);
    const bool on_deep = want.served;
    if (!on_deep) {
        if (transposed) want.served = true;     // (launch_mfma_convt_dgrad: every shape, no norm epilogue)
        else want = mfma_conv_dgrad_outcome(g, dst, ndst, norm);
    }
    if (!launch) return want;
    DgradOutcome got = want;
    if (on_deep) got = launch_deep_dgrad(g, transposed, dy, wm, dst, ndst, nb, deep, s);
    else if (transposed) launch_mfma_convt_dgrad(g, dy, wm, dst, ndst, s);
    else {
        const BnBwdStats bn = {norm ? nb->u : nullptr, norm ? nb->stat : nullptr, partial, norm ? nb->act : 0, dst[0].C};
        got = launch_mfma_conv_dgrad(g, dy, wm, dst, ndst, s, norm ? &bn : nullptr);
    }
    if (!(got == want)) throw std::runtime_error("dgrad: the launch did not do what its outcome query predicted");
    return want;
}

// conv_fwd, conv_dgrad and conv_wgrad: the launch of each direction of a conv / conv_trans from its ConvChoice member (conv_select.h),
// shared by the executor and the single-op surface and the only places of this file that map Fwd / Dgrad / Wgrad to launchers.  The
// callers keep the scheduling: the stream, when which filter form is packed, the forks, where the slabs lie.
struct FwdRan {
    int rows = 0;            // statistics partial rows the launch left in `part`
    bool dbl = false;        // ... as fp64 rows (the fp32 matrix-core convs)
    bool norm_done = false;  // the deep kernel ran the whole norm layer `nf` in its epilogue
};
// The three filter forms a family may read: w the fp32 torch-layout parameter, wf its fp32 tap-major copy (launch_pack_conv_w /
// launch_pack_convt_w), wm the bf16 MFMA pack -- only the one f reads (ConvChoice::mfma_fwd / param_fwd) need be there.  out_ncdhw
// (optional; head and direct): the fp32 NCDHW result; a head then writes no channels-last copy.  part (optional): where the
// statistics rows of `out` go.  nf (optional): the norm + activation behind the conv, offered to the deep kernel's epilogue.  An
// empty DeepScratch keeps the deep levels' split-K kernels out (they decline: the mfma kernels run).
FwdRan conv_fwd(Fwd f, bool transposed, int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const float* w, const float* wf,
                const void* wm, const float* bias, void* out, float* out_ncdhw, float* part, const DeepNormFwd* nf, const DeepScratch& deep,
                hipStream_t s) {
    FwdRan r;
    int rows = 0;
    switch (f) {
        case Fwd::deep:
        case Fwd::mfma:
            if (transposed) {
                if (!launch_deep_convt_fwd(g, src, nsrc, wm, bias, out, deep, s)) launch_mfma_convt_fwd(g, src, nsrc, wm, bias, out, s);
                return r;
            }
            // the deep levels: split-K kernel, the norm layer behind the conv in its epilogue (statistics, running statistics,
            // activated copy: the caller's norm passes have nothing left to do)
            if (f == Fwd::deep && launch_deep_conv_fwd(g, src, nsrc, wm, bias, out, nf, deep, s)) {
                r.norm_done = nf != nullptr;
                return r;
            }
            rows = launch_mfma_conv_fwd(g, src, nsrc, wm, bias, out, part, s);
            break;
        case Fwd::head:
            launch_head_fwd(dtype, g, src[0], w, bias, out_ncdhw ? nullptr : out, out_ncdhw, s);
            return r;
        case Fwd::first_mfma:
            rows = launch_conv_first_mfma(g, src, w, bias, out, part, s);
            break;
        case Fwd::first_f32_mfma:
            // fp32 engine, Cin = 1: the first conv on the fp32 matrix cores (filter read in torch layout), statistics in its epilogue
            rows = launch_conv_first_f32_mfma(g, src, w, bias, (float*)out, (double*)part, s);
            r.dbl = true;
            break;
        case Fwd::f32_mfma:
            if (transposed) { launch_convt_f32_mfma(g, src, wf, bias, (float*)out, s); return r; }
            // fp32 engine: the same IEEE fp32 products and sums as the VALU kernel below, on the fp32 matrix cores
            rows = launch_conv_f32_mfma(g, src, nsrc, wf, bias, (float*)out, s, (double*)part);
            r.dbl = true;
            break;
        case Fwd::direct:
            if (transposed) launch_convt_fwd_direct(dtype, g, src, nsrc, wf, bias, out, s);
            else launch_conv_fwd_direct(dtype, g, src, nsrc, wf, bias, out, out_ncdhw, s);
            return r;
    }
    r.rows = part ? rows : 0;
    return r;
}
// The input gradient: wm the bf16 MFMA dgrad pack, wd the fp32 tap-major dgrad copy (the one d reads).  nb, partial, deep and the
// returned outcome as mfma_dgrad's: only the matrix-core family has norm epilogues, the others leave the whole norm backward to
// the caller.  launch == false: the outcome alone.
DgradOutcome conv_dgrad(Dgrad d, bool transposed, int dtype, const ConvGeom& g, const void* dy, const void* wm, const float* wd,
                        const DstGrad* dst, int ndst, const DeepNormBwd* nb, float* partial, const DeepScratch& deep, hipStream_t s,
                        bool launch = true) {
    if (d == Dgrad::mfma) return mfma_dgrad(g, transposed, dy, wm, dst, ndst, nb, partial, deep, s, launch);
    DgradOutcome o;
    o.served = true;
    if (!launch) return o;
    if (d == Dgrad::f32_mfma) launch_conv_f32_mfma_dgrad(g, (const float*)dy, wd, dst, ndst, s);
    else if (transposed) launch_convt_dgrad_direct(dtype, g, dy, wd, dst, ndst, s);
    else launch_conv_dgrad_direct(dtype, g, dy, wd, dst, ndst, s);
    return o;
}
// The weight (+ bias) gradient, added into dw / db.  scratch: the slab region (the direct kernels take nullptr: no split of the voxel
// range); defer: the matrix-core slab kernels only write their slab, the caller's batched reduce sums it; polite: see kernels.h
// (the bf16 matrix-core kernels; the same value as given to *_scratch_bytes / *_splits); nbf (optional): the first conv applies the
// norm backward's element-wise pass as it stages dy.
void conv_wgrad(Wgrad w, bool transposed, int dtype, const ConvGeom& g, const SrcDesc* src, int nsrc, const void* dy, float* dw, float* db,
                void* scratch, hipStream_t s, bool defer, int polite, const NormBwdFuse* nbf) {
    switch (w) {
        case Wgrad::first_mfma: launch_conv_first_wgrad_mfma(g, src, dy, dw, db, scratch, s, defer, nbf); break;
        case Wgrad::mfma:
            if (transposed) launch_mfma_convt_wgrad(g, src, dy, dw, scratch, s, defer, db, polite);
            else launch_mfma_conv_wgrad(g, src, nsrc, dy, dw, db, scratch, s, defer, polite);
            break;
        case Wgrad::f32_mfma: launch_wgrad_f32_mfma(g, src, nsrc, (const float*)dy, dw, db, scratch, s); break;
        case Wgrad::small: launch_conv_wgrad_small(dtype, g, src, nsrc, dy, dw, db, scratch, s); break;
        case Wgrad::direct:
            if (transposed) launch_convt_wgrad_direct(dtype, g, src, nsrc, dy, dw, db, scratch, s);
            else launch_conv_wgrad_direct(dtype, g, src, nsrc, dy, dw, db, scratch, s);
            break;
    }
}

struct Exec {
    const unet_plan& p;
    char* ws;
    hipStream_t s;
    // the deep levels' kernels may run in this call: the workspace's arrival counters are known to be zero (cleared by the batched filter
    // pack of this forward, or of the forward whose packs / activations this call works on)
    bool deep_on = false;
    Exec(const unet_plan& plan, void* workspace, void* stream) : p(plan), ws((char*)workspace), s((hipStream_t)stream) {}
    DeepScratch deep() const {
        DeepScratch d;
        if (deep_on && p.deep_part_bytes) { d.part = (float*)(ws + p.deep_part_off); d.part_bytes = p.deep_part_bytes; d.cnt = (int*)(ws + p.deep_cnt_off); d.ncnt = p.deep_ncnt; }
        return d;
    }
    int* deep_cnt() const { return p.deep_part_bytes ? (int*)(ws + p.deep_cnt_off) : nullptr; }

    void* at(size_t off) const { return off == SIZE_MAX ? nullptr : ws + off; }   // a region the plan may not have laid out
    void* tptr(int t) const { return ws + p.t_off[t]; }
    void* gptr(int t) const { return at(p.g_off[t]); }
    float* stat(int n) const { return (float*)(ws + p.n_stat[n]); }
    float* coef(int n) const { return (float*)(ws + p.n_coef[n]); }
    float* partial() const { return (float*)(ws + p.partial_off); }

    // the raw tensor with its recorded norm + activation applied by the reader
    SrcDesc raw_src(int t) const {
        const Tensor& T = p.g.tensors[t];
        SrcDesc d;
        d.ptr = tptr(t); d.C = T.C; d.act = T.act;
        if (T.norm >= 0) { d.scale = stat(T.norm) + 2 * T.C; d.shift = stat(T.norm) + 3 * T.C; }
        return d;
    }
    // what consumers read: the activated copy when the plan keeps one (no per-read transform), else the raw tensor + transform
    SrcDesc src(int t) const {
        if (p.a_off[t] == SIZE_MAX) return raw_src(t);
        SrcDesc d;
        d.ptr = ws + p.a_off[t]; d.C = p.g.tensors[t].C;
        return d;
    }
    // after the producer (and its norm statistics) are done: write the activated copy
    void apply_view(int t) const {
        if (p.a_off[t] != SIZE_MAX) launch_apply_view(p.dtype, raw_src(t), ws + p.a_off[t], p.g.tensors[t].voxels(), s);
    }
    ConvGeom geom(const Op& op) const { return p.op_geom_of(op); }

    // on_head(level): called right after the launches that produce results[level] (a fused forward + loss issues that level's loss there)
    void forward(const float* const* params, float* const* buffers, const float* x, float* const* outs, int mode,
                 const std::function<void(int)>* on_head = nullptr) {
        const Graph& g = p.g;
        // UNET_MODE_PACKS_CURRENT: the filter packs this workspace holds were made from these parameter values (an earlier mode-1
        // forward on it since the last update): micro-steps 2..batch_size of an optimizer step skip the ~0.1 ms / 190 MB repack
        const bool packs_current = (mode & UNET_MODE_PACKS_CURRENT) != 0;
        mode &= 1;
        std::vector<int> fused_blocks(g.norms.size(), 0);   // > 0: the producing conv already wrote the statistics partials
        std::vector<char> fused_dbl(g.norms.size(), 0);     // ... as fp64 rows (the fp32 engine)
        std::vector<char> fused_done(g.norms.size(), 0);    // the producing conv ran the whole norm layer in its epilogue (kernels_mfma_deep.hip)
        // parameters in one flat contiguous buffer (the hosts allocate them so): every MFMA filter pack in ONE launch
        bool packed = false, pack_pending = false, pack2_pending = false;
        if (p.jobs_dev && packs_current) { packed = true; deep_on = true; }
        else if (p.jobs_dev) {
            if (p.is_flat(params)) {
                // training forward: the pack runs on the plan's side stream beside the input pack, the first conv (which reads the
                // fp32 filter) and its norm; the first kernel that needs packed filters waits for it.  (Eval forwards stay on the
                // caller's stream: they are re-entrant per workspace, the side stream and its events are per plan.)
                const int njobs = (int)p.pack_jobs.size();
                if (mode == 1 && p.side && !env().no_side_stream && !g_prof) {
                    HIP_OK(hipEventRecord(p.ev_fork, s));
                    HIP_OK(hipStreamWaitEvent(p.side, p.ev_fork, 0));
                    if (p.pack_split_op > 0 && p.pack_split_blocks > 0) {
                        // three launches: the top levels' forward packs (a few hundred KB: the first MFMA conv waits for these only), the
                        // other forward packs, the dgrad packs (nothing reads them before the backward).  Measured and not kept: a bounded
                        // grid for the later launches (no gain), the dgrad packs launched when the caller's stream reaches the 16^3 level
                        // (2.925-2.935 ms against 2.915: their 5800 short blocks delay the small levels' latency-bound kernels by more
                        // than they cost the bandwidth-bound ones), one launch for everything (a 20-us bubble in front of the first MFMA conv).
                        launch_mfma_pack_batched(params[0], ws, p.jobs_dev, njobs, p.pack_split_blocks, p.side, 0, 0, deep_cnt(), p.deep_ncnt);
                        HIP_OK(hipEventRecord(p.ev_join, p.side));
                        launch_mfma_pack_batched(params[0], ws, p.jobs_dev, njobs, p.pack_fwd_blocks - p.pack_split_blocks, p.side, p.pack_split_blocks);
                        HIP_OK(hipEventRecord(p.ev_pack, p.side));
                        pack2_pending = true;
                        launch_mfma_pack_batched(params[0], ws, p.jobs_dev, njobs, p.pack_blocks - p.pack_fwd_blocks, p.side, p.pack_fwd_blocks);
                        HIP_OK(hipEventRecord(p.ev_packd, p.side));
                    } else {
                        launch_mfma_pack_batched(params[0], ws, p.jobs_dev, njobs, p.pack_blocks, p.side, 0, 0, deep_cnt(), p.deep_ncnt);
                        HIP_OK(hipEventRecord(p.ev_join, p.side));
                    }
                    pack_pending = true;
                } else {
                    // an inference forward never reads a dgrad pack
                    ProfScope ps(-1, UNET_PROF_OTHER, s);
                    launch_mfma_pack_batched(params[0], ws, p.jobs_dev, njobs, mode == 1 ? p.pack_blocks : p.pack_fwd_blocks, s, 0, 0, deep_cnt(), p.deep_ncnt);
                }
                packed = true;
                deep_on = true;
            }
        }
        auto need_packs = [&](int op_index = 1 << 30) {
            if (pack_pending) { HIP_OK(hipStreamWaitEvent(s, p.ev_join, 0)); pack_pending = false; }
            if (pack2_pending && op_index >= p.pack_split_op) { HIP_OK(hipStreamWaitEvent(s, p.ev_pack, 0)); pack2_pending = false; }
        };
        for (size_t i = 0; i < g.ops.size(); ++i) {
            const Op& op = g.ops[i];
            ProfScope ps((int)i, (op.kind == OP_CONV || op.kind == OP_CONVT) ? UNET_PROF_CONV_FWD : op.kind == OP_NORM ? UNET_PROF_NORM_FWD : UNET_PROF_OTHER, s);
            switch (op.kind) {
                case OP_PACK_INPUT:
                    launch_pack_input(p.dtype, x, tptr(op.dst), g.in_c, g.tensors[op.dst].voxels(), s);
                    break;
                case OP_CONV:
                case OP_CONVT: {
                    if (op.out_level >= 0 && !(outs && outs[op.out_level])) break;  // result not wanted
                    const bool convt = op.kind == OP_CONVT;
                    SrcDesc sd[2] = {src(op.src[0]), op.nsrc > 1 ? src(op.src[1]) : SrcDesc()};
                    ConvGeom cg = geom(op);
                    float* wf = (float*)(ws + p.w_fwd[i]);
                    float* wd = (float*)(ws + p.w_dgrad[i]);
                    const int k3 = op.ks * op.ks * op.ks;
                    const ConvChoice& c = p.conv[i];
                    const Tensor& T = g.tensors[op.dst];
                    const bool want_stats = T.norm >= 0 && !(g.norms[T.norm].batch && mode == 0);
                    // the bf16 filter packs: the batched launch above, else made here
                    if (c.mfma_fwd()) {
                        need_packs((int)i);
                        void* const wmd = (mode == 1 && c.dgrad == Dgrad::mfma) ? ws + p.wm_dgrad[i] : nullptr;
                        if (!packed && convt) launch_mfma_pack_convt_w(params[op.weight], ws + p.wm_fwd[i], wmd, cg, s);
                        else if (!packed) launch_mfma_pack_conv_w(params[op.weight], ws + p.wm_fwd[i], wmd, cg, s);
                    }
                    // the fp32 tap-major copies [wf | wd]: for a forward that reads wf, and in training for a dgrad off the bf16 matrix cores,
                    // which reads wd (not a head's: its fused backward reads the parameter; the bf16 first conv's only when its input needs a
                    // gradient).  Behind the launch where the forward reads the parameter itself: off the first conv's path
                    const bool copies = !packs_current && ((!c.mfma_fwd() && !c.param_fwd()) ||
                                                           (mode == 1 && c.dgrad != Dgrad::mfma && c.fwd != Fwd::head &&
                                                            (c.fwd != Fwd::first_mfma || g.tensors[op.src[0]].needs_grad)));
                    auto pack_copies = [&]() {
                        if (convt) launch_pack_convt_w(params[op.weight], wf, wd, op.cin, op.cout, s);
                        else launch_pack_conv_w(params[op.weight], wf, wd, op.cin, op.cout, k3, s);
                    };
                    if (copies && !c.param_fwd()) pack_copies();
                    // the deep levels' split-K kernel takes the norm layer behind the conv into its epilogue: the OP_NORM that follows has
                    // nothing left to do
                    DeepNormFwd nf;
                    const bool fuse = deep_on && T.norm >= 0 && p.a_off[op.dst] != SIZE_MAX;
                    if (fuse) {
                        const Norm& n = g.norms[T.norm];
                        nf = {params[n.gamma], params[n.beta], n.eps, stat(T.norm), n.batch ? buffers[n.buffer] : nullptr,
                              n.batch ? buffers[n.buffer + 1] : nullptr, 0.1, (n.batch && mode == 0) ? 1 : 0, T.act, ws + p.a_off[op.dst]};
                    }
                    // (results[level] is written by the conv itself)
                    const FwdRan r = conv_fwd(c.fwd, convt, p.dtype, cg, sd, op.nsrc, params[op.weight], wf, at(p.wm_fwd[i]), params[op.bias],
                                              tptr(op.dst), op.out_level >= 0 ? outs[op.out_level] : nullptr, want_stats ? partial() : nullptr,
                                              fuse ? &nf : nullptr, deep(), s);
                    if (copies && c.param_fwd()) pack_copies();
                    if (r.norm_done) fused_done[T.norm] = 1;
                    else if (want_stats) { fused_blocks[T.norm] = r.rows; fused_dbl[T.norm] = r.dbl; }
                    break;
                }
                case OP_NORM: {
                    const Norm& n = g.norms[op.norm];
                    const Tensor& T = g.tensors[n.tensor];
                    if (fused_done[op.norm]) break;
                    // (fp32 tensors leave fp64 block partials: k_stats_partial, k_conv_f32_mfma)
                    norm_fwd_passes(p.dtype, tptr(n.tensor), n.C, T.voxels(), partial(), fused_blocks[op.norm], fused_dbl[op.norm] != 0,
                                    n.batch && mode == 0, params[n.gamma], params[n.beta], n.eps, stat(op.norm),
                                    n.batch ? buffers[n.buffer] : nullptr, n.batch ? buffers[n.buffer + 1] : nullptr, T.act,
                                    p.a_off[n.tensor] != SIZE_MAX ? ws + p.a_off[n.tensor] : nullptr, s);
                    break;
                }
                case OP_MATERIALIZE: {
                    SrcDesc sd[2] = {src(op.src[0]), op.nsrc > 1 ? src(op.src[1]) : SrcDesc()};
                    launch_materialize(p.dtype, sd, op.nsrc, tptr(op.dst), g.tensors[op.dst].voxels(), s);
                    break;
                }
                case OP_MAXPOOL: {
                    const Tensor& a = g.tensors[op.src[0]];
                    launch_maxpool_fwd(p.dtype, src(op.src[0]), tptr(op.dst), a.D, a.H, a.W, s);
                    break;
                }
                case OP_UPSAMPLE: {
                    const Tensor& a = g.tensors[op.src[0]];
                    launch_upsample_fwd(p.dtype, src(op.src[0]), tptr(op.dst), a.D, a.H, a.W, s);
                    break;
                }
                case OP_EXPORT:
                    if (outs && outs[op.out_level])
                        launch_export(p.dtype, src(op.src[0]), outs[op.out_level], g.tensors[op.src[0]].voxels(), s);
                    break;
            }
            // an activation recorded on a tensor that has no norm (e.g. "conv8,relu"): its copy is due right after the producer
            if (op.kind != OP_NORM && op.kind != OP_EXPORT && op.dst >= 0) {
                const Tensor& T = g.tensors[op.dst];
                if (T.norm < 0 && T.act != ACT_NONE) apply_view(op.dst);
            }
            if (on_head && op.out_level >= 0 && outs && outs[op.out_level] && (op.kind == OP_CONV || op.kind == OP_CONVT || op.kind == OP_EXPORT))
                (*on_head)(op.out_level);
        }
        need_packs();   // nothing consumed the packs (no MFMA op): still order the caller's stream after the side stream
    }

    // g[t] holds dL/d(view of t); turn it into dL/d(raw t) (and accumulate the norm's affine gradients)
    // no_apply: stop after the finalize (coef(T.norm) is final; dgamma / dbeta accumulated) -- the element-wise pass is fused into the one
    // consumer of dL/d(raw t) (the first conv's weight gradient).  rows > 0: the statistics rows that the dgrad which produced this
    // gradient left in partial()
    void view_backward(int t, const float* const* params, float* const* gparams, bool no_apply, int rows) {
        const Tensor& T = p.g.tensors[t];
        if (T.norm >= 0) {
            const Norm& n = p.g.norms[T.norm];
            norm_bwd_passes(p.dtype, gptr(t), tptr(t), T.C, T.voxels(), stat(T.norm), T.act, params[n.gamma], coef(T.norm),
                            gparams[n.gamma], gparams[n.beta], partial(), rows, no_apply, s);
        } else if (T.act != ACT_NONE) {
            launch_act_bwd(p.dtype, gptr(t), tptr(t), T.act, T.numel(), s);
        }
    }

    // Ops [op_lo, op_hi) are run (in reverse); ops >= op_hi are only replayed on the host (dry) to rebuild which gradient buffers
    // already hold a value: that state depends on the graph and on which grad_outs are given, not on earlier calls, so the
    // backward can be issued in parts (unet_backward_part) with collectives of finished gradient buckets in between.
    void backward(const float* const* params, const float* const* grad_outs, float* const* gparams, float* grad_x, int op_hi = 1 << 30,
                  int op_lo = 0) {
        const Graph& g = p.g;
        // the dgrad filter packs of this step were launched on the side stream in the middle of the forward.  The wait is unconditional:
        // the packs belong to a (workspace, stream) pair but the event is the plan's, and with two workspaces interleaved
        // (A.forward, B.forward, B.backward, A.backward) a consumed-once flag let A's backward run ahead of A's packs.  The event's latest
        // record is behind every earlier pack on the side stream, and waiting on a never-recorded or completed event costs nothing.
        if (p.side) HIP_OK(hipStreamWaitEvent(s, p.ev_packd, 0));
        // the deep levels' kernels: only behind a forward that made its packs with the batched launch (which cleared the counters)
        deep_on = p.jobs_dev && p.is_flat(params);
        std::vector<char> init(g.tensors.size(), 0);
        auto dst_of = [&](int t) {
            DstGrad d;
            d.C = g.tensors[t].C;
            d.ptr = g.tensors[t].needs_grad ? gptr(t) : nullptr;
            d.accumulate = init[t];
            return d;
        };
        auto mark = [&](const Op& op) {
            for (int k = 0; k < op.nsrc; ++k)
                if (g.tensors[op.src[k]].needs_grad) init[op.src[k]] = 1;
        };
        // sb: where the parameter-gradient kernels go.  fork() orders them after everything issued so far on the caller's stream
        // (dL/d(raw output) of the layer is final); the join at the end orders the caller's stream after them.
        const hipStream_t sb = (p.side && !env().no_side_stream && !g_prof) ? p.side : s;
        auto fork = [&]() {
            if (sb == s) return;
            HIP_OK(hipEventRecord(p.ev_fork, s));
            HIP_OK(hipStreamWaitEvent(sb, p.ev_fork, 0));
        };
        if (op_lo < 0) op_lo = 0;
        // The hand-off from a dgrad to the view_backward of its destination (a norm layer's view), rebuilt by the dry replay like init[]:
        // ONE slot for the statistics rows an epilogue left in partial() -- the next norm view_backward consumes it when it is that
        // tensor's, else drops it (its own statistics pass overwrites partial()) -- and, per tensor, "its whole norm backward already ran"
        int bn_tensor = -1, bn_rows = 0;
        std::vector<char> norm_done(g.tensors.size(), 0);
        // gradients in one flat buffer (both hosts allocate them so): the sliding-window wgrads only write their slabs here and ONE
        // batched reduce at the end of this call adds them all into the gradients
        const bool gflat = p.wz_jobs_dev && p.is_flat(gparams);
        std::vector<char> wz_ran(p.wz_jobs.size(), 0);
        int wz_pending = 0;
        // slabs of the weight gradients launched so far -> gradients: one launch per run of consecutive jobs (normally one).  Flushed
        // every few layers, not only at the end: a single reduce of everything would sit behind the last layer on the side stream
        // and the caller's stream waits for it at the join.
        auto flush_wz = [&](hipStream_t st) {
            for (size_t j = 0; j < wz_ran.size();) {
                if (!wz_ran[j]) { ++j; continue; }
                size_t e = j;
                int nblk = 0;
                while (e < wz_ran.size() && wz_ran[e]) { nblk += p.wz_jobs[e].nblk; wz_ran[e] = 0; ++e; }
                ProfScope pr(-1, UNET_PROF_WGRAD, st);
                launch_wgrad_reduce_batched(p.wz_jobs_dev, (int)j, (int)(e - j), p.wz_jobs[j].blk0, nblk, ws, gparams[0], st);
                j = e;
            }
            wz_pending = 0;
        };
        // weight / bias gradient of op i (its dL/d(raw output) is final), enqueued on sb
        auto do_wgrad = [&](int i) {
            const Op& op = g.ops[i];
            const int t = op.dst;
            SrcDesc sd[2] = {src(op.src[0]), op.nsrc > 1 ? src(op.src[1]) : SrcDesc()};
            ConvGeom cg = geom(op);
            // the stride-2 convs above 32^3 (wgrad_on_main, choose_polite): the kernel and its slab sum on the caller's stream, the slab in
            // the op's own region (the shared scratch is the side stream's)
            const bool on_main = op.kind == OP_CONV && p.wgrad_on_main[i] && p.wz_off[i] != SIZE_MAX;
            const bool defer = gflat && p.wz_job_of_op[i] >= 0 && !on_main;   // slab only: summed by the batched reduce below
            // the slab in the op's own region where the batched reduce sums it later, and for a conv's bf16 slab kernels whenever the plan
            // laid one out; else in the shared scratch
            const bool own = p.wz_off[i] != SIZE_MAX && (defer || (op.kind == OP_CONV && p.conv[i].wgrad == Wgrad::mfma));
            {   // the op's own bracket closes before flush_wz opens the batched reduce's (they would nest and count the reduce twice)
            ProfScope pw(i, UNET_PROF_WGRAD, sb);
            conv_wgrad(p.conv[i].wgrad, op.kind == OP_CONVT, p.dtype, cg, sd, op.nsrc, gptr(t), gparams[op.weight], gparams[op.bias],
                       ws + (own ? p.wz_off[i] : p.wgrad_off), on_main ? s : sb, defer, on_main ? 0 : p.side_polite[i], nullptr);
            }
            if (defer) { wz_ran[p.wz_job_of_op[i]] = 1; ++wz_pending; }
            if (wz_pending >= 3) flush_wz(sb);      // (every layer and one flush at the end both measured slower: profiles/r06 A/Bs)
        };
        // The backward starts at full resolution, where the caller's stream is bandwidth-bound, and then spends a long stretch in the
        // small levels, where it is launch-latency bound and the memory system idles.  The big weight gradients of the decoder's top
        // levels (everything they read stays in the workspace: each tensor has a gradient buffer of its own) are therefore HELD until
        // the caller's stream reaches the small levels and run beside those, instead of competing with the top levels' dgrad / norm
        // kernels for bandwidth.
        const int64_t hold_from = (int64_t)64 * 64 * 64, hold_below = (int64_t)32 * 32 * 32;
        std::vector<int> held;
        bool deep_seen = false;
        // An event record on the caller's stream is not free: the kernel behind it starts ~6 us late (time line of a step,
        // profiles/r07_timeline.txt: every dgrad that follows a fork).  The weight gradient of a layer can start any time after its
        // dL/d(raw output) is final, so forks are shared: layers wait in `pending` and ONE fork serves `fork_every` of them.
        constexpr int fork_every = 3;
        std::vector<int> pending;
        auto issue_pending = [&]() {
            if (pending.empty()) return;
            fork();
            for (int h : pending) do_wgrad(h);
            pending.clear();
        };
        for (int i = (int)g.ops.size() - 1; i >= op_lo; --i) {
            const Op& op = g.ops[i];
            const bool dry = i >= op_hi;
            if (op.kind == OP_NORM) continue;
            if (op.kind == OP_EXPORT) {
                if (grad_outs && grad_outs[op.out_level] && g.tensors[op.src[0]].needs_grad) {
                    if (!dry) launch_export_bwd(p.dtype, grad_outs[op.out_level], dst_of(op.src[0]), g.tensors[op.src[0]].voxels(), s);
                    mark(op);
                }
                continue;
            }
            int t = op.dst;
            if ((op.kind == OP_CONV) && op.out_level >= 0) {
                if (!(grad_outs && grad_outs[op.out_level])) continue;
                if (p.conv[i].fwd == Fwd::head) {
                    // fused head backward: dL/dW, dL/db and dL/d(source view) in one pass over (source, dL/dresults[level])
                    DstGrad dgh = dst_of(op.src[0]);
                    ProfScope ph(dry ? -2 : i, UNET_PROF_OTHER, s);
                    if (!dry) {
                        // the slab sum that finishes the head's dW / db feeds nothing on the caller's chain: on the side stream (a slab region
                        // per head, so the next level's head does not overwrite rows that have not been summed yet)
                        const bool defer = sb != s && p.head_op_off[i] != SIZE_MAX;
                        char* hs = ws + (defer ? p.head_op_off[i] : p.head_off);
                        launch_head_bwd(p.dtype, geom(op), src(op.src[0]), grad_outs[op.out_level], nullptr, params[op.weight], dgh,
                                        gparams[op.weight], gparams[op.bias], hs, s, defer);
                        if (defer) { fork(); launch_head_bwd_reduce(geom(op), gparams[op.weight], gparams[op.bias], hs, sb); }
                    }
                    if (dgh.ptr) mark(op);
                    continue;
                }
                if (!dry) launch_import_grad(p.dtype, grad_outs[op.out_level], gptr(t), g.tensors[t].C, g.tensors[t].voxels(), 0, s);
                init[t] = 1;
            }
            if (!g.tensors[t].needs_grad || !init[t]) continue;
            // The network's first conv with a norm behind it: dL/d(raw output) is only read by its weight gradient (the input needs no
            // gradient), which applies the norm backward's element-wise pass itself (NormBwdFuse) -- see the OP_CONV case below
            bool first_fused = false;
            if (!dry && p.conv[i].wgrad == Wgrad::first_mfma && g.tensors[t].norm >= 0 && !g.tensors[op.src[0]].needs_grad && sb != s &&
                p.wz_off[i] != SIZE_MAX && g.tensors[t].C % 8 == 0)
                first_fused = !env().no_first_wgrad_fuse;
            {
                const bool has_norm = g.tensors[t].norm >= 0;
                const bool done = has_norm && norm_done[t];    // dL/d(raw), the affine gradients and coef() are already there
                int rows = 0;
                if (done) norm_done[t] = 0;
                else if (has_norm) { if (bn_tensor == t) rows = bn_rows; bn_tensor = -1; }
                if (!dry) { ProfScope ps(i, UNET_PROF_NORM_BWD, s); if (!done) view_backward(t, params, gparams, first_fused, rows); }
            }
            switch (op.kind) {
                case OP_CONV:
                case OP_CONVT: {
                    SrcDesc sd[2] = {src(op.src[0]), op.nsrc > 1 ? src(op.src[1]) : SrcDesc()};
                    DstGrad dg[2] = {dst_of(op.src[0]), op.nsrc > 1 ? dst_of(op.src[1]) : DstGrad()};
                    ConvGeom cg = geom(op);
                    const float* wd = (const float*)(ws + p.w_dgrad[i]);
                    bool any = dg[0].ptr || (op.nsrc > 1 && dg[1].ptr);
                    // parameter gradients: on the side stream now, or held back (see `held`)
                    // The network's first conv (its input needs no gradient: nothing follows on the caller's stream) -- its weight gradient is
                    // the last kernel of the backward whichever stream it is on; on the caller's stream it starts without waiting for a fork
                    // and its reduce is not behind the side stream's queue.  Slab in the op's own region (the shared scratch is the side stream's).
                    if (!dry && !any && sb != s && p.conv[i].wgrad == Wgrad::first_mfma && p.wz_off[i] != SIZE_MAX) {
                        ProfScope pw(i, UNET_PROF_WGRAD, s);
                        const Tensor& To = g.tensors[t];
                        NormBwdFuse nf = {tptr(t), first_fused ? stat(To.norm) : nullptr, first_fused ? coef(To.norm) : nullptr, To.act};
                        conv_wgrad(p.conv[i].wgrad, false, p.dtype, cg, sd, op.nsrc, gptr(t), gparams[op.weight], gparams[op.bias], ws + p.wz_off[i],
                                   s, false, 0, first_fused ? &nf : nullptr);
                    } else
                    if (!dry) {
                        const int64_t vox = (int64_t)cg.Do * cg.Ho * cg.Wo;
                        if (!deep_seen && vox <= hold_below && !held.empty()) {     // the small levels begin: the held launches run beside them
                            deep_seen = true;
                            pending.insert(pending.begin(), held.begin(), held.end());
                            held.clear();
                            pending.push_back(i);
                            issue_pending();
                        } else if (!deep_seen && sb != s && vox >= hold_from) held.push_back(i);
                        else {
                            // forks are shared among the small levels' layers only (many short launches, the side stream has slack); a layer of
                            // 32^3 voxels or more forks at once: held back, the encoder's last weight gradients would start after the caller's
                            // stream has finished and lengthen the tail of the step (time line r07f2: +60 us before the join)
                            pending.push_back(i);
                            if ((int)pending.size() >= fork_every || sb == s || vox >= hold_below) issue_pending();
                        }
                    }
                    ProfScope pd(i, UNET_PROF_DGRAD, s);
                    if (any) {
                        // The source is a norm layer's view read by this conv alone: its gradient is complete when this dgrad
                        // has written it, so the statistics pass of that norm's backward (a second read of the gradient and of the
                        // raw tensor) moves into the dgrad's epilogue where the kernel has one (k_mfma_conv_z16).  The rows wait in
                        // partial(): the next thing the caller's stream runs is that tensor's view_backward.
                        // With several consumers the one with the lowest op index writes last -- accumulating -- and sees the complete
                        // gradient: for the skip tensors that is the stride-2 conv, whose dgrad (k_s2_scatter) fetches the old gradient
                        // and the raw tensor by LDS-DMA and has the epilogue too.  (Stride-1 kernels only take it when they WRITE.)
                        // The deep levels' split-K kernels, as the last writer of a norm layer's view, run that norm's whole backward.
                        // (Only the bf16 matrix-core family has such epilogues: conv_dgrad.)
                        const int ts = op.src[0];
                        const Tensor& Ts = g.tensors[ts];
                        const bool can = op.nsrc == 1 && Ts.norm >= 0 && p.first_consumer[ts] == i && p.dtype == UNET_DTYPE_BF16;
                        DeepNormBwd nb;
                        if (can) {
                            const Norm& n = g.norms[Ts.norm];
                            nb = {tptr(ts), stat(Ts.norm), params[n.gamma], coef(Ts.norm), gparams[n.gamma], gparams[n.beta], Ts.act};
                        }
                        // (dry: the outcome alone, which the launch of an earlier part reported then)
                        const DgradOutcome o = conv_dgrad(p.conv[i].dgrad, op.kind == OP_CONVT, p.dtype, cg, gptr(t), at(p.wm_dgrad[i]), wd, dg, op.nsrc,
                                                          can ? &nb : nullptr, partial(), deep(), s, !dry);
                        if (o.norm_done) norm_done[ts] = 1;
                        if (o.rows > 0) { bn_tensor = ts; bn_rows = o.rows; }
                        mark(op);
                    }
                    break;
                }
                case OP_MATERIALIZE: {
                    DstGrad dg[2] = {dst_of(op.src[0]), op.nsrc > 1 ? dst_of(op.src[1]) : DstGrad()};
                    if (dg[0].ptr || (op.nsrc > 1 && dg[1].ptr)) {
                        // the materialized tensor is act(norm(src)): its gradient passes to the view of src unchanged
                        if (!dry) launch_materialize_bwd(p.dtype, gptr(t), dg, op.nsrc, g.tensors[t].voxels(), s);
                        mark(op);
                    }
                    break;
                }
                case OP_MAXPOOL: {
                    const Tensor& a = g.tensors[op.src[0]];
                    DstGrad d = dst_of(op.src[0]);
                    if (d.ptr) { if (!dry) launch_maxpool_bwd(p.dtype, src(op.src[0]), gptr(t), d, a.D, a.H, a.W, s); mark(op); }
                    break;
                }
                case OP_UPSAMPLE: {
                    const Tensor& a = g.tensors[op.src[0]];
                    DstGrad d = dst_of(op.src[0]);
                    if (d.ptr) { if (!dry) launch_upsample_bwd(p.dtype, gptr(t), d, a.D, a.H, a.W, s); mark(op); }
                    break;
                }
                case OP_PACK_INPUT:
                    if (!dry && (grad_x)) launch_unpack_ncdhw(p.dtype, gptr(t), grad_x, g.in_c, g.tensors[t].voxels(), s);
                    break;
                default: break;
            }
        }
        pending.insert(pending.begin(), held.begin(), held.end());
        held.clear();
        issue_pending();
        flush_wz(sb);
        if (sb != s) {   // join: whatever the caller enqueues next (optimizer step, next forward) sees every gradient
            HIP_OK(hipEventRecord(p.ev_join, sb));
            HIP_OK(hipStreamWaitEvent(s, p.ev_join, 0));
        }
    }
};

void check_launch() { HIP_OK(hipGetLastError()); }

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* unet_last_error(void) { return g_err.c_str(); }
void unet_set_error(const char* msg) { g_err = msg ? msg : ""; }   // comm.cpp reports through the same thread-local message

int unet_init(int* n_devices) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { if (n_devices) *n_devices = 0; return fail(std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    if (n_devices) *n_devices = n;
    return 0;
}

int unet_device_info(int device, char* name, size_t name_len, size_t* total_mem, int* compute_units, int* is_gfx950) {
    hipDeviceProp_t pr;
    hipError_t e = hipGetDeviceProperties(&pr, device);
    if (e != hipSuccess) return fail(std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (name && name_len) { std::strncpy(name, pr.name, name_len - 1); name[name_len - 1] = 0; }
    if (total_mem) *total_mem = pr.totalGlobalMem;
    if (compute_units) *compute_units = pr.multiProcessorCount;
    if (is_gfx950) *is_gfx950 = std::strncmp(pr.gcnArchName, "gfx950", 6) == 0;
    return 0;
}

static bool create_cu_range_stream(int device, int cu_first, int cu_count, hipStream_t* out);
int unet_plan_create(const char* arch, int in_c, int out_c, int D, int H, int W, int dtype, int device, int impl, unet_plan** out) {
    if (!arch || !out) return fail("unet_plan_create: null argument");
    if (dtype != UNET_DTYPE_F32 && dtype != UNET_DTYPE_BF16) return fail("unet_plan_create: unknown dtype");
    unet_plan* p = nullptr;
    try {
        p = new unet_plan();
        p->g = Graph::build(arch, in_c, out_c, D, H, W);
        // a norm's affine gradients need the gradient of the tensor it sits on, even on the network input
        for (auto& n : p->g.norms) p->g.tensors[n.tensor].needs_grad = true;
        p->dtype = dtype; p->device = device; p->impl = impl; p->elsize = dtype == UNET_DTYPE_F32 ? 4 : 2;
        p->layout();
        // loss scratch: target pyramid + partials + per-level results
        {
            size_t off = 0;
            int oc = out_c;
            for (size_t l = 0; l < p->g.outputs.size(); ++l) {
                const auto& o = p->g.outputs[l];
                int64_t S = (int64_t)(D >> l) * (H >> l) * (W >> l);
                if (S <= 0) S = 1;
                off = align_up(off + (size_t)S * 8);                               // target level l (l >= 1)
                off = align_up(off + (size_t)(4 + 2 * oc) * 4);                    // level_out
                (void)o;
            }
            off = align_up(off + (size_t)1024 * (3 + 2 * oc) * 4);                // partials (level 0 ...)
            off = align_up(off + (size_t)1024 * (3 + 2 * oc) * 4);                // ... and the coarse levels, which may run on another stream
            p->loss_bytes = off;
        }
        // sgd segment table
        std::vector<SgdSeg> segs;
        int64_t o = 0;
        for (auto& pr : p->g.params) {
            int64_t n = 1;
            for (auto d : pr.shape) n *= d;
            SgdSeg sg;
            sg.offset = o; sg.count = n; sg.wd = pr.decay ? 1.f : 0.f;
            segs.push_back(sg);
            o += n;
        }
        p->n_param_elems = o;
        p->nseg = (int)segs.size();
        int nd = 0;
        if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0) {
            DeviceGuard dg(device);
            int pr_least = 0, pr_greatest = 0;   // the side stream yields to the caller's (critical-path) stream
            (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
            // (a CU-masked side stream -- unet_plan_side_cu_range -- measured slower than occupancy politeness: profiles/r10d_ab_cu_mask.txt)
            HIP_OK(hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, pr_least));
            // the plan's events only order its two streams on ONE device: no host ever waits on them, so the system-scope fence a
            // default event performs when it is recorded (cache write-back for host visibility) is not needed
            const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
            HIP_OK(hipEventCreateWithFlags(&p->ev_fork, evf));
            HIP_OK(hipEventCreateWithFlags(&p->ev_join, evf));
            HIP_OK(hipEventCreateWithFlags(&p->ev_pack, evf));
            HIP_OK(hipEventCreateWithFlags(&p->ev_packd, evf));
            HIP_OK(hipMalloc((void**)&p->segs_dev, segs.size() * sizeof(SgdSeg)));
            HIP_OK(hipMemcpy(p->segs_dev, segs.data(), segs.size() * sizeof(SgdSeg), hipMemcpyHostToDevice));
            if (!p->wz_jobs.empty()) {
                HIP_OK(hipMalloc((void**)&p->wz_jobs_dev, p->wz_jobs.size() * sizeof(WgradReduceJob)));
                HIP_OK(hipMemcpy(p->wz_jobs_dev, p->wz_jobs.data(), p->wz_jobs.size() * sizeof(WgradReduceJob), hipMemcpyHostToDevice));
            }
            if (!p->pack_jobs.empty()) {
                HIP_OK(hipMalloc((void**)&p->jobs_dev, p->pack_jobs.size() * sizeof(PackJob)));
                HIP_OK(hipMemcpy(p->jobs_dev, p->pack_jobs.data(), p->pack_jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
            }
            if (!p->sgd_tiles.empty()) {
                HIP_OK(hipMalloc((void**)&p->tiles_dev, p->sgd_tiles.size() * sizeof(SgdTile)));
                HIP_OK(hipMemcpy(p->tiles_dev, p->sgd_tiles.data(), p->sgd_tiles.size() * sizeof(SgdTile), hipMemcpyHostToDevice));
            }
        }
        *out = p;
        return 0;
    } catch (const std::exception& e) {
        delete p;
        return fail(e.what());
    }
}

void unet_plan_destroy(unet_plan* p) { delete p; }

int unet_plan_param_count(const unet_plan* p, int* n) { *n = (int)p->g.params.size(); return 0; }
int unet_plan_param_shape(const unet_plan* p, int i, int64_t dims[5], int* ndim) {
    if (i < 0 || i >= (int)p->g.params.size()) return fail("parameter index out of range");
    const auto& s = p->g.params[i].shape;
    *ndim = (int)s.size();
    for (size_t k = 0; k < s.size(); ++k) dims[k] = s[k];
    return 0;
}
int unet_plan_param_name(const unet_plan* p, int i, char* name, size_t name_len) {
    if (i < 0 || i >= (int)p->g.params.size()) return fail("parameter index out of range");
    if (name && name_len) { std::strncpy(name, p->g.params[i].name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    return 0;
}
int unet_plan_param_decay(const unet_plan* p, int i, int* decay) {
    if (i < 0 || i >= (int)p->g.params.size()) return fail("parameter index out of range");
    *decay = p->g.params[i].decay;
    return 0;
}
int unet_plan_param_fan_in(const unet_plan* p, int i, int64_t* fan_in, int* is_norm_weight) {
    if (i < 0 || i >= (int)p->g.params.size()) return fail("parameter index out of range");
    *fan_in = p->g.params[i].fan_in; *is_norm_weight = p->g.params[i].norm_weight;
    return 0;
}
int unet_plan_buffer_count(const unet_plan* p, int* n) { *n = (int)p->g.buffers.size(); return 0; }
int unet_plan_buffer_shape(const unet_plan* p, int i, int64_t* numel) {
    if (i < 0 || i >= (int)p->g.buffers.size()) return fail("buffer index out of range");
    *numel = p->g.buffers[i];
    return 0;
}
int unet_plan_output_count(const unet_plan* p, int* n) { *n = (int)p->g.outputs.size(); return 0; }
int unet_plan_output_shape(const unet_plan* p, int l, int64_t dims[5]) {
    if (l < 0 || l >= (int)p->g.outputs.size()) return fail("output level out of range");
    const auto& o = p->g.outputs[l];
    dims[0] = 1; dims[1] = o.C; dims[2] = o.D; dims[3] = o.H; dims[4] = o.W;
    return 0;
}
int unet_plan_workspace_bytes(const unet_plan* p, size_t* bytes) { *bytes = p->ws_bytes; return 0; }
int unet_plan_flops(const unet_plan* p, double* fwd, double* bwd) { *fwd = p->g.flops_fwd; *bwd = p->g.flops_bwd; return 0; }
size_t unet_plan_describe(const unet_plan* p, char* buf, size_t len) {
    std::string d = p->g.describe();
    if (buf && len) { std::strncpy(buf, d.c_str(), len - 1); buf[len - 1] = 0; }
    return d.size() + 1;
}

int unet_forward(const unet_plan* p, const float* const* params, float* const* buffers, const float* x, float* const* outs,
                 void* workspace, int mode, void* stream) {
    try {
        if (!p || !params || !x || !workspace) throw std::runtime_error("unet_forward: null argument");
        if (mode & ~(1 | UNET_MODE_PACKS_CURRENT)) throw std::runtime_error("unet_forward: unknown mode bits (0 = eval, 1 = train, optionally | UNET_MODE_PACKS_CURRENT)");
        if (!p->g.buffers.empty() && !buffers) throw std::runtime_error("unet_forward: architecture has bnorm layers but buffers is null");
        DeviceGuard dg(p->device);
        Exec ex(*p, workspace, stream);
        ex.forward(params, buffers, x, outs, mode);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_backward(const unet_plan* p, const float* const* params, const float* const* grad_outs, float* const* grad_params,
                  float* grad_x, void* workspace, void* stream) {
    try {
        if (!p || !params || !grad_params || !workspace) throw std::runtime_error("unet_backward: null argument");
        if (grad_x) throw std::runtime_error("unet_backward: grad_x must be NULL -- dL/dx is not computed (the input carries no gradient, as in train.cpp:619-628)");
        DeviceGuard dg(p->device);
        Exec ex(*p, workspace, stream);
        ex.backward(params, grad_outs, grad_params, grad_x);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_backward_part(const unet_plan* p, const float* const* params, const float* const* grad_outs, float* const* grad_params,
                       float* grad_x, void* workspace, int op_hi, int op_lo, void* stream) {
    try {
        if (!p || !params || !grad_params || !workspace) throw std::runtime_error("unet_backward_part: null argument");
        if (op_lo < 0 || op_hi < op_lo) throw std::runtime_error("unet_backward_part: invalid op range");
        if (grad_x) throw std::runtime_error("unet_backward_part: grad_x must be NULL -- dL/dx is not computed");
        DeviceGuard dg(p->device);
        Exec ex(*p, workspace, stream);
        ex.backward(params, grad_outs, grad_params, grad_x, op_hi, op_lo);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

// Buckets of the backward for overlapping the gradient all-reduce with it: bucket k = ops [op_lo[k], op_lo[k-1]) (op_lo[-1] = number
// of ops); when it has run, the gradients of the flat parameter elements [elem_lo[k], elem_lo[k-1]) are final.  A cut is made when the
// parameters finished since the last cut reach total/(max_buckets - 0.5) elements; the last bucket ends at op 0 / element 0.
int unet_plan_backward_buckets(const unet_plan* p, int max_buckets, int* n_buckets, int* op_lo, int64_t* elem_lo) {
    try {
        if (!p || !n_buckets || !op_lo || !elem_lo || max_buckets < 1) throw std::runtime_error("unet_plan_backward_buckets: bad argument");
        const Graph& g = p->g;
        const int nops = (int)g.ops.size();
        // first flat element of the parameters an op's backward finishes (conv/conv_trans: weight, bias and the norm layer recorded
        // on its output); INT64_MAX for ops without parameters
        std::vector<int64_t> first(nops, INT64_MAX);
        bool monotone = true;
        int64_t prev = -1;
        for (int i = 0; i < nops; ++i) {
            const Op& op = g.ops[i];
            if (op.kind != OP_CONV && op.kind != OP_CONVT) continue;
            int64_t f = p->p_off[op.weight];
            if (op.bias >= 0 && p->p_off[op.bias] < f) f = p->p_off[op.bias];
            first[i] = f;
            if (f <= prev) monotone = false;
            prev = f;
            const Tensor& T = g.tensors[op.dst];
            if (T.norm >= 0) {
                const Norm& n = g.norms[T.norm];
                if (p->p_off[n.gamma] < f || p->p_off[n.beta] < f) monotone = false;   // must lie behind the conv's own parameters
            }
        }
        int nb = 0;
        if (monotone && max_buckets > 1) {
            const double thr = (double)p->n_param_elems / ((double)max_buckets - 0.5);
            int64_t hi = p->n_param_elems;
            for (int i = nops - 1; i > 0 && nb < max_buckets - 1; --i) {
                if (first[i] == INT64_MAX) continue;
                if ((double)(hi - first[i]) >= thr) { op_lo[nb] = i; elem_lo[nb] = first[i]; hi = first[i]; ++nb; }
            }
        }
        op_lo[nb] = 0; elem_lo[nb] = 0; ++nb;
        *n_buckets = nb;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_plan_op_count(const unet_plan* p, int* n) { *n = (int)p->g.ops.size(); return 0; }
int unet_plan_op_info(const unet_plan* p, int i, int* kind, int* cin, int* cout, int* ks, int* stride, int64_t in_dims[3],
                      int64_t out_dims[3], char* name, size_t name_len) {
    if (i < 0 || i >= (int)p->g.ops.size()) return fail("op index out of range");
    const Op& op = p->g.ops[i];
    if (kind) *kind = (int)op.kind;
    if (cin) *cin = op.cin;
    if (cout) *cout = op.cout;
    if (ks) *ks = op.ks;
    if (stride) *stride = op.stride;
    const Tensor* a = op.nsrc > 0 && op.src[0] >= 0 ? &p->g.tensors[op.src[0]] : nullptr;
    const Tensor* o = op.dst >= 0 ? &p->g.tensors[op.dst] : nullptr;
    if (in_dims) { in_dims[0] = a ? a->D : 0; in_dims[1] = a ? a->H : 0; in_dims[2] = a ? a->W : 0; }
    if (out_dims) { out_dims[0] = o ? o->D : 0; out_dims[1] = o ? o->H : 0; out_dims[2] = o ? o->W : 0; }
    if (name && name_len) { std::strncpy(name, op.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    return 0;
}

int unet_profile_begin(void) {
    if (g_prof) return fail("unet_profile_begin: a profile is already open on this thread");
    g_prof = new ProfSink();
    return 0;
}
int unet_profile_end(int max_records, int* op_index, int* category, float* ms, int* n_records) {
    if (!g_prof) return fail("unet_profile_end: no open profile on this thread");
    ProfSink* ps = g_prof;
    g_prof = nullptr;
    int n = 0, rc = 0;
    for (auto& r : ps->recs) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(r.e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, r.e0, r.e1);
        if (e != hipSuccess) rc = fail(std::string("unet_profile_end: ") + hipGetErrorString(e));
        if (r.op != -2 && n < max_records && op_index && category && ms) { op_index[n] = r.op; category[n] = r.cat; ms[n] = t; ++n; }
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    if (n_records) *n_records = n;
    delete ps;
    return rc;
}

int unet_loss_scratch_bytes(const unet_plan* p, size_t* bytes) { *bytes = p->loss_bytes; return 0; }

namespace {
// calc_losses + the deep-supervision loop (train.cpp:501-552,634-706) in pieces, so that a fused forward + loss can issue a level's
// kernels as soon as its head is computed, on another stream: prepare() = totals reset + target pyramid; level_partial /
// level_finish = one level.  Levels that may run concurrently must use different partial areas (`area`).
struct LossRun {
    const unet_plan* p;
    const float* const* outs; const int64_t* target; float* const* grad_outs; float* losses_out;
    int C, oc, collapse, cost_mask;
    float inv;
    std::vector<int64_t*> tgt;
    std::vector<float*> lvl;
    float* partial[2];
    LossRun(const unet_plan* plan, const float* const* outs_, const int64_t* target_, int cost_mask_, int collapse_before, float* const* grad_outs_,
            float* losses_out_, void* scratch)
        : p(plan), outs(outs_), target(target_), grad_outs(grad_outs_), losses_out(losses_out_), collapse(collapse_before), cost_mask(cost_mask_) {
        if (!p || !outs || !target || !losses_out || !scratch) throw std::runtime_error("unet_loss: null argument");
        const Graph& g = p->g;
        C = g.out_c;
        if (collapse_before < 0 || collapse_before >= C) throw std::runtime_error("invalid collapse_before");
        oc = collapse_before ? C - collapse_before + 1 : C;
        const size_t nl = g.outputs.size();
        float wsum = 0.f;
        for (size_t k = 0; k < nl; ++k) wsum += 1.0f / (float)(1 << k);
        inv = 1.0f / wsum;
        char* sc = (char*)scratch;
        size_t off = 0;
        tgt.resize(nl); lvl.resize(nl);
        for (size_t l = 0; l < nl; ++l) {
            int64_t S = (int64_t)(g.D >> l) * (g.H >> l) * (g.W >> l);
            if (S <= 0) S = 1;
            tgt[l] = (int64_t*)(sc + off); off = align_up(off + (size_t)S * 8);
            lvl[l] = (float*)(sc + off); off = align_up(off + (size_t)(4 + 2 * C) * 4);
        }
        partial[0] = (float*)(sc + off); off = align_up(off + (size_t)1024 * (3 + 2 * C) * 4);
        partial[1] = (float*)(sc + off);
        int D = g.D, H = g.H, W = g.W;
        for (size_t k = 0; k < nl; ++k) {      // the reference's run-time checks (train.cpp:651-652,664-671), before anything is launched
            if (k > 0) {
                if ((D >> 1) <= 0 || (H >> 1) <= 0 || (W >> 1) <= 0) throw std::runtime_error("deep supervision target size became zero");
                D >>= 1; H >>= 1; W >>= 1;
            }
            const auto& o = g.outputs[k];
            if (o.C == 0 || !outs[k]) throw std::runtime_error("undefined deep supervision output at level " + std::to_string(k));
            if (o.C != C)
                throw std::runtime_error("output channel mismatch at level " + std::to_string(k) + ": tensor has " + std::to_string(o.C) +
                                         ", out_count is " + std::to_string(C));
            if (o.D != D || o.H != H || o.W != W) throw std::runtime_error("deep supervision output/target size mismatch at level " + std::to_string(k));
        }
    }
    size_t levels() const { return p->g.outputs.size(); }
    const int64_t* target_of(size_t k) const { return k == 0 ? target : tgt[k]; }
    int64_t voxels(size_t k) const { const auto& o = p->g.outputs[k]; return (int64_t)o.D * o.H * o.W; }
    void prepare(hipStream_t s) {
        HIP_OK(hipMemsetAsync(losses_out, 0, 4 * sizeof(float), s));
        const Graph& g = p->g;
        int D = g.D, H = g.H, W = g.W;
        for (size_t k = 1; k < levels(); ++k) {
            launch_target_half(target_of(k - 1), tgt[k], D, H, W, s);
            D >>= 1; H >>= 1; W >>= 1;
        }
    }
    void level_partial(size_t k, int area, hipStream_t s) { launch_loss_partial(outs[k], target_of(k), C, voxels(k), collapse, partial[area], s); }
    void level_finish(size_t k, int area, hipStream_t s) {
        const float w = (1.0f / (float)(1 << k)) * inv;
        launch_loss_finalize(partial[area], loss_blocks(voxels(k)), oc, w, cost_mask, lvl[k], losses_out, k == 0, s);
        if (grad_outs && grad_outs[k]) launch_loss_grad(outs[k], target_of(k), C, voxels(k), collapse, lvl[k], w, cost_mask, grad_outs[k], s);
    }
};
}  // namespace

int unet_loss(const unet_plan* p, const float* const* outs, const int64_t* target, int cost_mask, int collapse_before,
              float* const* grad_outs, float* losses_out, void* scratch, void* stream) {
    try {
        LossRun lr(p, outs, target, cost_mask, collapse_before, grad_outs, losses_out, scratch);
        DeviceGuard dg(p->device);
        hipStream_t s = (hipStream_t)stream;
        lr.prepare(s);
        for (size_t k = 0; k < lr.levels(); ++k) { lr.level_partial(k, 0, s); lr.level_finish(k, 0, s); }
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

// unet_forward (train mode) + unet_loss in one call, which lets the loss of the coarse levels leave the critical path: the target
// pyramid is built on the plan's side stream while the encoder runs, and the loss kernels of level k >= 1 are issued there as soon as
// head k exists (the decoder's remaining levels run meanwhile on the caller's stream).  Level 0 stays on the caller's stream; its
// finalize comes after the join, so totals[0] is summed in a fixed order (levels 1.. then 0) and stays bit-reproducible.
int unet_forward_loss(const unet_plan* p, const float* const* params, float* const* buffers, const float* x, float* const* outs,
                      const int64_t* target, int cost_mask, int collapse_before, float* const* grad_outs, float* losses_out,
                      void* loss_scratch, void* workspace, void* stream) {
    return unet_forward_loss_mode(p, params, buffers, x, outs, target, cost_mask, collapse_before, grad_outs, losses_out, loss_scratch, workspace, 1,
                                  stream);
}

int unet_forward_loss_mode(const unet_plan* p, const float* const* params, float* const* buffers, const float* x, float* const* outs,
                           const int64_t* target, int cost_mask, int collapse_before, float* const* grad_outs, float* losses_out,
                           void* loss_scratch, void* workspace, int mode, void* stream) {
    try {
        if ((mode & 1) != 1 || (mode & ~(1 | UNET_MODE_PACKS_CURRENT)))
            throw std::runtime_error("unet_forward_loss_mode: mode must be 1 (train), optionally | UNET_MODE_PACKS_CURRENT");
        if (!p || !params || !x || !workspace || !outs) throw std::runtime_error("unet_forward_loss: null argument");
        if (!p->g.buffers.empty() && !buffers) throw std::runtime_error("unet_forward_loss: architecture has bnorm layers but buffers is null");
        LossRun lr(p, outs, target, cost_mask, collapse_before, grad_outs, losses_out, loss_scratch);
        DeviceGuard dg(p->device);
        hipStream_t s = (hipStream_t)stream;
        const bool side = p->side && !env().no_side_stream && !g_prof;
        Exec ex(*p, workspace, stream);
        if (!side) {
            ex.forward(params, buffers, x, outs, mode);
            lr.prepare(s);
            for (size_t k = 0; k < lr.levels(); ++k) { lr.level_partial(k, 0, s); lr.level_finish(k, 0, s); }
            check_launch();
            return 0;
        }
        hipStream_t sd = p->side;
        bool prepared = false;
        // ONE fork for all coarse levels, taken when the last of them (level 1) has its head: an event record costs the caller's stream
        // ~6 us, the coarse levels' loss kernels ~0.1 ms in all, and the full-resolution decoder level that follows (~0.25 ms) covers them
        constexpr bool per_level = false;     // (a fork per level, as in round 2, measured no faster: profiles/r07_ab_stream_knobs.txt)
        std::function<void(int)> on_head = [&](int level) {
            if (level < 1 || (size_t)level >= lr.levels()) return;
            if (!per_level && level != 1) return;
            HIP_OK(hipEventRecord(p->ev_fork, s));             // results[level..] are final on the caller's stream here (and so is `target`)
            HIP_OK(hipStreamWaitEvent(sd, p->ev_fork, 0));
            if (!prepared) { lr.prepare(sd); prepared = true; }   // not at entry: the forward's filter pack goes first on the side stream
            for (size_t k = per_level ? (size_t)level : lr.levels() - 1; k >= (size_t)level; --k) {   // coarsest first: the order of the totals' sum
                lr.level_partial(k, 1, sd);
                lr.level_finish(k, 1, sd);
            }
        };
        ex.forward(params, buffers, x, outs, mode, &on_head);
        if (!prepared) {   // a single-level architecture: nothing went to the side stream
            HIP_OK(hipEventRecord(p->ev_fork, s));
            HIP_OK(hipStreamWaitEvent(sd, p->ev_fork, 0));
            lr.prepare(sd);
        }
        lr.level_partial(0, 0, s);
        HIP_OK(hipEventRecord(p->ev_join, sd));
        HIP_OK(hipStreamWaitEvent(s, p->ev_join, 0));
        lr.level_finish(0, 0, s);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

// A stream confined to CUs [cu_first, cu_first + cu_count) of EVERY XCD (indices wrap inside the XCD).  Bit i of the HIP CU mask is CU
// i / 8 of XCD i % 8 on this part (profiles/tools/cu_mask_probe.hip); every XCD keeps at least one CU, or the driver ignores the mask.
// Such a stream is created without hipStreamNonBlocking (the API has no flags): it synchronizes with the NULL stream like any blocking stream.
static bool create_cu_range_stream(int device, int cu_first, int cu_count, hipStream_t* out) {
    hipDeviceProp_t prop;
    if (cu_count <= 0 || hipGetDeviceProperties(&prop, device) != hipSuccess || prop.multiProcessorCount % 8 != 0) return false;
    const int per_xcd = prop.multiProcessorCount / 8;
    if (cu_count >= per_xcd) return false;
    std::vector<uint32_t> mask((prop.multiProcessorCount + 31) / 32, 0u);
    for (int c = 0; c < cu_count; ++c) {
        const int cu = ((cu_first + c) % per_xcd + per_xcd) % per_xcd;
        for (int x = 0; x < 8; ++x) { const int bit = cu * 8 + x; mask[bit / 32] |= 1u << (bit % 32); }
    }
    if (hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

int unet_stream_create_cu_range(int device, int cu_first, int cu_count, void** stream) {
    try {
        if (!stream) throw std::runtime_error("unet_stream_create_cu_range: null argument");
        DeviceGuard dg(device);
        hipStream_t st = nullptr;
        if (!create_cu_range_stream(device, cu_first, cu_count, &st)) throw std::runtime_error("unet_stream_create_cu_range: the device / driver does not take this CU range");
        *stream = (void*)st;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}
int unet_stream_destroy(void* stream) {
    if (stream && hipStreamDestroy((hipStream_t)stream) != hipSuccess) return fail("hipStreamDestroy failed");
    return 0;
}
int unet_plan_side_cu_range(unet_plan* p, int cu_first, int cu_count) {
    try {
        if (!p) throw std::runtime_error("unet_plan_side_cu_range: null plan");
        if (!p->side) return 0;
        DeviceGuard dg(p->device);
        hipStream_t st = nullptr;
        if (!create_cu_range_stream(p->device, cu_first, cu_count, &st)) throw std::runtime_error("unet_plan_side_cu_range: the device / driver does not take this CU range");
        HIP_OK(hipStreamSynchronize(p->side));
        HIP_OK(hipStreamDestroy(p->side));
        p->side = st;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_pack_filters(const unet_plan* p, const float* const* params, void* workspace, int with_dgrad, int* made, void* stream) {
    try {
        if (!p || !params || !workspace || !made) throw std::runtime_error("unet_pack_filters: null argument");
        *made = 0;
        if (!p->jobs_dev || p->pack_jobs.empty() || !p->is_flat(params)) return 0;
        DeviceGuard dg(p->device);
        launch_mfma_pack_batched(params[0], workspace, p->jobs_dev, (int)p->pack_jobs.size(), with_dgrad ? p->pack_blocks : p->pack_fwd_blocks,
                                 (hipStream_t)stream, 0, 0, p->deep_part_bytes ? (int*)((char*)workspace + p->deep_cnt_off) : nullptr, p->deep_ncnt);
        check_launch();
        *made = 1;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_sum_buffers(const float* const* bufs, int n, float* out, int64_t count, int zero_inputs, void* stream) {
    try {
        if (!bufs || !out || n < 1 || n > UNET_SUM_MAX_BUFFERS || count < 0) throw std::runtime_error("unet_sum_buffers: bad argument");
        for (int k = 0; k < n; ++k)
            if (!bufs[k] || (reinterpret_cast<uintptr_t>(bufs[k]) & 15)) throw std::runtime_error("unet_sum_buffers: null or misaligned buffer");
        if (reinterpret_cast<uintptr_t>(out) & 15) throw std::runtime_error("unet_sum_buffers: misaligned output");
        if (count == 0) return 0;
        launch_sum_buffers(bufs, n, out, count, zero_inputs, (hipStream_t)stream);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_sgd_step(const unet_plan* p, float* params, float* grads, float* mom, float lr, float momentum, int nesterov, float wd,
                  float clip_norm, float grad_scale, float* norm_out, void* scratch, void* stream) {
    try {
        if (!p || !params || !grads || !mom || !scratch) throw std::runtime_error("unet_sgd_step: null argument");
        if (!p->segs_dev) throw std::runtime_error("unet_sgd_step: plan was created without a device");
        DeviceGuard dg(p->device);
        hipStream_t s = (hipStream_t)stream;
        const int nblk = 1024;           // partial sums of squares (scratch: 64 KiB)
        float* partial = (float*)scratch;
        launch_sumsq_partial(grads, p->n_param_elems, grad_scale, partial, nblk, s);
        launch_sgd(params, grads, mom, p->n_param_elems, p->segs_dev, p->nseg, partial, nblk, lr, momentum, nesterov, wd, clip_norm,
                   grad_scale, norm_out, s);
        check_launch();
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

int unet_sgd_step_packed(const unet_plan* p, float* params, float* grads, float* mom, float lr, float momentum, int nesterov, float wd,
                         float clip_norm, float grad_scale, float* norm_out, void* workspace, int with_dgrad, int* made, void* scratch,
                         void* stream) {
    try {
        if (!p || !params || !grads || !mom || !scratch || !made) throw std::runtime_error("unet_sgd_step_packed: null argument");
        *made = 0;
        if (!p->tiles_dev || !p->jobs_dev || !workspace)   // no batched pack (the fp32 engine, ...): the plain update
            return unet_sgd_step(p, params, grads, mom, lr, momentum, nesterov, wd, clip_norm, grad_scale, norm_out, scratch, stream);
        if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(mom)) & 15)
            throw std::runtime_error("unet_sgd_step_packed: misaligned buffer");
        DeviceGuard dg(p->device);
        hipStream_t s = (hipStream_t)stream;
        const int nblk = 1024;           // as unet_sgd_step
        float* partial = (float*)scratch;
        launch_sumsq_partial(grads, p->n_param_elems, grad_scale, partial, nblk, s);
        launch_sgd_pack(params, grads, mom, p->tiles_dev, (int)p->sgd_tiles.size(), p->jobs_dev, workspace, with_dgrad,
                        p->deep_part_bytes ? (int*)((char*)workspace + p->deep_cnt_off) : nullptr, p->deep_ncnt, partial, nblk, lr, momentum,
                        nesterov, wd, clip_norm, grad_scale, norm_out, s);
        check_launch();
        *made = 1;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}

// ---- single-op surface ----
// The scratch of one call: the fp32 filter copies ([forward | dgrad], `half` bytes each), the bf16 MFMA filter pack, the statistics partials
struct OpScratch {
    size_t half, pack, partials;   // byte offsets of the dgrad copy, the pack and the partials
    OpScratch(int cin, int cout)
        : half(align_up((size_t)27 * round_up(cin, 8) * round_up(cout, 8) * 4)), pack(2 * half),
          partials(pack + align_up((size_t)160 * round_up(cin, 32) * round_up(cout, 32))) {}   // largest pack: stride-2 dgrad, 128 B per Cin*Cout
};
int unet_op_scratch_bytes(int cin, int cout, int D, int H, int W, size_t* bytes) {
    size_t b = OpScratch(cin, cout).partials + 4096;
    if (D > 0 && H > 0 && W > 0) {   // statistics partials of unet_op_conv3d_fwd_fused, behind the filter packs
        int64_t S = (int64_t)D * H * W;
        size_t blocks = (size_t)(S / 32 + 4096);   // >= any conv tile count (>= 64 voxels per tile, ragged edges) and >= stats_blocks(S)
        b += align_up(blocks * cout * 2 * 8);   // fp64 partials for fp32 tensors
    }
    if ((int64_t)cin * cout <= 1024) {   // small-weight wgrad slabs: <= 1024 row blocks x <= 1024 weights, + bias partials
        size_t w = ((size_t)1024 * 1024 + (size_t)1024 * cout) * 4 + 1024;
        if (w > b) b = w;
    }
    if (cout <= 8 || cin == 1) {   // register-accumulating small wgrads: <= 512 blocks x (weights + bias sums); covers a head's backward slab
                                   // (head_bwd_scratch_bytes: the same 512 rows of one tap), which unet_op_head_bwd is given
        size_t w = (size_t)512 * ((size_t)27 * cin * cout + cout) * 4 + 1024;
        if (w > b) b = w;
    }
    if (cin % 16 == 0 && cout % 16 == 0 && D > 0 && H > 0 && W > 0) {
        ConvGeom g;   // matrix-core wgrad slabs: stride-1 geometry has the most tiles
        g.Cin = cin; g.Cout = cout; g.D = g.Do = D; g.H = g.Ho = H; g.W = g.Wo = W; g.ks = 3; g.stride = 1;
        b = std::max(b, wgrad_f32_mfma_scratch_bytes(g));   // fp32: per-wave slabs (<= 64 MB) + the bias partials
        size_t w = std::max(mfma_wgrad_scratch_bytes(g, 0), mfma_wgrad_scratch_bytes(g, 1));   // unet_op_conv3d_bwd_weight may launch politely (UNET_OP_POLITE): more slab rows
        if (w > b) b = w;
        g.stride = 2; g.Do = (D - 1) / 2 + 1; g.Ho = (H - 1) / 2 + 1; g.Wo = (W - 1) / 2 + 1;
        w = std::max(mfma_wgrad_scratch_bytes(g, 0), mfma_wgrad_scratch_bytes(g, 1));
        if (w > b) b = w;
        g.Do = 2 * D; g.Ho = 2 * H; g.Wo = 2 * W;   // conv_trans
        w = mfma_convt_wgrad_scratch_bytes(g);
        if (w > b) b = w;
    }
    *bytes = b;
    return 0;
}

static ConvGeom op_geom(int cin, int cout, int D, int H, int W, int ks, int stride, bool transposed) {
    ConvGeom g;
    g.Cin = cin; g.Cout = cout; g.D = D; g.H = H; g.W = W; g.ks = ks; g.stride = stride;
    if (transposed) { g.Do = 2 * D; g.Ho = 2 * H; g.Wo = 2 * W; }
    else {
        int pad = (ks - 1) / 2;
        g.Do = (D + 2 * pad - ks) / stride + 1; g.Ho = (H + 2 * pad - ks) / stride + 1; g.Wo = (W + 2 * pad - ks) / stride + 1;
    }
    return g;
}
static void op_pack(const float* w, int cin, int cout, int k3, bool transposed, void* scratch, float** wf, float** wd, hipStream_t s) {
    *wf = (float*)scratch; *wd = (float*)((char*)scratch + OpScratch(cin, cout).half);
    if (transposed) launch_pack_convt_w(w, *wf, *wd, cin, cout, s);
    else launch_pack_conv_w(w, *wf, *wd, cin, cout, k3, s);
}
#define OP_TRY(...) try { __VA_ARGS__; check_launch(); return 0; } catch (const std::exception& e) { return fail(e.what()); }
// the single-op surface runs the deep levels' kernels (kernels_mfma_deep.hip) as the engine does; their partial tiles and arrival counters
// live in one allocation per device, made (and cleared) on first use -- every launch leaves the counters zero.  Ops of this surface
// that use it must not run concurrently on two streams of one device (the tests and tools that call it are single-stream).
static DeepScratch op_deep() {
    static std::mutex mu;
    static std::unordered_map<int, DeepScratch> per_dev;
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = per_dev.find(dev);
    if (it != per_dev.end()) return it->second;
    DeepScratch d;
    d.part_bytes = (size_t)8 << 20; d.ncnt = 4096;
    char* base = nullptr;
    HIP_OK(hipMalloc((void**)&base, d.part_bytes + (size_t)d.ncnt * 4));
    HIP_OK(hipMemset(base + d.part_bytes, 0, (size_t)d.ncnt * 4));
    d.part = (float*)base; d.cnt = (int*)(base + d.part_bytes);
    per_dev[dev] = d;
    return d;
}
// The conv / conv_trans entries below: geometry, sources and destinations, choose_conv, the filter form the choice reads packed into
// the scratch, then the executor's own launch of that direction (conv_fwd, conv_dgrad, conv_wgrad above).
// one bf16 MFMA filter pack of a call, forward or dgrad
static void* op_pack_mfma(const float* w, const ConvGeom& g, bool transposed, bool dgrad, void* scratch, hipStream_t s) {
    void* wm = (char*)scratch + OpScratch(g.Cin, g.Cout).pack;
    if (transposed) launch_mfma_pack_convt_w(w, dgrad ? nullptr : wm, dgrad ? wm : nullptr, g, s);
    else launch_mfma_pack_conv_w(w, dgrad ? nullptr : wm, dgrad ? wm : nullptr, g, s);
    return wm;
}
// the forward of an entry; use_deep == false: no deep scratch is passed, the split-K kernels stay out
static FwdRan op_conv_fwd(const ConvChoice& c, bool transposed, int dtype, const ConvGeom& g, const SrcDesc* sd, int nsrc, const float* w,
                          const float* b, void* y, float* part, const DeepNormFwd* nf, bool use_deep, void* scratch, hipStream_t s) {
    float *wf = nullptr, *wd;
    const void* wm = nullptr;
    if (c.mfma_fwd()) wm = op_pack_mfma(w, g, transposed, false, scratch, s);
    else if (!c.param_fwd()) op_pack(w, g.Cin, g.Cout, g.ks * g.ks * g.ks, transposed, scratch, &wf, &wd, s);
    return conv_fwd(c.fwd, transposed, dtype, g, sd, nsrc, w, wf, wm, b, y, nullptr, part, nf,
                    use_deep && c.mfma_fwd() ? op_deep() : DeepScratch(), s);
}
// the input gradient of an entry, into the destinations d[0 .. ndst) (one per source of the forward; a null ptr: not wanted)
static DgradOutcome op_conv_dgrad(Dgrad c, bool transposed, int dtype, const ConvGeom& g, const void* dy, const float* w, const DstGrad* d,
                                  int ndst, const DeepNormBwd* nb, float* part, void* scratch, hipStream_t s) {
    float *wf, *wd = nullptr;
    const void* wm = nullptr;
    if (c == Dgrad::mfma) wm = op_pack_mfma(w, g, transposed, true, scratch, s);
    else op_pack(w, g.Cin, g.Cout, g.ks * g.ks * g.ks, transposed, scratch, &wf, &wd, s);
    return conv_dgrad(c, transposed, dtype, g, dy, wm, wd, d, ndst, nb, part, c == Dgrad::mfma ? op_deep() : DeepScratch(), s);
}
// the plain sources of an entry as the op reads them: c0 channels of x0, then c1 of x1 (c1 = 0: one source); returns their number
static int op_sources(const char* who, SrcDesc sd[2], const void* x0, int c0, const void* x1, int c1) {
    if (c0 < 1 || c1 < 0) throw std::runtime_error(std::string(who) + ": c0 must be positive and c1 not negative");
    sd[0].ptr = x0; sd[0].C = c0;
    if (c1) { sd[1].ptr = x1; sd[1].C = c1; }
    return c1 ? 2 : 1;
}

// what the entry points below ask choose_conv for the plain sources of c0 (+ c1) channels, as integers; launches nothing
int unet_op_conv_choice2(int dtype, int impl, int c0, int c1, int cout, int D, int H, int W, int ks, int stride, int transposed, int out[3]) {
    try {
        if (!out) throw std::runtime_error("unet_op_conv_choice: null output");
        if (c0 < 1 || c1 < 0 || cout < 1 || D < 1 || H < 1 || W < 1) throw std::runtime_error("unet_op_conv_choice: sizes must be positive");
        const int cin = c0 + c1;
        const ConvGeom g = transposed ? op_geom(cin, cout, D, H, W, 2, 2, true) : op_geom(cin, cout, D, H, W, ks, stride, false);
        SrcDesc sd[2];
        const int nsrc = op_sources("unet_op_conv_choice", sd, nullptr, c0, nullptr, c1);
        const ConvChoice c = choose_conv(dtype, impl, g, sd, nsrc, false, transposed != 0);
        out[0] = (int)c.fwd; out[1] = (int)c.dgrad; out[2] = (int)c.wgrad;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}
int unet_op_conv_choice(int dtype, int impl, int cin, int cout, int D, int H, int W, int ks, int stride, int transposed, int out[3]) {
    return unet_op_conv_choice2(dtype, impl, cin, 0, cout, D, H, W, ks, stride, transposed, out);
}

int unet_op_conv3d_fwd2(int dtype, int impl, const void* x0, int c0, const void* x1, int c1, const float* w, const float* b, void* y,
                        int cout, int D, int H, int W, int ks, int stride, void* scratch, void* stream) {
    OP_TRY({
        SrcDesc sd[2];
        const int nsrc = op_sources("unet_op_conv3d_fwd2", sd, x0, c0, x1, c1);
        ConvGeom g = op_geom(c0 + c1, cout, D, H, W, ks, stride, false);
        const ConvChoice c = choose_conv(dtype, impl, g, sd, nsrc, false, false);
        op_conv_fwd(c, false, dtype, g, sd, nsrc, w, b, y, nullptr, nullptr, true, scratch, (hipStream_t)stream);
    })
}
int unet_op_conv3d_fwd(int dtype, int impl, const void* x, const float* w, const float* b, void* y, int cin, int cout, int D, int H,
                       int W, int ks, int stride, void* scratch, void* stream) {
    return unet_op_conv3d_fwd2(dtype, impl, x, cin, nullptr, 0, w, b, y, cout, D, H, W, ks, stride, scratch, stream);
}
int unet_op_conv3d_fwd_fused(int dtype, int impl, const void* x, const float* scale, const float* shift, int act, const float* w,
                             const float* b, void* y, float* stats, int cin, int cout, int D, int H, int W, int ks, int stride,
                             void* scratch, void* stream) {
    OP_TRY({
        hipStream_t s = (hipStream_t)stream;
        ConvGeom g = op_geom(cin, cout, D, H, W, ks, stride, false);
        SrcDesc sd; sd.ptr = x; sd.C = cin; sd.scale = scale; sd.shift = shift; sd.act = act;
        int64_t So = (int64_t)g.Do * g.Ho * g.Wo;
        float* part = (float*)((char*)scratch + OpScratch(cin, cout).partials);
        ConvChoice c = choose_conv(dtype, impl, g, &sd, 1, false, false);
        if (c.fwd == Fwd::first_f32_mfma) c.fwd = Fwd::direct;   // (the fp32 first conv too: this entry runs it on the direct kernel + a statistics pass)
        // (this entry passes no deep scratch: it keeps to the kernels that leave statistics rows)
        const FwdRan r = op_conv_fwd(c, false, dtype, g, &sd, 1, w, b, y, stats ? part : nullptr, nullptr, false, scratch, s);
        if (stats && r.rows) launch_stats_sum(part, r.rows, cout, stats, s, r.dbl);
        else if (stats) {
            launch_stats_partial(dtype, y, cout, So, part, s);
            launch_stats_sum(part, stats_blocks(So), cout, stats, s, dtype == UNET_DTYPE_F32);
        }
    })
}
int unet_op_conv3d_pack(int dtype, const float* w, void* wpacked, int cin, int cout, int D, int H, int W, int ks, int stride,
                        void* stream) {
    OP_TRY({
        ConvGeom g = op_geom(cin, cout, D, H, W, ks, stride, false);
        SrcDesc sd; sd.C = cin;
        if (!choose_conv(dtype, UNET_IMPL_AUTO, g, &sd, 1, false, false).mfma_fwd())
            throw std::runtime_error("unet_op_conv3d_pack: shape not covered by the MFMA kernels");
        launch_mfma_pack_conv_w(w, wpacked, nullptr, g, (hipStream_t)stream);
    })
}
int unet_op_conv3d_fwd_packed(int dtype, const void* x, const void* wpacked, const float* b, void* y, float* stats_partials,
                              int cin, int cout, int D, int H, int W, int ks, int stride, void* stream) {
    OP_TRY({
        ConvGeom g = op_geom(cin, cout, D, H, W, ks, stride, false);
        SrcDesc sd; sd.ptr = x; sd.C = cin;
        if (!choose_conv(dtype, UNET_IMPL_AUTO, g, &sd, 1, false, false).mfma_fwd())
            throw std::runtime_error("unet_op_conv3d_fwd_packed: shape not covered by the MFMA kernels");
        launch_mfma_conv_fwd(g, &sd, 1, wpacked, b, y, stats_partials, (hipStream_t)stream);
    })
}
// The input gradient as the executor runs it for a layer with one or two sources: a destination per source, written or added to, a
// null one skipped (that source needs no gradient).
int unet_op_conv3d_bwd_data2(int dtype, int impl, int transposed, const void* dy, const float* w, void* d0, int c0, int acc0, void* d1,
                             int c1, int acc1, int cout, int D, int H, int W, int ks, int stride, void* scratch, void* stream) {
    OP_TRY({
        const bool tr = transposed != 0;
        if (tr && c1) throw std::runtime_error("unet_op_conv3d_bwd_data2: a conv_trans has one source");
        SrcDesc sd[2];
        const int nsrc = op_sources("unet_op_conv3d_bwd_data2", sd, nullptr, c0, nullptr, c1);
        if (!d0 && !(nsrc > 1 && d1)) throw std::runtime_error("unet_op_conv3d_bwd_data2: no destination");
        ConvGeom g = tr ? op_geom(c0, cout, D, H, W, 2, 2, true) : op_geom(c0 + c1, cout, D, H, W, ks, stride, false);
        DstGrad d[2];
        d[0].ptr = d0; d[0].C = c0; d[0].accumulate = acc0 ? 1 : 0;
        if (nsrc > 1) { d[1].ptr = d1; d[1].C = c1; d[1].accumulate = acc1 ? 1 : 0; }
        const ConvChoice c = choose_conv(dtype, impl, g, sd, nsrc, false, tr);
        op_conv_dgrad(c.dgrad, tr, dtype, g, dy, w, d, nsrc, nullptr, nullptr, scratch, (hipStream_t)stream);
    })
}
int unet_op_conv3d_bwd_data(int dtype, int impl, const void* dy, const float* w, void* dx, int cin, int cout, int D, int H, int W,
                            int ks, int stride, void* scratch, void* stream) {
    return unet_op_conv3d_bwd_data2(dtype, impl, 0, dy, w, dx, cin, 0, nullptr, 0, 0, cout, D, H, W, ks, stride, scratch, stream);
}
// A conv k3 and the norm + activation behind it, bf16, as the executor runs that layer (conv_fwd): on the deep levels the split-K kernel
// with the norm in its epilogue (DEEP_FWD_NORM), else the MFMA conv with its statistics rows and the norm's separate launches.
int unet_op_conv3d_fwd_norm(const void* x0, const void* x1, int cin0, int cin1, const float* w, const float* b, const float* gamma,
                            const float* beta, double eps, float* rm, float* rv, double momentum, int use_running, int act, void* y,
                            void* y_act, float* stat, int cout, int D, int H, int W, int stride, void* scratch, void* stream) {
    OP_TRY({
        hipStream_t s = (hipStream_t)stream;
        const int cin = cin0 + cin1, nsrc = x1 ? 2 : 1;
        ConvGeom g = op_geom(cin, cout, D, H, W, 3, stride, false);
        SrcDesc sd[2];
        sd[0].ptr = x0; sd[0].C = cin0;
        if (x1) { sd[1].ptr = x1; sd[1].C = cin1; }
        const ConvChoice c = choose_conv(UNET_DTYPE_BF16, UNET_IMPL_AUTO, g, sd, nsrc, false, false);
        if (!c.mfma_fwd() || (use_running && (!rm || !rv)))
            throw std::runtime_error("unet_op_conv3d_fwd_norm: shape not covered by the MFMA kernels, or eval mode without running statistics");
        float* part = (float*)((char*)scratch + OpScratch(cin, cout).partials);
        const DeepNormFwd nf = {gamma, beta, eps, stat, rm, rv, momentum, use_running ? 1 : 0, act, y_act};
        const FwdRan r = op_conv_fwd(c, false, UNET_DTYPE_BF16, g, sd, nsrc, w, b, y, use_running ? nullptr : part, &nf, true, scratch, s);
        if (!r.norm_done)
            norm_fwd_passes(UNET_DTYPE_BF16, y, cout, (int64_t)g.Do * g.Ho * g.Wo, part, r.rows, r.dbl, use_running != 0, gamma, beta, eps,
                            stat, rm, rv, act, y_act, s);
    })
}
// The dgrad of a conv k3 s1 (or of a conv_trans k2 s2: transposed) into the view of a norm layer's tensor u, then that norm's backward
// as the executor runs it (conv_dgrad): on the deep levels in the split-K kernel's epilogue (DEEP_BWD_NORM), else the dgrad (with the
// statistics epilogue where the kernel has one) and the norm's separate backward launches.
int unet_op_conv3d_bwd_data_norm_strided(int transposed, int stride, const void* dy, const float* w, void* dx, int accumulate, const void* u,
                                         const float* stat, const float* gamma, int act, float* coef, float* dgamma, float* dbeta, int cin,
                                         int cout, int D, int H, int W, void* scratch, void* stream) {
    OP_TRY({
        hipStream_t s = (hipStream_t)stream;
        if (!transposed && stride != 1 && stride != 2) throw std::runtime_error("unet_op_conv3d_bwd_data_norm: stride must be 1 or 2");
        ConvGeom g = op_geom(cin, cout, D, H, W, transposed ? 2 : 3, transposed ? 2 : stride, transposed != 0);
        SrcDesc sd; sd.C = cin;
        const ConvChoice c = choose_conv(UNET_DTYPE_BF16, UNET_IMPL_AUTO, g, &sd, 1, false, transposed != 0);
        if (c.dgrad != Dgrad::mfma) throw std::runtime_error("unet_op_conv3d_bwd_data_norm: shape not covered by the MFMA kernels");
        float* part = (float*)((char*)scratch + OpScratch(cin, cout).partials);
        DstGrad d; d.ptr = dx; d.C = cin; d.accumulate = accumulate ? 1 : 0;
        const DeepNormBwd nb = {u, stat, gamma, coef, dgamma, dbeta, act};
        const DgradOutcome o = op_conv_dgrad(c.dgrad, transposed != 0, UNET_DTYPE_BF16, g, dy, w, &d, 1, &nb, part, scratch, s);
        if (!o.norm_done) norm_bwd_passes(UNET_DTYPE_BF16, dx, u, cin, (int64_t)D * H * W, stat, act, gamma, coef, dgamma, dbeta, part, o.rows, false, s);
    })
}
int unet_op_conv3d_bwd_data_norm(int transposed, const void* dy, const float* w, void* dx, int accumulate, const void* u, const float* stat,
                                 const float* gamma, int act, float* coef, float* dgamma, float* dbeta, int cin, int cout, int D, int H,
                                 int W, void* scratch, void* stream) {
    return unet_op_conv3d_bwd_data_norm_strided(transposed, 1, dy, w, dx, accumulate, u, stat, gamma, act, coef, dgamma, dbeta, cin, cout, D, H, W,
                                                scratch, stream);
}
int unet_op_conv3d_bwd_weight2(int dtype, int impl, const void* x0, int c0, const void* x1, int c1, const void* dy, float* dw, float* db,
                               int cout, int D, int H, int W, int ks, int stride, void* scratch, void* stream) {
    OP_TRY({
        SrcDesc sd[2];
        const int nsrc = op_sources("unet_op_conv3d_bwd_weight2", sd, x0, c0, x1, c1);
        ConvGeom g = op_geom(c0 + c1, cout, D, H, W, ks, stride, false);
        const ConvChoice c = choose_conv(dtype, impl, g, sd, nsrc, false, false);
        // (the direct kernel gets no scratch from this surface: one block range, no slab; polite: UNET_OP_POLITE)
        conv_wgrad(c.wgrad, false, dtype, g, sd, nsrc, dy, dw, db, c.wgrad == Wgrad::direct ? nullptr : scratch, (hipStream_t)stream, false,
                   env().op_polite ? 1 : 0, nullptr);
    })
}
int unet_op_conv3d_bwd_weight(int dtype, int impl, const void* x, const void* dy, float* dw, float* db, int cin, int cout, int D,
                              int H, int W, int ks, int stride, void* scratch, void* stream) {
    return unet_op_conv3d_bwd_weight2(dtype, impl, x, cin, nullptr, 0, dy, dw, db, cout, D, H, W, ks, stride, scratch, stream);
}
int unet_op_convt_fwd(int dtype, int impl, const void* x, const float* w, const float* b, void* y, int cin, int cout, int D, int H,
                      int W, void* scratch, void* stream) {
    OP_TRY({
        ConvGeom g = op_geom(cin, cout, D, H, W, 2, 2, true);
        SrcDesc sd; sd.ptr = x; sd.C = cin;
        const ConvChoice c = choose_conv(dtype, impl, g, &sd, 1, false, true);
        op_conv_fwd(c, true, dtype, g, &sd, 1, w, b, y, nullptr, nullptr, true, scratch, (hipStream_t)stream);
    })
}
int unet_op_convt_bwd_data(int dtype, int impl, const void* dy, const float* w, void* dx, int cin, int cout, int D, int H, int W,
                           void* scratch, void* stream) {
    return unet_op_conv3d_bwd_data2(dtype, impl, 1, dy, w, dx, cin, 0, nullptr, 0, 0, cout, D, H, W, 2, 2, scratch, stream);
}
int unet_op_convt_bwd_weight(int dtype, int impl, const void* x, const void* dy, float* dw, float* db, int cin, int cout, int D, int H,
                             int W, void* scratch, void* stream) {
    OP_TRY({
        ConvGeom g = op_geom(cin, cout, D, H, W, 2, 2, true);
        SrcDesc sd; sd.ptr = x; sd.C = cin;
        const ConvChoice c = choose_conv(dtype, impl, g, &sd, 1, false, true);
        conv_wgrad(c.wgrad, true, dtype, g, &sd, 1, dy, dw, db, c.wgrad == Wgrad::direct ? nullptr : scratch, (hipStream_t)stream, false, 0, nullptr);
    })
}
int unet_op_pack_ndhwc(int dtype, const float* x, void* y, int C, int64_t S, void* stream) {
    OP_TRY({ launch_pack_input(dtype, x, y, C, S, (hipStream_t)stream); })
}
int unet_op_unpack_ncdhw(int dtype, const void* x, float* y, int C, int64_t S, void* stream) {
    OP_TRY({ launch_unpack_ncdhw(dtype, x, y, C, S, (hipStream_t)stream); })
}

// ---- the layer kernels of kernels_elem.hip, through the launchers the executor uses ----
static void op_layer_args(const char* who, int dtype, int C, int64_t S) {
    if ((dtype != UNET_DTYPE_F32 && dtype != UNET_DTYPE_BF16) || C < 1 || S < 1)
        throw std::runtime_error(std::string(who) + ": unknown element type, or a size that is not positive");
}
static SrcDesc op_view_src(const void* x, int C, const float* scale, const float* shift, int act) {
    if (!x || (scale == nullptr) != (shift == nullptr) || act < 0 || act > 3)
        throw std::runtime_error("single-op view: null source, scale without shift (or the reverse), or unknown activation");
    SrcDesc d;
    d.ptr = x; d.C = C; d.scale = scale; d.shift = shift; d.act = act;
    return d;
}
// A head (conv k1 s1 that writes one of the network's results) as a plan runs it: Fwd::head of choose_conv, launch_head_fwd / launch_head_bwd
// (+ launch_head_bwd_reduce) called as conv_fwd and the executor's backward call them.
static ConvGeom op_head_geom(const char* who, int dtype, int cin, int cout, int64_t S, SrcDesc* sd) {
    if (dtype != UNET_DTYPE_F32 && dtype != UNET_DTYPE_BF16) throw std::runtime_error(std::string(who) + ": unknown dtype");
    if (cin < 1 || cout < 1 || S < 1 || S > INT32_MAX) throw std::runtime_error(std::string(who) + ": sizes must be positive (S below 2^31)");
    const ConvGeom g = op_geom(cin, cout, (int)S, 1, 1, 1, 1, false);
    if (choose_conv(dtype, UNET_IMPL_AUTO, g, sd, 1, true, false).fwd != Fwd::head)
        throw std::runtime_error(std::string(who) + ": shape not covered by the head kernels (Cout <= 8, Cin 16 * 2^k <= 256)");
    return g;
}
int unet_op_head_fwd(int dtype, const void* x, int cin, const float* scale, const float* shift, int act, const float* w, const float* b,
                     void* y_cl, float* y_ncdhw, int cout, int64_t S, void* stream) {
    OP_TRY({
        if (!y_cl && !y_ncdhw) throw std::runtime_error("unet_op_head_fwd: no output");
        SrcDesc sd = op_view_src(x, cin, scale, shift, act);
        const ConvGeom g = op_head_geom("unet_op_head_fwd", dtype, cin, cout, S, &sd);
        launch_head_fwd(dtype, g, sd, w, b, y_cl, y_ncdhw, (hipStream_t)stream);
    })
}
int unet_op_head_bwd(int dtype, const void* x, int cin, const float* scale, const float* shift, int act, const float* dy_ncdhw,
                     const void* dy_cl, const float* w, void* dx, int acc, float* dw, float* db, int cout, int64_t S, int defer,
                     void* scratch, void* stream) {
    OP_TRY({
        hipStream_t s = (hipStream_t)stream;
        if ((dy_ncdhw != nullptr) == (dy_cl != nullptr)) throw std::runtime_error("unet_op_head_bwd: exactly one form of dy must be given");
        if (!dw || !db || !scratch) throw std::runtime_error("unet_op_head_bwd: dw, db and scratch must be given");
        SrcDesc sd = op_view_src(x, cin, scale, shift, act);
        const ConvGeom g = op_head_geom("unet_op_head_bwd", dtype, cin, cout, S, &sd);
        DstGrad d; d.ptr = dx; d.C = cin; d.accumulate = acc ? 1 : 0;
        launch_head_bwd(dtype, g, sd, dy_ncdhw, dy_cl, w, d, dw, db, scratch, s, defer != 0);
        if (defer) launch_head_bwd_reduce(g, dw, db, scratch, s);
    })
}
static void op_pool_dims(const char* who, int D, int H, int W) {
    // Graph::build refuses a network in which a tensor's extent becomes zero, so no plan pools an extent of 1
    if (D < 2 || H < 2 || W < 2) throw std::runtime_error(std::string(who) + ": max_pool of an extent below 2 leaves an empty tensor");
}
int unet_op_norm_fwd(int dtype, const void* raw, const float* gamma, const float* beta, double eps, float* rm, float* rv, int use_running,
                     int act, void* act_out, float* stat, int C, int64_t S, void* scratch, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_norm_fwd", dtype, C, S);
        if (!raw || !gamma || !beta || !stat || !scratch || (rm == nullptr) != (rv == nullptr) || (use_running && !rm))
            throw std::runtime_error("unet_op_norm_fwd: null argument, or eval mode without running statistics");
        norm_fwd_passes(dtype, raw, C, S, (float*)scratch, 0, false, use_running != 0, gamma, beta, eps, stat, rm, rv, act, act_out,
                        (hipStream_t)stream);
    })
}
int unet_op_norm_bwd(int dtype, void* g, const void* u, const float* stat, int act, const float* gamma, float* coef, float* dgamma,
                     float* dbeta, int C, int64_t S, void* scratch, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_norm_bwd", dtype, C, S);
        if (!g || !u || !stat || !gamma || !coef || !dgamma || !dbeta || !scratch) throw std::runtime_error("unet_op_norm_bwd: null argument");
        norm_bwd_passes(dtype, g, u, C, S, stat, act, gamma, coef, dgamma, dbeta, (float*)scratch, 0, false, (hipStream_t)stream);
    })
}
// the branches of norm_fwd_passes / norm_bwd_passes and of the launchers they call, from the launchers' own predicates (kernels.h).  How
// the two pass functions combine them is restated here (see the note above norm_fwd_passes) and must follow them.
int unet_op_norm_choice(int dtype, int C, int64_t S, int out[5]) {
    try {
        if (!out) throw std::runtime_error("unet_op_norm_choice: null output");
        op_layer_args("unet_op_norm_choice", dtype, C, S);
        const int rows = stats_blocks(S);
        const bool fused = fused_norm_ok(dtype, C, rows);
        const int separate = finalize_threads(rows) == 64 ? 1 : 2;
        const ViewCopy copy = apply_view_form(dtype, C, S);
        out[0] = fused ? 0 : separate;
        out[1] = fused ? 0 : copy == ViewCopy::vec8g ? 1 : copy == ViewCopy::vec8 ? 2 : 3;
        out[2] = !vec8_ok(dtype, C) ? 2 : C / 8 <= STATS8_SHUFFLE_MAX_G8 ? 0 : 1;
        out[3] = fused ? 0 : separate;
        out[4] = fused ? 0 : vec8_ok(dtype, C) ? 1 : 2;
        return 0;
    } catch (const std::exception& e) { return fail(e.what()); }
}
int unet_op_view(int dtype, const void* x0, int c0, const float* scale0, const float* shift0, int act0, const void* x1, int c1,
                 const float* scale1, const float* shift1, int act1, void* out, int64_t S, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_view", dtype, c0, S);
        if (!out || c1 < 0 || (x1 == nullptr) != (c1 == 0)) throw std::runtime_error("unet_op_view: null output, or a second source without channels");
        SrcDesc sd[2];
        sd[0] = op_view_src(x0, c0, scale0, shift0, act0);
        if (x1) sd[1] = op_view_src(x1, c1, scale1, shift1, act1);
        launch_materialize(dtype, sd, x1 ? 2 : 1, out, S, (hipStream_t)stream);
    })
}
int unet_op_view_bwd(int dtype, const void* gout, void* d0, int c0, int acc0, void* d1, int c1, int acc1, int64_t S, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_view_bwd", dtype, c0, S);
        if (!gout || c1 < 0 || (d1 && !c1)) throw std::runtime_error("unet_op_view_bwd: null gradient, or a second destination without channels");
        DstGrad dg[2];
        dg[0].ptr = d0; dg[0].C = c0; dg[0].accumulate = acc0 ? 1 : 0;
        dg[1].ptr = d1; dg[1].C = c1; dg[1].accumulate = acc1 ? 1 : 0;
        launch_materialize_bwd(dtype, gout, dg, c1 ? 2 : 1, S, (hipStream_t)stream);
    })
}
int unet_op_apply_view(int dtype, const void* x, int C, const float* scale, const float* shift, int act, void* out, int64_t S,
                       void* stream) {
    OP_TRY({
        op_layer_args("unet_op_apply_view", dtype, C, S);
        if (!out) throw std::runtime_error("unet_op_apply_view: null output");
        launch_apply_view(dtype, op_view_src(x, C, scale, shift, act), out, S, (hipStream_t)stream);
    })
}
int unet_op_act_bwd(int dtype, void* g, const void* u, int act, int64_t n, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_act_bwd", dtype, 1, n);
        if (!g || !u || act < 0 || act > 3) throw std::runtime_error("unet_op_act_bwd: null argument or unknown activation");
        launch_act_bwd(dtype, g, u, act, n, (hipStream_t)stream);
    })
}
int unet_op_maxpool_fwd(int dtype, const void* x, int C, const float* scale, const float* shift, int act, void* out, int D, int H, int W,
                        void* stream) {
    OP_TRY({
        op_layer_args("unet_op_maxpool_fwd", dtype, C, 1);
        op_pool_dims("unet_op_maxpool_fwd", D, H, W);
        if (!out) throw std::runtime_error("unet_op_maxpool_fwd: null output");
        launch_maxpool_fwd(dtype, op_view_src(x, C, scale, shift, act), out, D, H, W, (hipStream_t)stream);
    })
}
int unet_op_maxpool_bwd(int dtype, const void* x, int C, const float* scale, const float* shift, int act, const void* gout, void* dx,
                        int accumulate, int D, int H, int W, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_maxpool_bwd", dtype, C, 1);
        op_pool_dims("unet_op_maxpool_bwd", D, H, W);
        if (!gout || !dx) throw std::runtime_error("unet_op_maxpool_bwd: null gradient");
        DstGrad d; d.ptr = dx; d.C = C; d.accumulate = accumulate ? 1 : 0;
        launch_maxpool_bwd(dtype, op_view_src(x, C, scale, shift, act), gout, d, D, H, W, (hipStream_t)stream);
    })
}
int unet_op_upsample_fwd(int dtype, const void* x, int C, const float* scale, const float* shift, int act, void* out, int D, int H, int W,
                         void* stream) {
    OP_TRY({
        op_layer_args("unet_op_upsample_fwd", dtype, C, (int64_t)D * H * W);
        if (D < 1 || H < 1 || W < 1 || !out) throw std::runtime_error("unet_op_upsample_fwd: null output, or a size that is not positive");
        launch_upsample_fwd(dtype, op_view_src(x, C, scale, shift, act), out, D, H, W, (hipStream_t)stream);
    })
}
int unet_op_upsample_bwd(int dtype, const void* gout, void* dx, int C, int accumulate, int D, int H, int W, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_upsample_bwd", dtype, C, (int64_t)D * H * W);
        if (D < 1 || H < 1 || W < 1 || !gout || !dx) throw std::runtime_error("unet_op_upsample_bwd: null gradient, or a size that is not positive");
        DstGrad d; d.ptr = dx; d.C = C; d.accumulate = accumulate ? 1 : 0;
        launch_upsample_bwd(dtype, gout, d, D, H, W, (hipStream_t)stream);
    })
}
int unet_op_export_view(int dtype, const void* x, int C, const float* scale, const float* shift, int act, float* y, int64_t S,
                        void* stream) {
    OP_TRY({
        op_layer_args("unet_op_export_view", dtype, C, S);
        if (!y) throw std::runtime_error("unet_op_export_view: null output");
        launch_export(dtype, op_view_src(x, C, scale, shift, act), y, S, (hipStream_t)stream);
    })
}
int unet_op_import_grad(int dtype, const float* g, void* o, int C, int64_t S, int accumulate, void* stream) {
    OP_TRY({
        op_layer_args("unet_op_import_grad", dtype, C, S);
        if (!g || !o) throw std::runtime_error("unet_op_import_grad: null argument");
        launch_import_grad(dtype, g, o, C, S, accumulate ? 1 : 0, (hipStream_t)stream);
    })
}


// ---- on-GPU sample augmentation (include/unet_augment.h) ----
static const char* augment_recipe_error(const UnetAugmentRecipe* r) {
    if (!r) return "unet_augment: null recipe";
    for (int d = 0; d < 3; ++d)
        if (r->dims[d] < 1) return "unet_augment: dims must be positive";
    if (r->channels < 1 || r->channels > UNET_AUG_MAX_CHANNELS) return "unet_augment: channels out of range (1..UNET_AUG_MAX_CHANNELS)";
    if (r->n_foci < 0 || r->n_foci > UNET_AUG_MAX_FOCI) return "unet_augment: n_foci out of range (0..UNET_AUG_MAX_FOCI)";
    if (r->trunc_top < 0 || r->trunc_bottom < 0) return "unet_augment: negative truncation";
    if (r->downsample)
        for (int d = 0; d < 3; ++d)
            if (r->low_dims[d] < 1 || r->low_dims[d] > r->dims[d]) return "unet_augment: low_dims must be in 1..dims";
    for (int k = 0; k < r->n_foci; ++k)
        if (!(r->foci_radius[k] > 0.f)) return "unet_augment: distortion radius must be positive";
    return nullptr;
}
int unet_augment_scratch_bytes(const UnetAugmentRecipe* recipe, size_t* bytes) {
    if (const char* e = augment_recipe_error(recipe)) return fail(e);
    if (!bytes) return fail("unet_augment_scratch_bytes: null output");
    *bytes = augment_scratch_bytes(*recipe);
    return 0;
}
int unet_augment_run(const UnetAugmentRecipe* recipe, float* image, float* label, void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = augment_recipe_error(recipe)) return fail(e);
    if (!image || !label || !scratch) return fail("unet_augment_run: null device pointer");
    if (scratch_bytes < augment_scratch_bytes(*recipe)) return fail("unet_augment_run: scratch too small (see unet_augment_scratch_bytes)");
    OP_TRY({
        // the volumes' device is the one to launch on, whatever the calling thread's current device is
        hipPointerAttribute_t at;
        HIP_OK(hipPointerGetAttributes(&at, image));
        DeviceGuard guard(at.device);
        launch_augment(*recipe, image, label, scratch, (hipStream_t)stream);
    })
}

// ---- simulate_modality (include/unet_augment.h) ----
static const char* simulate_recipe_error(const UnetSimulateRecipe* r) {
    if (!r) return "unet_simulate_modality: null recipe";
    for (int d = 0; d < 3; ++d)
        if (r->dims[d] < 1) return "unet_simulate_modality: dims must be positive";
    if (r->with_label && (r->max_label < 0 || r->max_label >= UNET_SIM_MAX_LABELS)) return "unet_simulate_modality: max_label out of range";
    for (int k = 0; k < UNET_SIM_TERMS; ++k)
        if (r->term_a[k] > 3 || r->term_b[k] > 3 || r->term_c[k] > 3 || r->term_d[k] > 3) return "unet_simulate_modality: exponents must be 0..3";
    return nullptr;
}
int unet_simulate_modality_scratch_bytes(const UnetSimulateRecipe* recipe, size_t* bytes) {
    if (const char* e = simulate_recipe_error(recipe)) return fail(e);
    if (!bytes) return fail("unet_simulate_modality_scratch_bytes: null output");
    *bytes = simulate_scratch_bytes(*recipe);
    return 0;
}
int unet_simulate_modality_run(const UnetSimulateRecipe* recipe, float* t1w, const float* label, void* scratch, size_t scratch_bytes,
                               void* stream) {
    if (const char* e = simulate_recipe_error(recipe)) return fail(e);
    if (!t1w || !scratch || (recipe->with_label && !label)) return fail("unet_simulate_modality_run: null device pointer");
    if (scratch_bytes < simulate_scratch_bytes(*recipe)) return fail("unet_simulate_modality_run: scratch too small");
    OP_TRY({
        hipPointerAttribute_t at;
        HIP_OK(hipPointerGetAttributes(&at, t1w));
        DeviceGuard guard(at.device);
        launch_simulate_modality(*recipe, t1w, label, scratch, (hipStream_t)stream);
    })
}

// ---- quality control counts (include/unet_qc.h) ----
static const char* qc_args_error(int out_c, int64_t voxels, int collapse_before) {
    if (out_c < 1) return "unet_qc: out_c must be positive";
    if (collapse_before < 0 || collapse_before >= out_c) return "invalid collapse_before";   // qc.cpp:73-74
    if (voxels <= 0) return "unet_qc: voxels must be positive";
    if (voxels > ((int64_t)1 << 40)) return "unet_qc: too many voxels";   // the per-block partial counts are 32-bit
    return nullptr;
}
int unet_qc_scratch_bytes(int out_c, int64_t voxels, int collapse_before, size_t* bytes) {
    if (const char* e = qc_args_error(out_c, voxels, collapse_before)) return fail(e);
    if (!bytes) return fail("unet_qc_scratch_bytes: null output");
    *bytes = qc_scratch_bytes(out_c, voxels, collapse_before);
    return 0;
}
int unet_qc_counts(const float* logits, const float* label, const float* image0, int out_c, int64_t voxels, int collapse_before,
                   int shift_by, uint64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = qc_args_error(out_c, voxels, collapse_before)) return fail(e);
    if (!logits || !label || !counts || !scratch) return fail("unet_qc_counts: null device pointer");
    if (shift_by < 0) return fail("unet_qc_counts: shift_by must not be negative");
    if (shift_by > 0 && !image0) return fail("unet_qc_counts: shift_by > 0 needs image0");
    if (scratch_bytes < qc_scratch_bytes(out_c, voxels, collapse_before)) return fail("unet_qc_counts: scratch too small (see unet_qc_scratch_bytes)");
    OP_TRY({
        hipPointerAttribute_t at;
        HIP_OK(hipPointerGetAttributes(&at, logits));
        DeviceGuard guard(at.device);
        launch_qc_counts(logits, label, image0, out_c, voxels, collapse_before, shift_by, counts, scratch, (hipStream_t)stream);
    })
}

// ---- template/subject training feed (include/unet_feed.h) ----
static const char* feed_args_error(const void* label, int64_t voxels, const void* scratch, size_t scratch_bytes) {
    if (voxels <= 0) return "unet_feed: voxels must be positive";
    if (!label || !scratch) return "unet_feed: null device pointer";
    if (scratch_bytes < feed_scratch_bytes(voxels)) return "unet_feed: scratch too small (see unet_feed_scratch_bytes)";
    return nullptr;
}
#define FEED_ON_DEVICE_OF(ptr, ...)                \
    OP_TRY({                                       \
        hipPointerAttribute_t at;                  \
        HIP_OK(hipPointerGetAttributes(&at, ptr)); \
        DeviceGuard guard(at.device);              \
        __VA_ARGS__;                               \
    })
int unet_feed_scratch_bytes(int64_t voxels, size_t* bytes) {
    if (voxels <= 0) return fail("unet_feed: voxels must be positive");
    if (!bytes) return fail("unet_feed_scratch_bytes: null output");
    *bytes = feed_scratch_bytes(voxels);
    return 0;
}
int unet_feed_label_max(const float* label, int64_t voxels, int32_t* out_max, void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = feed_args_error(label, voxels, scratch, scratch_bytes)) return fail(e);
    if (!out_max) return fail("unet_feed_label_max: null output");
    FEED_ON_DEVICE_OF(label, launch_feed_label_max(label, voxels, (int*)out_max, scratch, (hipStream_t)stream));
}
int unet_feed_prepare(const float* image0, float* label, int64_t voxels, int normalize, int shift_by, int32_t* label_max,
                      void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = feed_args_error(label, voxels, scratch, scratch_bytes)) return fail(e);
    if (shift_by < 0) return fail("unet_feed_prepare: shift_by must not be negative");
    if (shift_by > 0 && !image0) return fail("unet_feed_prepare: shift_by > 0 needs image0");
    FEED_ON_DEVICE_OF(label, launch_feed_prepare(image0, label, voxels, normalize, shift_by, (int*)label_max, scratch, (hipStream_t)stream));
}
int unet_feed_target(const float* label, int64_t voxels, int normalize, int64_t* target, void* scratch, size_t scratch_bytes,
                     void* stream) {
    if (const char* e = feed_args_error(label, voxels, scratch, scratch_bytes)) return fail(e);
    if (!target) return fail("unet_feed_target: null device pointer");
    FEED_ON_DEVICE_OF(label, launch_feed_target(label, voxels, normalize, target, scratch, (hipStream_t)stream));
}
int unet_feed_schedule(uint64_t seed, int batch_size, int n_template, int n_subject, int64_t first, int64_t count, int32_t* out_case,
                       int32_t* out_is_template) {
    if (batch_size < 1) return fail("unet_feed_schedule: batch_size must be positive");
    if (n_template < 0 || n_subject < 0 || n_template + n_subject == 0) return fail("unet_feed_schedule: no cases");
    if (first < 0 || count < 0) return fail("unet_feed_schedule: first and count must not be negative");
    if (count && (!out_case || !out_is_template)) return fail("unet_feed_schedule: null output");
    // train.cpp:391-401, with the library's own engine and distributions: the draws are the reference's for a given seed
    std::uniform_int_distribution<int> template_gen(0, std::max<int>(1, n_template) - 1);
    std::uniform_int_distribution<int> non_template_gen(0, std::max<int>(1, n_subject) - 1);
    std::mt19937 gen(seed);
    for (int64_t seed_id = 0; seed_id < first + count; ++seed_id) {
        const bool use_template = n_subject == 0 || seed_id % batch_size < n_template;
        const int c = use_template ? template_gen(gen) : non_template_gen(gen);
        if (seed_id < first) continue;
        out_case[seed_id - first] = c;
        out_is_template[seed_id - first] = use_template ? 1 : 0;
    }
    return 0;
}

// ---- inference post-processing chain (include/unet_postproc.h) ----
static const char* pp_class_error(int out_c, int64_t voxels) {
    if (out_c < 2) return "unet_postproc: out_c must be at least 2 (channel 0 is the background)";
    if (out_c - 1 > 65535) return "unet_postproc: more than 65535 foreground classes do not fit a uint16 label";
    if (voxels <= 0) return "unet_postproc: voxels must be positive";
    return nullptr;
}
static const char* pp_volume_error(int w, int h, int d, int n_planes, void* scratch, size_t scratch_bytes) {
    if (w <= 0 || h <= 0 || d <= 0) return "unet_postproc: volume dimensions must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31) || d > 65535 || h > 4 * 65535)
        return "unet_postproc: volume beyond 2^31 voxels, 65535 slices or 4 x 65535 rows";
    if (n_planes < 0 || n_planes > 65535) return "unet_postproc: n_planes must be in [0, 65535]";
    if (!scratch) return "unet_postproc: null scratch";
    if (scratch_bytes < postproc_scratch_bytes(n_planes, (int64_t)w * h * d))
        return "unet_postproc: scratch too small (see unet_postproc_scratch_bytes)";
    return nullptr;
}
int unet_postproc_scratch_bytes(int out_c, int64_t voxels, size_t* bytes) {
    if (const char* e = pp_class_error(out_c, voxels)) return fail(e);
    if (!bytes) return fail("unet_postproc_scratch_bytes: null output");
    *bytes = postproc_scratch_bytes(out_c - 1, voxels);
    return 0;
}
int unet_postproc_softmax(const float* logits, int out_c, int64_t voxels, float threshold, float* label_prob, float* fg_prob,
                          uint16_t* label, void* stream) {
    if (const char* e = pp_class_error(out_c, voxels)) return fail(e);
    if (!logits) return fail("unet_postproc_softmax: null logits");
    if (!label_prob && !fg_prob && !label) return fail("unet_postproc_softmax: no output wanted");
    return run_on_device_of(logits, stream, [&](hipStream_t s) {
        launch_postproc_softmax(logits, out_c, voxels, threshold, label_prob, fg_prob, label, s);
    });
}
int unet_postproc_argmax_planes(const float* label_prob, int n_planes, int64_t voxels, const float* fg_prob, float threshold,
                                uint16_t* label, void* stream) {
    if (const char* e = pp_class_error(n_planes + 1, voxels)) return fail(e);
    if (!label_prob || !fg_prob || !label) return fail("unet_postproc_argmax_planes: null device pointer");
    return run_on_device_of(label_prob, stream, [&](hipStream_t s) {
        launch_postproc_argmax_planes(label_prob, n_planes, voxels, fg_prob, threshold, label, s);
    });
}
int unet_postproc_defragment(int w, int h, int d, int each, float threshold, double size_ratio, float* fg_prob, float* label_prob,
                             int n_planes, uint16_t* label, void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = pp_volume_error(w, h, d, each ? n_planes : 1, scratch, scratch_bytes)) return fail(e);
    if (n_planes < 0 || n_planes > 65535) return fail("unet_postproc: n_planes must be in [0, 65535]");
    if (each && (!label_prob || n_planes < 1)) return fail("unet_postproc_defragment: defragment_each needs label_prob planes");
    if (!each && !fg_prob) return fail("unet_postproc_defragment: defragment needs fg_prob (create_mask)");
    if (label_prob && n_planes < 1 && !each) return fail("unet_postproc_defragment: label_prob given with no planes");
    if (!(size_ratio == size_ratio)) return fail("unet_postproc_defragment: size_ratio is NaN");
    return run_on_device_of(each ? label_prob : fg_prob, stream, [&](hipStream_t s) {
        launch_postproc_defragment(w, h, d, each, threshold, size_ratio, fg_prob, each ? label_prob : (n_planes ? label_prob : nullptr),
                                   n_planes, each ? nullptr : label, scratch, s);
    });
}
int unet_postproc_plane_op(int op, float param, int w, int h, int d, float* label_prob, int n_planes, void* scratch,
                           size_t scratch_bytes, void* stream) {
    if (op < UNET_PP_UPPER_THRESHOLD || op > UNET_PP_SMOOTH) return fail("unet_postproc_plane_op: unknown op " + std::to_string(op));
    if (const char* e = pp_volume_error(w, h, d, n_planes, scratch, scratch_bytes)) return fail(e);
    if (!label_prob || n_planes < 1) return fail("unet_postproc_plane_op: no label_prob planes");
    return run_on_device_of(label_prob, stream, [&](hipStream_t s) { launch_postproc_plane_op(op, param, w, h, d, label_prob, n_planes, scratch, s); });
}

// ---- between a scan's grid and the model's (include/unet_space.h) ----
static const char* space_grid_error(int w, int h, int d) {
    if (w <= 0 || h <= 0 || d <= 0) return "unet_space: volume dimensions must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31) || space_bricks(w, h, d) > ((int64_t)1 << 30))
        return "unet_space: a grid must stay below 2^31 voxels (and 2^30 bricks of 16 x 4 x 4)";
    return nullptr;
}
int unet_space_scratch_bytes(int64_t dst_voxels, int channels, size_t* bytes) {
    if (dst_voxels <= 0 || dst_voxels >= ((int64_t)1 << 31)) return fail("unet_space: dst_voxels must be in [1, 2^31)");
    if (channels <= 0) return fail("unet_space: channels must be positive");
    if (!bytes) return fail("unet_space_scratch_bytes: null output");
    *bytes = space_scratch_bytes(dst_voxels, channels);
    return 0;
}
int unet_space_resample(const float* src, int sw, int sh, int sd, float* dst, int dw, int dh, int dd, int channels,
                        const UnetSpaceMap* map, int mode, int normalize, void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = space_grid_error(sw, sh, sd)) return fail(e);
    if (const char* e = space_grid_error(dw, dh, dd)) return fail(e);
    if (channels <= 0) return fail("unet_space: channels must be positive");
    if (!src || !dst) return fail("unet_space_resample: null device pointer");
    if (!map) return fail("unet_space_resample: null map");
    if (mode != UNET_SPACE_LINEAR && mode != UNET_SPACE_MAJORITY) return fail("unet_space_resample: unknown mode " + std::to_string(mode));
    if (normalize && mode != UNET_SPACE_LINEAR) return fail("unet_space_resample: normalize goes with UNET_SPACE_LINEAR only");
    if (normalize && !scratch) return fail("unet_space_resample: normalize needs scratch");
    if (normalize && scratch_bytes < space_scratch_bytes((int64_t)dw * dh * dd, channels))
        return fail("unet_space_resample: scratch too small (see unet_space_scratch_bytes)");
    const UnetSpaceMap m = *map;
    return run_on_device_of(dst, stream, [&](hipStream_t s) {
        launch_space_resample(src, sw, sh, sd, dst, dw, dh, dd, channels, m, mode, normalize, scratch, s);
    });
}
int unet_space_postproc(const float* logits, int out_c, int mw, int mh, int md, const UnetSpaceMap* map, int nw, int nh, int nd,
                        float threshold, float* label_prob, float* fg_prob, uint16_t* label, void* stream) {
    if (const char* e = pp_class_error(out_c, 1)) return fail(e);
    if (const char* e = space_grid_error(mw, mh, md)) return fail(e);
    if (const char* e = space_grid_error(nw, nh, nd)) return fail(e);
    if (!logits) return fail("unet_space_postproc: null logits");
    if (!map) return fail("unet_space_postproc: null map");
    if (!label_prob && !fg_prob && !label) return fail("unet_space_postproc: no output wanted");
    const UnetSpaceMap m = *map;
    return run_on_device_of(logits, stream, [&](hipStream_t s) {
        launch_space_postproc(logits, out_c, mw, mh, md, m, nw, nh, nd, threshold, label_prob, fg_prob, label, s);
    });
}

// ---- a scan larger than the model's field of view, in blended tiles (include/unet_tiles.h) ----
static std::string tiles_args_error(const char* who, const void* tiles, int out_c, int tw, int th, int td, const UnetTilePlan* plan, int cw,
                                    int ch, int cd) {
    const std::string w = std::string(who) + ": ";
    if (!tiles) return w + "null tiles";
    if (!plan) return w + "null plan";
    if (out_c < 2) return w + "out_c must be at least 2 (channel 0 is the background)";
    if (out_c > 65536) return w + "more than 65535 foreground classes do not fit a uint16 label";
    if (tw <= 0 || th <= 0 || td <= 0) return w + "tile dimensions must be positive";
    if (tw > UNET_TILES_MAX_DIM || th > UNET_TILES_MAX_DIM || td > UNET_TILES_MAX_DIM)
        return w + "a tile dimension above " + std::to_string(UNET_TILES_MAX_DIM) + " (the weights must stay exact in fp32)";
    if (cw <= 0 || ch <= 0 || cd <= 0) return w + "canvas dimensions must be positive";
    if ((int64_t)cw * ch * cd >= ((int64_t)1 << 31) || space_bricks(cw, ch, cd) > ((int64_t)1 << 30))
        return w + "the canvas must stay below 2^31 voxels (and 2^30 bricks of 16 x 4 x 4)";
    const int t[3] = {tw, th, td}, c[3] = {cw, ch, cd};
    for (int a = 0; a < 3; ++a) {
        const std::string ax = w + "axis " + "xyz"[a] + ": ";
        const int n = plan->n[a];
        const int* o = plan->origin[a];
        if (n < 1 || n > UNET_TILES_MAX_AXIS) return ax + "n must be in [1, " + std::to_string(UNET_TILES_MAX_AXIS) + "], got " + std::to_string(n);
        if (o[0] != 0) return ax + "the first origin must be 0";
        if (o[n - 1] != c[a] - t[a]) return ax + "the last origin must be canvas - tile = " + std::to_string(c[a] - t[a]);
        for (int i = 1; i < n; ++i) {
            if (o[i] <= o[i - 1]) return ax + "the origins must ascend";
            if (o[i] - o[i - 1] > t[a]) return ax + "a gap between tiles " + std::to_string(i - 1) + " and " + std::to_string(i);
        }
    }
    return std::string();
}
int unet_tiles_blend(const float* tiles, int out_c, int tw, int th, int td, const UnetTilePlan* plan, int cw, int ch, int cd,
                     float* canvas, void* stream) {
    const std::string e = tiles_args_error("unet_tiles_blend", tiles, out_c, tw, th, td, plan, cw, ch, cd);
    if (!e.empty()) return fail(e);
    if (!canvas) return fail("unet_tiles_blend: null canvas");
    const UnetTilePlan p = *plan;
    return run_on_device_of(tiles, stream, [&](hipStream_t s) { launch_tiles_blend(tiles, out_c, tw, th, td, p, cw, ch, cd, canvas, s); });
}
int unet_tiles_postproc(const float* tiles, int out_c, int tw, int th, int td, const UnetTilePlan* plan, int cw, int ch, int cd,
                        float threshold, float* label_prob, float* fg_prob, uint16_t* label, void* stream) {
    const std::string e = tiles_args_error("unet_tiles_postproc", tiles, out_c, tw, th, td, plan, cw, ch, cd);
    if (!e.empty()) return fail(e);
    if (!label_prob && !fg_prob && !label) return fail("unet_tiles_postproc: no output wanted");
    const UnetTilePlan p = *plan;
    return run_on_device_of(tiles, stream, [&](hipStream_t s) {
        launch_tiles_postproc(tiles, out_c, tw, th, td, p, cw, ch, cd, threshold, label_prob, fg_prob, label, s);
    });
}

// ---- the patch feed: training windows cut out of a canvas larger than the field of view (include/unet_patches.h) ----
static std::string patches_class_error(const std::string& w, int64_t voxels, int classes) {
    if (voxels <= 0) return w + "voxels must be positive";
    if (voxels >= ((int64_t)1 << 31)) return w + "the canvas must stay below 2^31 voxels";
    if (classes < 0 || classes > UNET_PATCHES_MAX_CLASSES)
        return w + "classes must be in [0, " + std::to_string(UNET_PATCHES_MAX_CLASSES) + "], got " + std::to_string(classes);
    return std::string();
}
static std::string patches_window_error(const std::string& w, int W, int H, int D, int tw, int th, int td) {
    if (W <= 0 || H <= 0 || D <= 0) return w + "canvas dimensions must be positive";
    if (tw <= 0 || th <= 0 || td <= 0) return w + "window dimensions must be positive";
    if ((int64_t)W * H * D >= ((int64_t)1 << 31)) return w + "the canvas must stay below 2^31 voxels";
    if (tw > W || th > H || td > D) return w + "the window must fit the canvas (no padding)";
    return std::string();
}
int unet_patches_index_bytes(int64_t voxels, int classes, size_t* bytes) {
    const std::string e = patches_class_error("unet_patches_index_bytes: ", voxels, classes);
    if (!e.empty()) return fail(e);
    if (!bytes) return fail("unet_patches_index_bytes: null output");
    *bytes = patches_index_bytes(voxels, classes ? classes : 2);
    return 0;
}
int unet_patches_index(const float* label, int64_t voxels, int classes, int32_t* index, size_t index_bytes, void* stream) {
    const std::string e = patches_class_error("unet_patches_index: ", voxels, classes);
    if (!e.empty()) return fail(e);
    if (!label || !index) return fail("unet_patches_index: null device pointer");
    if (index_bytes < patches_index_bytes(voxels, classes ? classes : 2)) return fail("unet_patches_index: index too small (see unet_patches_index_bytes)");
    return run_on_device_of(label, stream, [&](hipStream_t s) { launch_patches_index(label, voxels, classes, index, s); });
}
int unet_patches_pick(const float* label, const int32_t* index, int classes, int W, int H, int D, int tw, int th, int td,
                      const UnetPatchPick* picks, int n, int32_t* origins, void* stream) {
    const std::string w = "unet_patches_pick: ";
    std::string e = patches_window_error(w, W, H, D, tw, th, td);
    if (e.empty()) e = patches_class_error(w, (int64_t)W * H * D, classes);
    if (!e.empty()) return fail(e);
    if (!label || !index || !origins) return fail(w + "null device pointer");
    if (n < 1 || n > UNET_PATCHES_MAX_PICKS) return fail(w + "n must be in [1, " + std::to_string(UNET_PATCHES_MAX_PICKS) + "], got " + std::to_string(n));
    if (!picks) return fail(w + "null picks");
    return run_on_device_of(label, stream, [&](hipStream_t s) { launch_patches_pick(label, index, classes, W, H, D, tw, th, td, picks, n, origins, s); });
}
int unet_patches_crop(const float* image, int channels, const float* label, int W, int H, int D, int tw, int th, int td,
                      const int32_t* origin, float* x, float* lab, void* stream) {
    const std::string w = "unet_patches_crop: ";
    const std::string e = patches_window_error(w, W, H, D, tw, th, td);
    if (!e.empty()) return fail(e);
    if (channels < 1 || channels > 65534) return fail(w + "channels must be in [1, 65534], got " + std::to_string(channels));
    if (td > 65535) return fail(w + "a window of more than 65535 slices");
    if (!image || !x || !origin) return fail(w + "null device pointer");
    if (lab && !label) return fail(w + "lab without a label to cut it from");
    return run_on_device_of(image, stream, [&](hipStream_t s) { launch_patches_crop(image, channels, label, W, H, D, tw, th, td, origin, x, lab, s); });
}
int unet_patches_draws(uint64_t seed, uint64_t index, uint32_t first_k, int count, uint32_t* out) {
    if (count < 0) return fail("unet_patches_draws: count must not be negative");
    if (count && !out) return fail("unet_patches_draws: null output");
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    auto mix = [](uint64_t z) {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const uint64_t base = mix(mix(seed + G) ^ index);
    for (int i = 0; i < count; ++i) out[i] = (uint32_t)(mix(base + ((uint64_t)first_k + (uint64_t)i + 1) * G) >> 32);
    return 0;
}

// ---- test-time mirroring: the members' logits flipped back, swapped back and averaged (include/unet_mirror.h) ----
static std::string mirror_args_error(const char* who, const void* stack, int out_c, int w, int h, int d, int n_members, const int* masks,
                                     int swap_axis, const int* pairs, int n_pairs) {
    const std::string e = std::string(who) + ": ";
    if (!stack) return e + "null stack";
    if (out_c < 2) return e + "out_c must be at least 2 (channel 0 is the background)";
    if (out_c > 65536) return e + "more than 65535 foreground classes do not fit a uint16 label";
    if (w <= 0 || h <= 0 || d <= 0) return e + "volume dimensions (w, h, d) must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return e + "a volume must stay below 2^31 voxels";
    if (n_members != 1 && n_members != 2 && n_members != 4 && n_members != 8)
        return e + "n_members must be 1, 2, 4 or 8, got " + std::to_string(n_members);
    if (!masks) return e + "null masks";
    if (masks[0] != 0) return e + "masks must start at 0 (member 0 is the identity)";
    int bits = 0;
    for (int k = 0; k < n_members; ++k) {
        if (masks[k] < 0 || masks[k] > 7) return e + "a mask must be in [0, 7], got " + std::to_string(masks[k]);
        if (k && masks[k] <= masks[k - 1]) return e + "masks must strictly ascend";
        bits |= masks[k];
    }
    if (swap_axis < -1 || swap_axis > 2) return e + "swap_axis must be -1 (none), 0, 1 or 2, got " + std::to_string(swap_axis);
    if (n_pairs < 0 || n_pairs > UNET_MIRROR_MAX_PAIRS)
        return e + "n_pairs must be in [0, " + std::to_string(UNET_MIRROR_MAX_PAIRS) + "], got " + std::to_string(n_pairs);
    if (n_pairs && !pairs) return e + "null pairs";
    if (n_pairs && swap_axis < 0) return e + "pairs given without a swap_axis";
    if (swap_axis >= 0 && !((bits >> swap_axis) & 1)) return e + "swap_axis " + "xyz"[swap_axis] + " is not mirrored by any member";
    for (int i = 0; i < 2 * n_pairs; ++i) {
        if (pairs[i] < 0 || pairs[i] >= out_c) return e + "pairs: class " + std::to_string(pairs[i]) + " is not in [0, out_c)";
        for (int j = 0; j < i; ++j)
            if (pairs[j] == pairs[i]) return e + "pairs: class " + std::to_string(pairs[i]) + " appears twice (the pairs must be disjoint, a != b)";
    }
    return std::string();
}
int unet_mirror_combine(const float* stack, int out_c, int w, int h, int d, int n_members, const int* masks, int swap_axis,
                        const int* pairs, int n_pairs, float* mean, uint8_t* agreement, void* stream) {
    const std::string e = mirror_args_error("unet_mirror_combine", stack, out_c, w, h, d, n_members, masks, swap_axis, pairs, n_pairs);
    if (!e.empty()) return fail(e);
    if (!mean && !agreement) return fail("unet_mirror_combine: no output wanted");
    return run_on_device_of(stack, stream, [&](hipStream_t s) {
        launch_mirror_combine(stack, out_c, w, h, d, n_members, masks, swap_axis, pairs, n_pairs, mean, agreement, s);
    });
}
int unet_mirror_postproc(const float* stack, int out_c, int w, int h, int d, int n_members, const int* masks, int swap_axis,
                         const int* pairs, int n_pairs, float threshold, float* label_prob, float* fg_prob, uint16_t* label,
                         uint8_t* agreement, void* stream) {
    const std::string e = mirror_args_error("unet_mirror_postproc", stack, out_c, w, h, d, n_members, masks, swap_axis, pairs, n_pairs);
    if (!e.empty()) return fail(e);
    if (!label_prob && !fg_prob && !label && !agreement) return fail("unet_mirror_postproc: no output wanted");
    return run_on_device_of(stack, stream, [&](hipStream_t s) {
        launch_mirror_postproc(stack, out_c, w, h, d, n_members, masks, swap_axis, pairs, n_pairs, threshold, label_prob, fg_prob, label,
                               agreement, s);
    });
}

// ---- the model ensemble: members' probabilities folded into a running state, then read out (include/unet_ensemble.h) ----
static std::string ens_args_error(const char* who, int out_c, int64_t voxels) {
    const std::string e = std::string(who) + ": ";
    if (out_c < 2) return e + "out_c must be at least 2 (channel 0 is the background)";
    if (out_c > 65536) return e + "more than 65535 foreground classes do not fit a uint16 label";
    if (voxels <= 0) return e + "voxels must be positive";
    if (voxels >= ((int64_t)1 << 31)) return e + "a volume must stay below 2^31 voxels";
    return std::string();
}
int unet_ens_state_bytes(int out_c, int64_t voxels, size_t* bytes) {
    const std::string e = ens_args_error("unet_ens_state_bytes", out_c, voxels);
    if (!e.empty()) return fail(e);
    if (!bytes) return fail("unet_ens_state_bytes: null output");
    *bytes = ens_state_bytes(out_c, voxels);
    return 0;
}
int unet_ens_accumulate(const float* logits, int out_c, int64_t voxels, float weight, int first, void* state, size_t state_bytes,
                        void* stream) {
    const std::string e = ens_args_error("unet_ens_accumulate", out_c, voxels);
    if (!e.empty()) return fail(e);
    if (!logits) return fail("unet_ens_accumulate: null logits");
    if (!state) return fail("unet_ens_accumulate: null state");
    if (!(weight > 0.f && weight <= 1.f)) return fail("unet_ens_accumulate: weight must be finite and in (0, 1] (the weights are normalised)");
    if (state_bytes < ens_state_bytes(out_c, voxels)) return fail("unet_ens_accumulate: state too small (see unet_ens_state_bytes)");
    if ((uintptr_t)logits % 4 || (uintptr_t)state % 4) return fail("unet_ens_accumulate: logits and state must be 4-byte aligned");
    return run_on_device_of(logits, stream, [&](hipStream_t s) {
        launch_ens_accumulate(logits, out_c, voxels, weight, first != 0, (float*)state, s);
    });
}
int unet_ens_finalize(const void* state, size_t state_bytes, int out_c, int64_t voxels, float threshold, float* label_prob,
                      float* fg_prob, uint16_t* label, float* entropy, float* mutual_info, void* stream) {
    const std::string e = ens_args_error("unet_ens_finalize", out_c, voxels);
    if (!e.empty()) return fail(e);
    if (!state) return fail("unet_ens_finalize: null state");
    if (state_bytes < ens_state_bytes(out_c, voxels)) return fail("unet_ens_finalize: state too small (see unet_ens_state_bytes)");
    if ((uintptr_t)state % 4) return fail("unet_ens_finalize: state must be 4-byte aligned");
    if (!label_prob && !fg_prob && !label && !entropy && !mutual_info) return fail("unet_ens_finalize: no output wanted");
    return run_on_device_of(state, stream, [&](hipStream_t s) {
        launch_ens_finalize((const float*)state, out_c, voxels, threshold, label_prob, fg_prob, label, entropy, mutual_info, s);
    });
}

// ---- the pre-processing commands of a model (include/unet_preproc.h) ----
static const char* preproc_volume_error(const void* src, const void* dst, int w, int h, int d, int channels) {
    if (!src || !dst) return "unet_preproc: null device pointer";
    if (src == dst) return "unet_preproc: src and dst must differ (the commands run out of place)";
    if (w <= 0 || h <= 0 || d <= 0) return "unet_preproc: volume dimensions must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return "unet_preproc: a grid must stay below 2^31 voxels";
    if (channels <= 0 || channels > 65535) return "unet_preproc: channels must be in [1, 65535]";
    return nullptr;
}
int unet_preproc_filter(const float* src, float* dst, int w, int h, int d, int channels, int kind, int impl, void* stream) {
    if (const char* e = preproc_volume_error(src, dst, w, h, d, channels)) return fail(e);
    if (kind != UNET_PREPROC_GAUSSIAN && kind != UNET_PREPROC_MEAN) return fail("unet_preproc_filter: unknown kind " + std::to_string(kind));
    if (impl < UNET_PREPROC_IMPL_DEFAULT || impl > UNET_PREPROC_IMPL_VOXEL) return fail("unet_preproc_filter: unknown impl " + std::to_string(impl));
    if (preproc_filter_blocks(w, h, d, channels) >= ((int64_t)1 << 31)) return fail("unet_preproc_filter: too many tiles for one launch");
    return run_on_device_of(dst, stream, [&](hipStream_t s) { launch_preproc_filter(src, dst, w, h, d, channels, kind, impl, s); });
}
int unet_preproc_downsample(const float* src, float* dst, int w, int h, int d, int channels, void* stream) {
    if (const char* e = preproc_volume_error(src, dst, w, h, d, channels)) return fail(e);
    return run_on_device_of(dst, stream, [&](hipStream_t s) { launch_preproc_downsample(src, dst, w, h, d, channels, s); });
}
int unet_preproc_upsample(const float* src, float* dst, int w, int h, int d, int channels, void* stream) {
    if (const char* e = preproc_volume_error(src, dst, w, h, d, channels)) return fail(e);
    if (8 * (int64_t)w * h * d >= ((int64_t)1 << 31)) return fail("unet_preproc_upsample: the result must stay below 2^31 voxels");
    return run_on_device_of(dst, stream, [&](hipStream_t s) { launch_preproc_upsample(src, dst, w, h, d, channels, s); });
}
int unet_preproc_permute(const float* src, float* dst, int w, int h, int d, int channels, int op, void* stream) {
    if (const char* e = preproc_volume_error(src, dst, w, h, d, channels)) return fail(e);
    if (op < UNET_PREPROC_FLIP_X || op > UNET_PREPROC_SWAP_XZ) return fail("unet_preproc_permute: unknown op " + std::to_string(op));
    return run_on_device_of(dst, stream, [&](hipStream_t s) { launch_preproc_permute(src, dst, w, h, d, channels, op, s); });
}
int unet_preproc_scratch_bytes(int64_t values, size_t* bytes) {
    if (values <= 0) return fail("unet_preproc: values must be positive");
    if (!bytes) return fail("unet_preproc_scratch_bytes: null output");
    *bytes = preproc_scratch_bytes(values);
    return 0;
}
int unet_preproc_normalize(float* buf, int64_t values, void* scratch, size_t scratch_bytes, void* stream) {
    if (!buf) return fail("unet_preproc_normalize: null device pointer");
    if (values <= 0) return fail("unet_preproc: values must be positive");
    if (!scratch) return fail("unet_preproc_normalize: null scratch");
    if (scratch_bytes < preproc_scratch_bytes(values)) return fail("unet_preproc_normalize: scratch too small (see unet_preproc_scratch_bytes)");
    return run_on_device_of(buf, stream, [&](hipStream_t s) { launch_preproc_normalize(buf, values, scratch, s); });
}

// ---- checks the headers below word alike (w: the message prefix, "unet_xxx: ") ----
static std::string ptr_error(const std::string& w, const void* p, const char* name, int align) {
    if (!p) return w + "null " + name;
    if ((uintptr_t)p & (uintptr_t)(align - 1)) return w + name + " must be " + std::to_string(align) + "-byte aligned";
    return std::string();
}
static std::string labelling_size_error(const std::string& w, int64_t voxels, int n_classes) {
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return w + "voxels must be in [1, 2^31), got " + std::to_string(voxels);
    if (n_classes < 1 || n_classes > 65536) return w + "n_classes must be in [1, 65536], got " + std::to_string(n_classes);
    return std::string();
}
// the labelling's connectivity and impl.  UNET_CONN_IMPL_*, UNET_INST_LABEL_* and UNET_MORPH_IMPL_* are the same three values, so the
// one range serves the calls of all three headers; a caller whose header has no connectivity passes 6
static_assert(UNET_INST_LABEL_DEFAULT == UNET_CONN_IMPL_DEFAULT && UNET_INST_LABEL_GLOBAL == UNET_CONN_IMPL_GLOBAL &&
              UNET_MORPH_IMPL_DEFAULT == UNET_CONN_IMPL_DEFAULT && UNET_MORPH_IMPL_GLOBAL == UNET_CONN_IMPL_GLOBAL, "one impl range");
static std::string conn_error(const std::string& w, int connectivity, int impl) {
    if (connectivity != UNET_CONN_6 && connectivity != UNET_CONN_18 && connectivity != UNET_CONN_26)
        return w + "connectivity must be 6, 18 or 26, got " + std::to_string(connectivity);
    if (impl < UNET_CONN_IMPL_DEFAULT || impl > UNET_CONN_IMPL_GLOBAL) return w + "unknown impl " + std::to_string(impl);
    return std::string();
}
static std::string listed_range_error(const std::string& w, const uint32_t* listed, int n_listed, int n_classes) {
    for (int i = 0; i < n_listed; ++i)
        if (listed[i] == 0 || listed[i] >= (uint32_t)n_classes)
            return w + "listed class " + std::to_string(listed[i]) + " is not in [1, " + std::to_string(n_classes - 1) + "]";
    return std::string();
}
// the caller's list as the labelling takes it: a copy (the caller's is consumed here), ascending, each class once
static std::vector<uint32_t> listed_classes(const uint32_t* listed, int n_listed) {
    std::vector<uint32_t> classes(listed, listed + n_listed);
    std::sort(classes.begin(), classes.end());
    classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
    return classes;
}

// ---- a model's single_component_label (include/unet_components.h) ----
static const char* components_size_error(int64_t voxels, int n_classes) {
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return "unet_components: voxels must be in [1, 2^31)";
    if (n_classes < 1 || n_classes > 65536) return "unet_components: n_classes must be in [1, 65536]";
    return nullptr;
}
int unet_components_scratch_bytes(int64_t voxels, int n_classes, size_t* bytes) {
    if (const char* e = components_size_error(voxels, n_classes)) return fail(e);
    if (!bytes) return fail("unet_components_scratch_bytes: null output");
    *bytes = components_scratch_bytes(voxels, n_classes);
    return 0;
}
// what follows the argument checks of unet_components_keep_largest and unet_conn_keep_largest, which word theirs differently
static int keep_largest_call(const std::string& who, int w, int h, int d, uint16_t* label, int n_classes, const uint32_t* listed, int n_listed,
                             uint32_t* removed, int connectivity, int impl, void* scratch, void* stream) {
    const std::string e = listed_range_error(who, listed, n_listed, n_classes);
    if (!e.empty()) return fail(e);
    const std::vector<uint32_t> classes = listed_classes(listed, n_listed);
    return run_on_device_of(label, stream, [&](hipStream_t s) {
        launch_components_keep_largest(w, h, d, label, n_classes, classes.data(), (int)classes.size(), removed, impl, connectivity, scratch, s);
    });
}
int unet_components_keep_largest(int w, int h, int d, uint16_t* label, int n_classes, const uint32_t* listed, int n_listed,
                                 uint32_t* removed, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    if (w <= 0 || h <= 0 || d <= 0) return fail("unet_components: volume dimensions must be positive");
    if (const char* e = components_size_error((int64_t)w * h * d, n_classes)) return fail(e);
    if (!label) return fail("unet_components_keep_largest: null label");
    if (n_listed < 0) return fail("unet_components_keep_largest: n_listed must not be negative");
    if (n_listed > 0 && !listed) return fail("unet_components_keep_largest: null list");
    if (impl < UNET_COMPONENTS_IMPL_DEFAULT || impl > UNET_COMPONENTS_IMPL_GLOBAL)
        return fail("unet_components_keep_largest: unknown impl " + std::to_string(impl));
    if (!scratch) return fail("unet_components_keep_largest: null scratch");
    if (scratch_bytes < components_scratch_bytes((int64_t)w * h * d, n_classes))
        return fail("unet_components_keep_largest: scratch too small (see unet_components_scratch_bytes)");
    return keep_largest_call("unet_components_keep_largest: ", w, h, d, label, n_classes, listed, n_listed, removed, 6, impl, scratch, stream);
}

// ---- the atlas preparation of load_atlas (include/unet_atlas.h) ----
static const char* atlas_size_error(int64_t voxels, int n_regions, int n_tissues, int max_rounds) {
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return "unet_atlas: voxels must be in [1, 2^31)";
    if (n_regions < 0 || n_regions > 65535) return "unet_atlas: n_regions must be in [0, 65535]";
    if (n_tissues < 1 || n_tissues > 256) return "unet_atlas: n_tissues must be in [1, 256]";
    if (max_rounds < 0 || max_rounds > 65534) return "unet_atlas: max_rounds must be in [0, 65534]";
    return nullptr;
}
int unet_atlas_scratch_bytes(int64_t voxels, int n_regions, int n_tissues, int max_rounds, size_t* bytes) {
    if (const char* e = atlas_size_error(voxels, n_regions, n_tissues, max_rounds)) return fail(e);
    if (!bytes) return fail("unet_atlas_scratch_bytes: null output");
    *bytes = atlas_scratch_bytes(voxels, n_regions, n_tissues, max_rounds);
    return 0;
}
int unet_atlas_reclassify(int64_t voxels, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_regions, int n_tissues, int flags,
                          uint32_t* votes, uint32_t* tissue_total, uint32_t* covered, uint8_t* majority, uint32_t* erased, int impl,
                          void* scratch, size_t scratch_bytes, void* stream) {
    if (const char* e = atlas_size_error(voxels, n_regions, n_tissues, 0)) return fail(e);
    if (!tissue) return fail("unet_atlas_reclassify: null tissue");
    if (tissue_bytes != 1 && tissue_bytes != 2) return fail("unet_atlas_reclassify: tissue_bytes must be 1 or 2, got " + std::to_string(tissue_bytes));
    if (!atlas) return fail("unet_atlas_reclassify: null atlas");
    if ((uintptr_t)atlas & 1) return fail("unet_atlas_reclassify: atlas must be 2-byte aligned");
    if (flags & ~(UNET_ATLAS_CLAMP | UNET_ATLAS_PRESERVE | UNET_ATLAS_COUNT_ONLY))
        return fail("unet_atlas_reclassify: unknown flags " + std::to_string(flags));
    if (impl < UNET_ATLAS_IMPL_DEFAULT || impl > UNET_ATLAS_IMPL_GLOBAL) return fail("unet_atlas_reclassify: unknown impl " + std::to_string(impl));
    if (!scratch) return fail("unet_atlas_reclassify: null scratch");
    if (scratch_bytes < atlas_scratch_bytes(1, n_regions, n_tissues, 0))   // the tables only: no per-voxel scratch
        return fail("unet_atlas_reclassify: scratch too small (see unet_atlas_scratch_bytes)");
    return run_on_device_of(atlas, stream, [&](hipStream_t s) {
        launch_atlas_reclassify(voxels, tissue, tissue_bytes, atlas, n_regions, n_tissues, flags, votes, tissue_total, covered, majority,
                                erased, impl, scratch, s);
    });
}
int unet_atlas_grow(int w, int h, int d, const void* tissue, int tissue_bytes, uint16_t* atlas, int n_tissues, int flags,
                    const uint8_t* grow, int max_rounds, int smooth_rounds, uint32_t* filled, uint32_t* relabelled, uint32_t* info,
                    void* scratch, size_t scratch_bytes, void* stream) {
    if (w <= 0 || h <= 0 || d <= 0) return fail("unet_atlas_grow: volume dimensions must be positive");
    if (const char* e = atlas_size_error((int64_t)w * h * d, 0, n_tissues, max_rounds)) return fail(e);
    if (smooth_rounds < 0 || smooth_rounds > 16) return fail("unet_atlas_grow: smooth_rounds must be in [0, 16]");
    if (!tissue) return fail("unet_atlas_grow: null tissue");
    if (tissue_bytes != 1 && tissue_bytes != 2) return fail("unet_atlas_grow: tissue_bytes must be 1 or 2, got " + std::to_string(tissue_bytes));
    if (!atlas) return fail("unet_atlas_grow: null atlas");
    if ((uintptr_t)atlas & 1) return fail("unet_atlas_grow: atlas must be 2-byte aligned");
    if (flags & ~(UNET_ATLAS_CLAMP | UNET_ATLAS_PRESERVE)) return fail("unet_atlas_grow: unknown flags " + std::to_string(flags));
    if (!grow) return fail("unet_atlas_grow: null grow list");
    if (!scratch) return fail("unet_atlas_grow: null scratch");
    if (scratch_bytes < atlas_scratch_bytes((int64_t)w * h * d, 0, n_tissues, max_rounds))
        return fail("unet_atlas_grow: scratch too small (see unet_atlas_scratch_bytes)");
    return run_on_device_of(atlas, stream, [&](hipStream_t s) {   // grow is consumed inside the launcher, before this returns
        launch_atlas_grow(w, h, d, tissue, tissue_bytes, atlas, n_tissues, flags, grow, max_rounds, smooth_rounds, filled, relabelled,
                          info, scratch, s);
    });
}

// ---- the parcellation of a subject (include/unet_register.h) ----
static std::string reg_grids_error(const char* who, const void* subject, int sbytes, int sw, int sh, int sd, const void* tmpl, int tbytes,
                                   int tw, int th, int td, int n_tissues) {
    const std::string w = std::string(who) + ": ";
    if (!subject) return w + "null subject";
    if (!tmpl) return w + "null template";
    if (sbytes != 1 && sbytes != 2) return w + "sbytes must be 1 or 2, got " + std::to_string(sbytes);
    if (tbytes != 1 && tbytes != 2) return w + "tbytes must be 1 or 2, got " + std::to_string(tbytes);
    if (sw <= 0 || sh <= 0 || sd <= 0) return w + "subject dimensions must be positive";
    if (tw <= 0 || th <= 0 || td <= 0) return w + "template dimensions must be positive";
    if ((int64_t)sw * sh * sd >= ((int64_t)1 << 31)) return w + "the subject grid must stay below 2^31 voxels";
    if ((int64_t)tw * th * td >= ((int64_t)1 << 31)) return w + "the template grid must stay below 2^31 voxels";
    if (n_tissues < 2 || n_tissues > UNET_REG_MAX_TISSUES) return w + "n_tissues must be in [2, 16], got " + std::to_string(n_tissues);
    return std::string();
}
static bool reg_stride_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
int unet_reg_scratch_bytes(int64_t subject_voxels, int n_tissues, int max_iterations, size_t* bytes) {
    if (subject_voxels <= 0 || subject_voxels >= ((int64_t)1 << 31)) return fail("unet_reg: subject_voxels must be in [1, 2^31)");
    if (n_tissues < 2 || n_tissues > UNET_REG_MAX_TISSUES) return fail("unet_reg: n_tissues must be in [2, 16], got " + std::to_string(n_tissues));
    if (max_iterations < 1 || max_iterations > UNET_REG_MAX_ITERATIONS) return fail("unet_reg: max_iterations must be in [1, 1024]");
    if (!bytes) return fail("unet_reg_scratch_bytes: null output");
    *bytes = reg_scratch_bytes(n_tissues);   // the state and the counters: nothing per voxel, nothing per iteration
    return 0;
}
int unet_reg_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                  int n_tissues, const float* maps, int K, int stride, uint32_t* hist, int impl, void* scratch, size_t scratch_bytes,
                  void* stream) {
    (void)scratch; (void)scratch_bytes;   // reserved
    const std::string e = reg_grids_error("unet_reg_hist", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (!maps) return fail("unet_reg_hist: null maps");
    if (K < 1 || K > UNET_REG_MAX_MAPS) return fail("unet_reg_hist: K must be in [1, 25], got " + std::to_string(K));
    if (!reg_stride_ok(stride)) return fail("unet_reg_hist: stride must be 1, 2, 4 or 8, got " + std::to_string(stride));
    if (!hist) return fail("unet_reg_hist: null hist");
    if ((uintptr_t)hist & 3) return fail("unet_reg_hist: hist must be 4-byte aligned");
    if (impl < UNET_REG_IMPL_DEFAULT || impl > UNET_REG_IMPL_GLOBAL) return fail("unet_reg_hist: unknown impl " + std::to_string(impl));
    return run_on_device_of(hist, stream, [&](hipStream_t s) {   // maps is consumed inside the launcher, before this returns
        launch_reg_hist(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, maps, K, stride, hist, impl, s);
    });
}
int unet_reg_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    int n_tissues, const float* init, const float* step, const int* stages, int n_stages, int max_iterations,
                    float* map_out, int64_t* trace, int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string e = reg_grids_error("unet_reg_search", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (!init) return fail("unet_reg_search: null init");
    if (!step) return fail("unet_reg_search: null step");
    bool any = false;
    for (int i = 0; i < 12; ++i) {
        if (!std::isfinite(step[i]) || step[i] < 0.f) return fail("unet_reg_search: step[" + std::to_string(i) + "] must be finite and >= 0");
        any |= step[i] > 0.f;
    }
    if (!any) return fail("unet_reg_search: at least one step must be > 0");
    if (n_stages < 1 || n_stages > UNET_REG_MAX_STAGES) return fail("unet_reg_search: n_stages must be in [1, 4], got " + std::to_string(n_stages));
    if (!stages) return fail("unet_reg_search: null stages");
    for (int g = 0; g < n_stages; ++g) {
        const std::string st = "unet_reg_search: stage " + std::to_string(g) + ": ";
        if (!reg_stride_ok(stages[3 * g])) return fail(st + "stride must be 1, 2, 4 or 8, got " + std::to_string(stages[3 * g]));
        if (stages[3 * g + 1] < 0 || stages[3 * g + 1] > stages[3 * g + 2] || stages[3 * g + 2] > UNET_REG_MAX_LEVEL)
            return fail(st + "levels must satisfy 0 <= first_level <= last_level <= 20");
    }
    if (max_iterations < 1 || max_iterations > UNET_REG_MAX_ITERATIONS) return fail("unet_reg_search: max_iterations must be in [1, 1024]");
    if (!map_out) return fail("unet_reg_search: null map_out");
    if ((uintptr_t)map_out & 3) return fail("unet_reg_search: map_out must be 4-byte aligned");
    if ((uintptr_t)trace & 7) return fail("unet_reg_search: trace must be 8-byte aligned");
    if (!info) return fail("unet_reg_search: null info");
    if ((uintptr_t)info & 7) return fail("unet_reg_search: info must be 8-byte aligned");
    if (impl < UNET_REG_IMPL_DEFAULT || impl > UNET_REG_IMPL_GLOBAL) return fail("unet_reg_search: unknown impl " + std::to_string(impl));
    if (!scratch) return fail("unet_reg_search: null scratch");
    if (scratch_bytes < reg_scratch_bytes(n_tissues)) return fail("unet_reg_search: scratch too small (see unet_reg_scratch_bytes)");
    return run_on_device_of(map_out, stream, [&](hipStream_t s) {   // init, step and stages are consumed inside the launcher
        launch_reg_search(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, init, step, stages, n_stages, max_iterations,
                          map_out, trace, info, impl, scratch, s);
    });
}
int unet_reg_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                   const uint16_t* atlas, int n_tissues, const float* map, uint16_t* out, uint32_t* counts, void* stream) {
    const std::string e = reg_grids_error("unet_reg_carry", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (!atlas) return fail("unet_reg_carry: null atlas");
    if ((uintptr_t)atlas & 1) return fail("unet_reg_carry: atlas must be 2-byte aligned");
    if (!map) return fail("unet_reg_carry: null map");
    if (!out) return fail("unet_reg_carry: null out");
    if ((uintptr_t)out & 1) return fail("unet_reg_carry: out must be 2-byte aligned");
    if ((uintptr_t)counts & 3) return fail("unet_reg_carry: counts must be 4-byte aligned");
    return run_on_device_of(out, stream, [&](hipStream_t s) {   // map is consumed inside the launcher
        launch_reg_carry(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, atlas, n_tissues, map, out, counts, s);
    });
}

// ---- the co-registration of two intensity images (include/unet_coreg.h) ----
static bool coreg_bins_ok(int bins) { return bins == 8 || bins == 16 || bins == 32; }
static std::string coreg_grids_error(const std::string& w, const void* fixed, int fw, int fh, int fd, const void* moving, int mw, int mh,
                                     int md, int bins) {
    if (!fixed) return w + "null fixed";
    if (!moving) return w + "null moving";
    if (fw <= 0 || fh <= 0 || fd <= 0) return w + "fixed dimensions must be positive";
    if (mw <= 0 || mh <= 0 || md <= 0) return w + "moving dimensions must be positive";
    if ((int64_t)fw * fh * fd >= ((int64_t)1 << 31)) return w + "the fixed grid must stay below 2^31 voxels";
    if ((int64_t)mw * mh * md >= ((int64_t)1 << 31)) return w + "the moving grid must stay below 2^31 voxels";
    if (!coreg_bins_ok(bins)) return w + "bins must be 8, 16 or 32, got " + std::to_string(bins);
    return std::string();
}
int unet_coreg_scratch_bytes(int64_t fixed_voxels, int bins, int max_iterations, size_t* bytes) {
    if (fixed_voxels <= 0 || fixed_voxels >= ((int64_t)1 << 31)) return fail("unet_coreg: fixed_voxels must be in [1, 2^31)");
    if (!coreg_bins_ok(bins)) return fail("unet_coreg: bins must be 8, 16 or 32, got " + std::to_string(bins));
    if (max_iterations < 1 || max_iterations > UNET_COREG_MAX_ITERATIONS) return fail("unet_coreg: max_iterations must be in [1, 1024]");
    if (!bytes) return fail("unet_coreg_scratch_bytes: null output");
    *bytes = coreg_scratch_bytes(bins);   // the state and the counters: nothing per voxel, nothing per iteration
    return 0;
}
int unet_coreg_code(const float* image, int64_t voxels, float lo, float hi, int bins, uint8_t* codes, void* stream) {
    const std::string w = "unet_coreg_code: ";
    if (std::string e = ptr_error(w, image, "image", 4); !e.empty()) return fail(e);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail(w + "voxels must be in [1, 2^31)");
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(w + "lo and hi must be finite");
    if (!(lo < hi)) return fail(w + "lo must be below hi");
    if (!coreg_bins_ok(bins)) return fail(w + "bins must be 8, 16 or 32, got " + std::to_string(bins));
    const float diff = hi - lo, scale = (float)bins / diff;   // fp32: one subtraction, one division
    if (!std::isfinite(diff) || !std::isfinite(scale) || !(scale > 0.f)) return fail(w + "the scale bins / (hi - lo) must be finite");
    if (!codes) return fail(w + "null codes");
    return run_on_device_of(codes, stream, [&](hipStream_t s) { launch_coreg_code(image, voxels, lo, scale, bins, codes, s); });
}
int unet_coreg_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                    const float* maps, int K, int stride, uint32_t* hist, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    (void)scratch; (void)scratch_bytes;   // reserved
    const std::string w = "unet_coreg_hist: ";
    if (std::string e = coreg_grids_error(w, fixed, fw, fh, fd, moving, mw, mh, md, bins); !e.empty()) return fail(e);
    if (!maps) return fail(w + "null maps");
    if (K < 1 || K > UNET_COREG_MAX_MAPS) return fail(w + "K must be in [1, 25], got " + std::to_string(K));
    if (!reg_stride_ok(stride)) return fail(w + "stride must be 1, 2, 4 or 8, got " + std::to_string(stride));
    if (std::string e = ptr_error(w, hist, "hist", 4); !e.empty()) return fail(e);
    if (impl < UNET_COREG_IMPL_DEFAULT || impl > UNET_COREG_IMPL_GLOBAL) return fail(w + "unknown impl " + std::to_string(impl));
    return run_on_device_of(hist, stream, [&](hipStream_t s) {   // maps is consumed inside the launcher, before this returns
        launch_coreg_hist(fixed, fw, fh, fd, moving, mw, mh, md, bins, maps, K, stride, hist, impl, s);
    });
}
int unet_coreg_score(const uint32_t* hist, int K, int bins, int64_t* scores, void* stream) {
    const std::string w = "unet_coreg_score: ";
    if (std::string e = ptr_error(w, hist, "hist", 4); !e.empty()) return fail(e);
    if (K < 1 || K > UNET_COREG_MAX_MAPS) return fail(w + "K must be in [1, 25], got " + std::to_string(K));
    if (!coreg_bins_ok(bins)) return fail(w + "bins must be 8, 16 or 32, got " + std::to_string(bins));
    if (std::string e = ptr_error(w, scores, "scores", 8); !e.empty()) return fail(e);
    return run_on_device_of(scores, stream, [&](hipStream_t s) { launch_coreg_score(hist, K, bins, scores, s); });
}
int unet_coreg_search(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins,
                      const float* init, const float* step, const int* stages, int n_stages, int max_iterations, float* map_out,
                      int64_t* trace, int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string w = "unet_coreg_search: ";
    if (std::string e = coreg_grids_error(w, fixed, fw, fh, fd, moving, mw, mh, md, bins); !e.empty()) return fail(e);
    if (!init) return fail(w + "null init");
    if (!step) return fail(w + "null step");
    bool any = false;
    for (int i = 0; i < 12; ++i) {
        if (!std::isfinite(step[i]) || step[i] < 0.f) return fail(w + "step[" + std::to_string(i) + "] must be finite and >= 0");
        any |= step[i] > 0.f;
    }
    if (!any) return fail(w + "at least one step must be > 0");
    if (n_stages < 1 || n_stages > UNET_COREG_MAX_STAGES) return fail(w + "n_stages must be in [1, 4], got " + std::to_string(n_stages));
    if (!stages) return fail(w + "null stages");
    for (int g = 0; g < n_stages; ++g) {
        const std::string st = w + "stage " + std::to_string(g) + ": ";
        if (!reg_stride_ok(stages[3 * g])) return fail(st + "stride must be 1, 2, 4 or 8, got " + std::to_string(stages[3 * g]));
        if (stages[3 * g + 1] < 0 || stages[3 * g + 1] > stages[3 * g + 2] || stages[3 * g + 2] > UNET_COREG_MAX_LEVEL)
            return fail(st + "levels must satisfy 0 <= first_level <= last_level <= 20");
    }
    if (max_iterations < 1 || max_iterations > UNET_COREG_MAX_ITERATIONS) return fail(w + "max_iterations must be in [1, 1024]");
    if (std::string e = ptr_error(w, map_out, "map_out", 4); !e.empty()) return fail(e);
    if ((uintptr_t)trace & 7) return fail(w + "trace must be 8-byte aligned");
    if (std::string e = ptr_error(w, info, "info", 8); !e.empty()) return fail(e);
    if (impl < UNET_COREG_IMPL_DEFAULT || impl > UNET_COREG_IMPL_GLOBAL) return fail(w + "unknown impl " + std::to_string(impl));
    if (!scratch) return fail(w + "null scratch");
    if (scratch_bytes < coreg_scratch_bytes(bins)) return fail(w + "scratch too small (see unet_coreg_scratch_bytes)");
    return run_on_device_of(map_out, stream, [&](hipStream_t s) {   // init, step and stages are consumed inside the launcher
        launch_coreg_search(fixed, fw, fh, fd, moving, mw, mh, md, bins, init, step, stages, n_stages, max_iterations, map_out, trace, info,
                            impl, scratch, s);
    });
}

// ---- the starts of a registration (include/unet_start.h) ----
int unet_start_scratch_bytes(int n_tissues, int n, size_t* bytes) {
    if (n_tissues < 2 || n_tissues > UNET_REG_MAX_TISSUES) return fail("unet_start: n_tissues must be in [2, 16], got " + std::to_string(n_tissues));
    if (n < 1 || n > UNET_START_MAX_STATES) return fail("unet_start: n must be in [1, 4], got " + std::to_string(n));
    if (!bytes) return fail("unet_start_scratch_bytes: null output");
    *bytes = start_scratch_bytes(n_tissues, n);   // the states, their counters and the sequential searches' scratch: nothing per voxel
    return 0;
}
int unet_start_moments(const void* volume, int vbytes, int w, int h, int d, int lo, int hi, uint64_t* sums, void* stream) {
    const std::string wh = "unet_start_moments: ";
    if (!volume) return fail(wh + "null volume");
    if (vbytes != 1 && vbytes != 2) return fail(wh + "vbytes must be 1 or 2, got " + std::to_string(vbytes));
    if (w <= 0 || h <= 0 || d <= 0) return fail(wh + "volume dimensions must be positive");
    if (w > UNET_START_MAX_DIM || h > UNET_START_MAX_DIM || d > UNET_START_MAX_DIM) return fail(wh + "volume dimensions must stay below 65536");
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return fail(wh + "the volume must stay below 2^31 voxels");
    if (lo < 0 || lo > 65535) return fail(wh + "lo must be in [0, 65535], got " + std::to_string(lo));
    if (hi < 0 || hi > 65535) return fail(wh + "hi must be in [0, 65535], got " + std::to_string(hi));
    if (std::string e = ptr_error(wh, sums, "sums", 8); !e.empty()) return fail(e);
    return run_on_device_of(sums, stream, [&](hipStream_t s) { launch_start_moments(volume, vbytes, w, h, d, lo, hi, sums, s); });
}
int unet_start_pick(const uint32_t* hist, int S, int n_tissues, const float* maps, int n, int always, int64_t* scores, float* inits,
                    int32_t* picked, void* stream) {
    const std::string w = "unet_start_pick: ";
    if (std::string e = ptr_error(w, hist, "hist", 4); !e.empty()) return fail(e);
    if (S < 1 || S > UNET_START_MAX_STARTS) return fail(w + "S must be in [1, 125], got " + std::to_string(S));
    if (n_tissues < 2 || n_tissues > UNET_REG_MAX_TISSUES) return fail(w + "n_tissues must be in [2, 16], got " + std::to_string(n_tissues));
    if (std::string e = ptr_error(w, maps, "maps", 4); !e.empty()) return fail(e);
    if (n < 1 || n > UNET_START_MAX_STATES || n > S) return fail(w + "n must be in [1, min(S, 4)], got " + std::to_string(n));
    if (always < -1 || always >= S) return fail(w + "always must be -1 or in [0, S), got " + std::to_string(always));
    if (std::string e = ptr_error(w, scores, "scores", 8); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, inits, "inits", 4); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, picked, "picked", 4); !e.empty()) return fail(e);
    return run_on_device_of(picked, stream, [&](hipStream_t s) { launch_start_pick(hist, S, n_tissues, maps, n, always, scores, inits, picked, s); });
}
int unet_start_search(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                      int n_tissues, const float* inits, int n, const float* step, const int* stages, int n_stages, int max_iterations,
                      float* maps_out, int64_t* trace, int64_t* info, int32_t* best, float* best_map, int impl, void* scratch,
                      size_t scratch_bytes, void* stream) {
    const std::string w = "unet_start_search: ";
    const std::string e = reg_grids_error("unet_start_search", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (std::string pe = ptr_error(w, inits, "inits", 4); !pe.empty()) return fail(pe);
    if (n < 1 || n > UNET_START_MAX_STATES) return fail(w + "n must be in [1, 4], got " + std::to_string(n));
    if (!step) return fail(w + "null step");
    bool any = false;
    for (int i = 0; i < 12; ++i) {
        if (!std::isfinite(step[i]) || step[i] < 0.f) return fail(w + "step[" + std::to_string(i) + "] must be finite and >= 0");
        any |= step[i] > 0.f;
    }
    if (!any) return fail(w + "at least one step must be > 0");
    if (n_stages < 1 || n_stages > UNET_REG_MAX_STAGES) return fail(w + "n_stages must be in [1, 4], got " + std::to_string(n_stages));
    if (!stages) return fail(w + "null stages");
    for (int g = 0; g < n_stages; ++g) {
        const std::string st = w + "stage " + std::to_string(g) + ": ";
        if (!reg_stride_ok(stages[3 * g])) return fail(st + "stride must be 1, 2, 4 or 8, got " + std::to_string(stages[3 * g]));
        if (stages[3 * g + 1] < 0 || stages[3 * g + 1] > stages[3 * g + 2] || stages[3 * g + 2] > UNET_REG_MAX_LEVEL)
            return fail(st + "levels must satisfy 0 <= first_level <= last_level <= 20");
    }
    if (max_iterations < 1 || max_iterations > UNET_REG_MAX_ITERATIONS) return fail(w + "max_iterations must be in [1, 1024]");
    if (std::string pe = ptr_error(w, maps_out, "maps_out", 4); !pe.empty()) return fail(pe);
    if ((uintptr_t)trace & 7) return fail(w + "trace must be 8-byte aligned");
    if (std::string pe = ptr_error(w, info, "info", 8); !pe.empty()) return fail(pe);
    if (std::string pe = ptr_error(w, best, "best", 4); !pe.empty()) return fail(pe);
    if (std::string pe = ptr_error(w, best_map, "best_map", 4); !pe.empty()) return fail(pe);
    if (impl < UNET_START_IMPL_DEFAULT || impl > UNET_START_IMPL_SEQUENTIAL) return fail(w + "unknown impl " + std::to_string(impl));
    if (!scratch) return fail(w + "null scratch");
    if (scratch_bytes < start_scratch_bytes(n_tissues, n)) return fail(w + "scratch too small (see unet_start_scratch_bytes)");
    if (impl != UNET_START_IMPL_SEQUENTIAL)   // DEFAULT: BATCHED
        return run_on_device_of(maps_out, stream, [&](hipStream_t s) {   // step and stages are consumed inside the launcher
            launch_start_search(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, inits, n, step, stages, n_stages,
                                max_iterations, maps_out, trace, info, best, best_map, scratch, s);
        });
    // SEQUENTIAL: the register module's entry point takes its start from the host: one copy and one wait, then n searches in a row
    float host_inits[UNET_START_MAX_STATES * 12];
    if (int rc = run_on_device_of(maps_out, stream, [&](hipStream_t s) {
            HIP_OK(hipMemcpyAsync(host_inits, inits, (size_t)n * 12 * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
        }))
        return rc;
    for (int s = 0; s < n; ++s)
        if (int rc = unet_reg_search(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, host_inits + 12 * s, step, stages,
                                     n_stages, max_iterations, maps_out + 12 * s, trace ? trace + (size_t)s * 4 * max_iterations : nullptr,
                                     info + 4 * s, UNET_REG_IMPL_DEFAULT, start_seq_scratch(scratch, n_tissues, n, s),
                                     start_seq_scratch_bytes(n_tissues), stream))
            return rc;
    return run_on_device_of(maps_out, stream, [&](hipStream_t s) { launch_start_close(info, maps_out, n, best, best_map, s); });
}

// ---- the non-linear refinement of a parcellation (include/unet_warp.h) ----
static bool warp_g_ok(int g) { return g == 4 || g == 8 || g == 16 || g == 32; }
static std::string warp_g_error(const std::string& w, int g) {
    return warp_g_ok(g) ? std::string() : w + "g must be 4, 8, 16 or 32, got " + std::to_string(g);
}
// the levels of a fit: n_levels x {g, first_step, last_step, max_sweeps, limit}
static std::string warp_levels_error(const std::string& w, const int* levels, int n_levels) {
    if (n_levels < 1 || n_levels > UNET_WARP_MAX_LEVELS) return w + "n_levels must be in [1, 4], got " + std::to_string(n_levels);
    if (!levels) return w + "null levels";
    int rows = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* v = levels + 5 * l;
        const std::string lv = w + "level " + std::to_string(l) + ": ";
        if (!warp_g_ok(v[0])) return lv + "g must be 4, 8, 16 or 32, got " + std::to_string(v[0]);
        if (l && 2 * v[0] != levels[5 * (l - 1)]) return lv + "g must be half the level before's, got " + std::to_string(v[0]);
        for (int e = 1; e <= 2; ++e)
            if (v[e] < 1 || v[e] > UNET_WARP_MAX_STEP || (v[e] & (v[e] - 1)))
                return lv + (e == 1 ? "first_step" : "last_step") + " must be a power of two in [1, 16384], got " + std::to_string(v[e]);
        if (v[1] < v[2]) return lv + "first_step must not be below last_step";
        if (v[3] < 1 || v[3] > UNET_WARP_MAX_SWEEPS) return lv + "max_sweeps must be in [1, 16], got " + std::to_string(v[3]);
        if (v[4] < 0) return lv + "limit must not be negative, got " + std::to_string(v[4]);
        for (int s = v[1]; s >= v[2]; s >>= 1) ++rows;
    }
    if (rows > UNET_WARP_MAX_ROWS) return w + "levels hold " + std::to_string(rows) + " (level, step) pairs, more than 32";
    return std::string();
}
// a grid of the warps, the co-registration's warps and their geometry: positive dimensions, below 2^31 voxels
static std::string grid_dims_error(const std::string& w, const char* name, int a, int b, int c) {
    if (a <= 0 || b <= 0 || c <= 0) return w + name + " dimensions must be positive";
    if ((int64_t)a * b * c >= ((int64_t)1 << 31)) return w + "the " + name + " grid must stay below 2^31 voxels";
    return std::string();
}
// What a sweep and a fit of unet_warp.h and of unet_cowarp.h take behind their grids, checked once: the ranges are the same (the
// static_assert of the section below); a header's own are its g and levels rules and the call that sizes its scratch, with its name
struct LatticeRules {
    std::string (*g_error)(const std::string&, int);
    std::string (*levels_error)(const std::string&, const int*, int);
    size_t (*scratch_bytes)(int, int, int, const int*, int);
    const char* see;
};
static const LatticeRules warp_rules = {warp_g_error, warp_levels_error, warp_scratch_bytes, "unet_warp_scratch_bytes"};
static std::string lattice_scratch_error(const std::string& w, const LatticeRules& r, int sw, int sh, int sd, const int* levels, int n_levels,
                                         int impl, const void* scratch, size_t scratch_bytes) {
    if (impl < UNET_WARP_IMPL_DEFAULT || impl > UNET_WARP_IMPL_VOXEL) return w + "unknown impl " + std::to_string(impl);
    if (!scratch) return w + "null scratch";
    if (scratch_bytes < r.scratch_bytes(sw, sh, sd, levels, n_levels)) return w + "scratch too small (see " + r.see + ")";
    return std::string();
}
static std::string lattice_sweep_error(const std::string& w, const LatticeRules& r, int sw, int sh, int sd, const float* map, const int32_t* D,
                                       int g, int step, int limit, const int64_t* info, int impl, const void* scratch, size_t scratch_bytes) {
    if (!map) return w + "null map";
    if (std::string e = ptr_error(w, D, "D", 4); !e.empty()) return e;
    if (std::string e = r.g_error(w, g); !e.empty()) return e;
    if (step < 1 || step > UNET_WARP_MAX_DISP) return w + "step must be in [1, 32767], got " + std::to_string(step);
    if (limit < 0) return w + "limit must not be negative, got " + std::to_string(limit);
    if (std::string e = ptr_error(w, info, "info", 8); !e.empty()) return e;
    const int level[5] = {g, 1, 1, 1, 0};
    return lattice_scratch_error(w, r, sw, sh, sd, level, 1, impl, scratch, scratch_bytes);
}
static std::string lattice_fit_error(const std::string& w, const LatticeRules& r, int sw, int sh, int sd, const float* map, const int* levels,
                                     int n_levels, const int32_t* D_out, const int64_t* report, int impl, const void* scratch,
                                     size_t scratch_bytes) {
    if (!map) return w + "null map";
    if (std::string e = r.levels_error(w, levels, n_levels); !e.empty()) return e;
    if (std::string e = ptr_error(w, D_out, "D_out", 4); !e.empty()) return e;
    if (std::string e = ptr_error(w, report, "report", 8); !e.empty()) return e;
    return lattice_scratch_error(w, r, sw, sh, sd, levels, n_levels, impl, scratch, scratch_bytes);
}
int unet_warp_lattice(int sw, int sh, int sd, int g, int* nx, int* ny, int* nz) {
    const std::string w = "unet_warp_lattice: ";
    if (std::string e = grid_dims_error(w, "subject", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (!nx || !ny || !nz) return fail(w + "null output");
    *nx = (sw + g - 1) / g + 1;
    *ny = (sh + g - 1) / g + 1;
    *nz = (sd + g - 1) / g + 1;
    return 0;
}
int unet_warp_scratch_bytes(int sw, int sh, int sd, int n_tissues, const int* levels, int n_levels, size_t* bytes) {
    const std::string w = "unet_warp_scratch_bytes: ";
    if (std::string e = grid_dims_error(w, "subject", sw, sh, sd); !e.empty()) return fail(e);
    if (n_tissues < 2 || n_tissues > UNET_WARP_MAX_TISSUES) return fail(w + "n_tissues must be in [2, 16], got " + std::to_string(n_tissues));
    if (std::string e = warp_levels_error(w, levels, n_levels); !e.empty()) return fail(e);
    if (!bytes) return fail(w + "null output");
    *bytes = warp_scratch_bytes(sw, sh, sd, levels, n_levels);
    return 0;
}
int unet_warp_hist(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                   int n_tissues, const float* map, const int32_t* D, int g, uint32_t* hist, void* stream) {
    const std::string w = "unet_warp_hist: ";
    const std::string e = reg_grids_error("unet_warp_hist", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (!map) return fail(w + "null map");
    if (std::string pe = ptr_error(w, D, "D", 4); !pe.empty()) return fail(pe);
    if (std::string ge = warp_g_error(w, g); !ge.empty()) return fail(ge);
    if (std::string pe = ptr_error(w, hist, "hist", 4); !pe.empty()) return fail(pe);
    return run_on_device_of(hist, stream, [&](hipStream_t s) {   // map is consumed inside the launcher, before this returns
        launch_warp_hist(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, map, D, g, hist, s);
    });
}
int unet_warp_sweep(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    int n_tissues, const float* map, int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch,
                    size_t scratch_bytes, void* stream) {
    const std::string w = "unet_warp_sweep: ";
    const std::string e = reg_grids_error("unet_warp_sweep", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    const std::string se = lattice_sweep_error(w, warp_rules, sw, sh, sd, map, D, g, step, limit, info, impl, scratch, scratch_bytes);
    if (!se.empty()) return fail(se);
    return run_on_device_of(D, stream, [&](hipStream_t s) {
        launch_warp_sweep(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, map, D, g, step, limit, info, impl, scratch, s);
    });
}
int unet_warp_refine(const int32_t* D_coarse, int sw, int sh, int sd, int g, int32_t* D_fine, void* stream) {
    const std::string w = "unet_warp_refine: ";
    if (std::string pe = ptr_error(w, D_coarse, "D_coarse", 4); !pe.empty()) return fail(pe);
    if (std::string e = grid_dims_error(w, "subject", sw, sh, sd); !e.empty()) return fail(e);
    if (g != 8 && g != 16 && g != 32) return fail(w + "g must be 8, 16 or 32, got " + std::to_string(g));
    if (std::string pe = ptr_error(w, D_fine, "D_fine", 4); !pe.empty()) return fail(pe);
    return run_on_device_of(D_fine, stream, [&](hipStream_t s) { launch_warp_refine(D_coarse, sw, sh, sd, g, D_fine, s); });
}
int unet_warp_fit(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                  int n_tissues, const float* map, const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch,
                  size_t scratch_bytes, void* stream) {
    const std::string w = "unet_warp_fit: ";
    const std::string e = reg_grids_error("unet_warp_fit", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    const std::string fe = lattice_fit_error(w, warp_rules, sw, sh, sd, map, levels, n_levels, D_out, report, impl, scratch, scratch_bytes);
    if (!fe.empty()) return fail(fe);
    return run_on_device_of(D_out, stream, [&](hipStream_t s) {   // map and levels are consumed inside the launcher
        launch_warp_fit(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues, map, levels, n_levels, D_out, report, impl,
                        scratch, s);
    });
}
int unet_warp_carry(const void* subject, int sbytes, int sw, int sh, int sd, const void* template_, int tbytes, int tw, int th, int td,
                    const uint16_t* atlas, int n_tissues, const float* map, const int32_t* D, int g, uint16_t* out, uint32_t* counts,
                    void* stream) {
    const std::string w = "unet_warp_carry: ";
    const std::string e = reg_grids_error("unet_warp_carry", subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, n_tissues);
    if (!e.empty()) return fail(e);
    if (std::string pe = ptr_error(w, atlas, "atlas", 2); !pe.empty()) return fail(pe);
    if (!map) return fail(w + "null map");
    if (std::string pe = ptr_error(w, D, "D", 4); !pe.empty()) return fail(pe);
    if (std::string ge = warp_g_error(w, g); !ge.empty()) return fail(ge);
    if (std::string pe = ptr_error(w, out, "out", 2); !pe.empty()) return fail(pe);
    if ((uintptr_t)counts & 3) return fail(w + "counts must be 4-byte aligned");
    return run_on_device_of(out, stream, [&](hipStream_t s) {   // map is consumed inside the launcher
        launch_warp_carry(subject, sbytes, sw, sh, sd, template_, tbytes, tw, th, td, atlas, n_tissues, map, D, g, out, counts, s);
    });
}

// ---- the non-linear refinement of a co-registration (include/unet_cowarp.h) ----
static std::string cowarp_g_error(const std::string& w, int g) {
    return g == 4 || g == 8 || g == 16 ? std::string() : w + "g must be 4, 8 or 16, got " + std::to_string(g);
}
// the levels of a fit: unet_warp.h's rows, without g = 32
static std::string cowarp_levels_error(const std::string& w, const int* levels, int n_levels) {
    if (n_levels < 1 || n_levels > UNET_COWARP_MAX_LEVELS) return w + "n_levels must be in [1, 3], got " + std::to_string(n_levels);
    if (!levels) return w + "null levels";
    for (int l = 0; l < n_levels; ++l)
        if (std::string e = cowarp_g_error(w + "level " + std::to_string(l) + ": ", levels[5 * l]); !e.empty()) return e;
    return warp_levels_error(w, levels, n_levels);
}
static_assert(UNET_COWARP_MAX_STEP == UNET_WARP_MAX_STEP && UNET_COWARP_MAX_SWEEPS == UNET_WARP_MAX_SWEEPS &&
              UNET_COWARP_MAX_ROWS == UNET_WARP_MAX_ROWS && UNET_COWARP_MAX_DISP == UNET_WARP_MAX_DISP &&
              UNET_COWARP_IMPL_DEFAULT == UNET_WARP_IMPL_DEFAULT && UNET_COWARP_IMPL_VOXEL == UNET_WARP_IMPL_VOXEL, "one schedule for both warps");
static const LatticeRules cowarp_rules = {cowarp_g_error, cowarp_levels_error, cowarp_scratch_bytes, "unet_cowarp_scratch_bytes"};
int unet_cowarp_scratch_bytes(int fw, int fh, int fd, int bins, const int* levels, int n_levels, size_t* bytes) {
    const std::string w = "unet_cowarp_scratch_bytes: ";
    if (std::string e = grid_dims_error(w, "fixed", fw, fh, fd); !e.empty()) return fail(e);
    if (!coreg_bins_ok(bins)) return fail(w + "bins must be 8, 16 or 32, got " + std::to_string(bins));
    if (std::string e = cowarp_levels_error(w, levels, n_levels); !e.empty()) return fail(e);
    if (!bytes) return fail(w + "null output");
    *bytes = cowarp_scratch_bytes(fw, fh, fd, levels, n_levels);
    return 0;
}
int unet_cowarp_hist(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins, const float* map,
                     const int32_t* D, int g, uint32_t* hist, void* stream) {
    const std::string w = "unet_cowarp_hist: ";
    if (std::string e = coreg_grids_error(w, fixed, fw, fh, fd, moving, mw, mh, md, bins); !e.empty()) return fail(e);
    if (!map) return fail(w + "null map");
    if (std::string e = ptr_error(w, D, "D", 4); !e.empty()) return fail(e);
    if (std::string e = cowarp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, hist, "hist", 4); !e.empty()) return fail(e);
    return run_on_device_of(hist, stream, [&](hipStream_t s) {   // map is consumed inside the launcher, before this returns
        launch_cowarp_hist(fixed, fw, fh, fd, moving, mw, mh, md, bins, map, D, g, hist, s);
    });
}
int unet_cowarp_weights(const uint32_t* hist, int bins, int16_t* weights, void* stream) {
    const std::string w = "unet_cowarp_weights: ";
    if (std::string e = ptr_error(w, hist, "hist", 4); !e.empty()) return fail(e);
    if (!coreg_bins_ok(bins)) return fail(w + "bins must be 8, 16 or 32, got " + std::to_string(bins));
    if (std::string e = ptr_error(w, weights, "weights", 2); !e.empty()) return fail(e);
    return run_on_device_of(weights, stream, [&](hipStream_t s) { launch_cowarp_weights(hist, bins, weights, s); });
}
int unet_cowarp_sweep(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins, const float* map,
                      int32_t* D, int g, int step, int limit, int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string w = "unet_cowarp_sweep: ";
    if (std::string e = coreg_grids_error(w, fixed, fw, fh, fd, moving, mw, mh, md, bins); !e.empty()) return fail(e);
    const std::string se = lattice_sweep_error(w, cowarp_rules, fw, fh, fd, map, D, g, step, limit, info, impl, scratch, scratch_bytes);
    if (!se.empty()) return fail(se);
    return run_on_device_of(D, stream, [&](hipStream_t s) {
        launch_cowarp_sweep(fixed, fw, fh, fd, moving, mw, mh, md, bins, map, D, g, step, limit, info, impl, scratch, s);
    });
}
int unet_cowarp_fit(const uint8_t* fixed, int fw, int fh, int fd, const uint8_t* moving, int mw, int mh, int md, int bins, const float* map,
                    const int* levels, int n_levels, int32_t* D_out, int64_t* report, int impl, void* scratch, size_t scratch_bytes,
                    void* stream) {
    const std::string w = "unet_cowarp_fit: ";
    if (std::string e = coreg_grids_error(w, fixed, fw, fh, fd, moving, mw, mh, md, bins); !e.empty()) return fail(e);
    const std::string fe = lattice_fit_error(w, cowarp_rules, fw, fh, fd, map, levels, n_levels, D_out, report, impl, scratch, scratch_bytes);
    if (!fe.empty()) return fail(fe);
    return run_on_device_of(D_out, stream, [&](hipStream_t s) {   // map and levels are consumed inside the launcher
        launch_cowarp_fit(fixed, fw, fh, fd, moving, mw, mh, md, bins, map, levels, n_levels, D_out, report, impl, scratch, s);
    });
}
int unet_cowarp_resample(const float* moving, int mw, int mh, int md, int fw, int fh, int fd, const float* map, const int32_t* D, int g,
                         float* out, void* stream) {
    const std::string w = "unet_cowarp_resample: ";
    if (std::string e = ptr_error(w, moving, "moving", 4); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "moving", mw, mh, md); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "fixed", fw, fh, fd); !e.empty()) return fail(e);
    if (!map) return fail(w + "null map");
    if (std::string e = ptr_error(w, D, "D", 4); !e.empty()) return fail(e);
    if (std::string e = cowarp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, out, "out", 4); !e.empty()) return fail(e);
    return run_on_device_of(out, stream, [&](hipStream_t s) { launch_cowarp_resample(moving, mw, mh, md, fw, fh, fd, map, D, g, out, s); });
}

// ---- the geometry of a fitted lattice warp (include/unet_deform.h) ----
static std::string opt_ptr_error(const std::string& w, const void* p, const char* name, int align) {
    return p ? ptr_error(w, p, name, align) : std::string();
}
static_assert(UNET_DEFORM_MAX_DISP == UNET_WARP_MAX_DISP, "a field of either warp");
int unet_deform_jacobian(int sw, int sh, int sd, const float* map, const int32_t* D, int g, float* det, int64_t* info, void* stream) {
    const std::string w = "unet_deform_jacobian: ";
    if (std::string e = grid_dims_error(w, "subject", sw, sh, sd); !e.empty()) return fail(e);
    if (!map) return fail(w + "null map");
    if (std::string e = ptr_error(w, D, "D", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = opt_ptr_error(w, det, "det", 4); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, info, "info", 8); !e.empty()) return fail(e);
    return run_on_device_of(info, stream, [&](hipStream_t s) {   // map is consumed inside the launcher, before this returns
        launch_deform_jacobian(sw, sh, sd, map, D, g, det, info, s);
    });
}
int unet_deform_pull(const void* volume, int kind, int sw, int sh, int sd, int tw, int th, int td, const float* map, const float* inv,
                     const int32_t* D, int g, int iters, void* out, float* pos, int64_t* info, int impl, void* stream) {
    const std::string w = "unet_deform_pull: ";
    if (kind < UNET_DEFORM_KIND_F32 || kind > UNET_DEFORM_KIND_U16) return fail(w + "unknown kind " + std::to_string(kind));
    const int bytes = kind == UNET_DEFORM_KIND_F32 ? 4 : kind == UNET_DEFORM_KIND_U16 ? 2 : 1;
    if (std::string e = ptr_error(w, volume, "volume", bytes); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "subject", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "template", tw, th, td); !e.empty()) return fail(e);
    if (!map) return fail(w + "null map");
    if (!inv) return fail(w + "null inv");
    if (std::string e = opt_ptr_error(w, D, "D", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (iters < 0 || iters > UNET_DEFORM_MAX_ITERS) return fail(w + "iters must be in [0, 32], got " + std::to_string(iters));
    if (std::string e = ptr_error(w, out, "out", bytes); !e.empty()) return fail(e);
    if (std::string e = opt_ptr_error(w, pos, "pos", 4); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, info, "info", 8); !e.empty()) return fail(e);
    if (impl < UNET_DEFORM_IMPL_DEFAULT || impl > UNET_DEFORM_IMPL_TILE) return fail(w + "unknown impl " + std::to_string(impl));
    return run_on_device_of(info, stream, [&](hipStream_t s) {   // map and inv are consumed inside the launcher
        launch_deform_pull(volume, kind, sw, sh, sd, tw, th, td, map, inv, D, g, iters, out, pos, info, impl, s);
    });
}

// ---- the intensity-inhomogeneity correction (include/unet_bias.h) ----
// the levels of a fit: n_levels x {g, sweeps, lam}
static std::string bias_levels_error(const std::string& w, const int* levels, int n_levels) {
    if (n_levels < 1 || n_levels > UNET_BIAS_MAX_LEVELS) return w + "n_levels must be in [1, 4], got " + std::to_string(n_levels);
    if (!levels) return w + "null levels";
    for (int l = 0; l < n_levels; ++l) {
        const int* v = levels + 3 * l;
        const std::string lv = w + "level " + std::to_string(l) + ": ";
        if (std::string e = warp_g_error(lv, v[0]); !e.empty()) return e;
        if (l && 2 * v[0] != levels[3 * (l - 1)]) return lv + "g must be half the level before's, got " + std::to_string(v[0]);
        if (v[1] < 1 || v[1] > UNET_BIAS_MAX_SWEEPS) return lv + "sweeps must be in [1, 16], got " + std::to_string(v[1]);
        if (v[2] < 0 || v[2] > UNET_BIAS_MAX_LAM) return lv + "lam must be in [0, 4096], got " + std::to_string(v[2]);
    }
    return std::string();
}
// q, the labels, the grid and the classes, as levels, residual and fit take them
static std::string bias_labelled_error(const std::string& w, const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd,
                                       const int* classes, int K) {
    if (std::string e = ptr_error(w, q, "q", 4); !e.empty()) return e;
    if (!labels) return w + "null labels";
    if (lbytes != 1 && lbytes != 2) return w + "lbytes must be 1 or 2, got " + std::to_string(lbytes);
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return e;
    if (K < 1 || K > UNET_BIAS_MAX_CLASSES) return w + "K must be in [1, 16], got " + std::to_string(K);
    if (!classes) return w + "null classes";
    for (int k = 0; k < K; ++k) {
        if (classes[k] < 0 || classes[k] > 65535) return w + "classes must be label values in [0, 65535], got " + std::to_string(classes[k]);
        for (int j = 0; j < k; ++j)
            if (classes[j] == classes[k]) return w + "classes must be distinct, got " + std::to_string(classes[k]) + " twice";
    }
    return std::string();
}
static std::string bias_clip_error(const std::string& w, int clip) {
    return clip < 0 || clip > UNET_BIAS_MAX ? w + "clip must be in [0, 8192], got " + std::to_string(clip) : std::string();
}
static std::string bias_scratch_error(const std::string& w, int sw, int sh, int sd, const int* levels, int n_levels, int impl,
                                      const void* scratch, size_t scratch_bytes) {
    if (impl < UNET_BIAS_IMPL_DEFAULT || impl > UNET_BIAS_IMPL_VOXEL) return w + "unknown impl " + std::to_string(impl);
    if (!scratch) return w + "null scratch";
    if (scratch_bytes < bias_scratch_bytes(sw, sh, sd, levels, n_levels)) return w + "scratch too small (see unet_bias_scratch_bytes)";
    return std::string();
}
int unet_bias_lattice(int sw, int sh, int sd, int g, int* nx, int* ny, int* nz) {
    const std::string w = "unet_bias_lattice: ";
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (!nx || !ny || !nz) return fail(w + "null output");
    *nx = (sw + g - 1) / g + 1;
    *ny = (sh + g - 1) / g + 1;
    *nz = (sd + g - 1) / g + 1;
    return 0;
}
int unet_bias_scratch_bytes(int sw, int sh, int sd, const int* levels, int n_levels, size_t* bytes) {
    const std::string w = "unet_bias_scratch_bytes: ";
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = bias_levels_error(w, levels, n_levels); !e.empty()) return fail(e);
    if (!bytes) return fail(w + "null output");
    *bytes = bias_scratch_bytes(sw, sh, sd, levels, n_levels);
    return 0;
}
int unet_bias_logcode(const float* v, int64_t voxels, int32_t* q, void* stream) {
    const std::string w = "unet_bias_logcode: ";
    if (std::string e = ptr_error(w, v, "v", 4); !e.empty()) return fail(e);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail(w + "voxels must be in [1, 2^31), got " + std::to_string(voxels));
    if (std::string e = ptr_error(w, q, "q", 4); !e.empty()) return fail(e);
    return run_on_device_of(q, stream, [&](hipStream_t s) { launch_bias_logcode(v, voxels, q, s); });
}
int unet_bias_levels(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, const int32_t* B,
                     int g, int64_t* levels_out, void* stream) {
    const std::string w = "unet_bias_levels: ";
    if (std::string e = bias_labelled_error(w, q, labels, lbytes, sw, sh, sd, classes, K); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, B, "B", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, levels_out, "levels_out", 8); !e.empty()) return fail(e);
    return run_on_device_of(levels_out, stream, [&](hipStream_t s) {   // classes is consumed inside the launcher, before this returns
        launch_bias_levels(q, labels, lbytes, sw, sh, sd, classes, K, B, g, levels_out, s);
    });
}
int unet_bias_residual(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K,
                       const int64_t* levels_in, int clip, int16_t* r, void* stream) {
    const std::string w = "unet_bias_residual: ";
    if (std::string e = bias_labelled_error(w, q, labels, lbytes, sw, sh, sd, classes, K); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, levels_in, "levels_in", 8); !e.empty()) return fail(e);
    if (std::string e = bias_clip_error(w, clip); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, r, "r", 16); !e.empty()) return fail(e);
    return run_on_device_of(r, stream, [&](hipStream_t s) {
        launch_bias_residual(q, labels, lbytes, sw, sh, sd, classes, K, levels_in, clip, r, s);
    });
}
int unet_bias_sweep(const int16_t* r, int sw, int sh, int sd, int32_t* B, int g, int lam, int64_t* info, int impl, void* scratch,
                    size_t scratch_bytes, void* stream) {
    const std::string w = "unet_bias_sweep: ";
    if (std::string e = ptr_error(w, r, "r", 16); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, B, "B", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (lam < 0 || lam > UNET_BIAS_MAX_LAM) return fail(w + "lam must be in [0, 4096], got " + std::to_string(lam));
    if (std::string e = ptr_error(w, info, "info", 8); !e.empty()) return fail(e);
    if (impl < UNET_BIAS_IMPL_DEFAULT || impl > UNET_BIAS_IMPL_VOXEL) return fail(w + "unknown impl " + std::to_string(impl));
    if (!scratch) return fail(w + "null scratch");
    if (scratch_bytes < bias_sweep_scratch_bytes(sw, sh, sd, g)) return fail(w + "scratch too small (256 + 16 bytes per node, rounded up to 256)");
    return run_on_device_of(B, stream, [&](hipStream_t s) { launch_bias_sweep(r, sw, sh, sd, B, g, lam, info, impl, scratch, s); });
}
int unet_bias_refine(const int32_t* B_coarse, int sw, int sh, int sd, int g, int32_t* B_fine, void* stream) {
    const std::string w = "unet_bias_refine: ";
    if (std::string e = ptr_error(w, B_coarse, "B_coarse", 4); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (g != 8 && g != 16 && g != 32) return fail(w + "g must be 8, 16 or 32, got " + std::to_string(g));
    if (std::string e = ptr_error(w, B_fine, "B_fine", 4); !e.empty()) return fail(e);
    return run_on_device_of(B_fine, stream, [&](hipStream_t s) { launch_bias_refine(B_coarse, sw, sh, sd, g, B_fine, s); });
}
int unet_bias_cost(const int16_t* r, int sw, int sh, int sd, const int32_t* B, int g, int64_t* cost, void* stream) {
    const std::string w = "unet_bias_cost: ";
    if (std::string e = ptr_error(w, r, "r", 2); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, B, "B", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, cost, "cost", 8); !e.empty()) return fail(e);
    return run_on_device_of(cost, stream, [&](hipStream_t s) { launch_bias_cost(r, sw, sh, sd, B, g, cost, s); });
}
int unet_bias_fit(const int32_t* q, const void* labels, int lbytes, int sw, int sh, int sd, const int* classes, int K, int clip,
                  const int* levels, int n_levels, int outer, int32_t* B_out, int64_t* report, int impl, void* scratch, size_t scratch_bytes,
                  void* stream) {
    const std::string w = "unet_bias_fit: ";
    if (std::string e = bias_labelled_error(w, q, labels, lbytes, sw, sh, sd, classes, K); !e.empty()) return fail(e);
    if (std::string e = bias_clip_error(w, clip); !e.empty()) return fail(e);
    if (std::string e = bias_levels_error(w, levels, n_levels); !e.empty()) return fail(e);
    if (outer < 1 || outer > UNET_BIAS_MAX_OUTER) return fail(w + "outer must be in [1, 8], got " + std::to_string(outer));
    if (std::string e = ptr_error(w, B_out, "B_out", 4); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, report, "report", 8); !e.empty()) return fail(e);
    if (std::string e = bias_scratch_error(w, sw, sh, sd, levels, n_levels, impl, scratch, scratch_bytes); !e.empty()) return fail(e);
    return run_on_device_of(B_out, stream, [&](hipStream_t s) {   // classes and levels are consumed inside the launcher
        launch_bias_fit(q, labels, lbytes, sw, sh, sd, classes, K, clip, levels, n_levels, outer, B_out, report, impl, scratch, s);
    });
}
static_assert(UNET_BIAS_MAX_LEVELS * UNET_BIAS_MAX_OUTER <= UNET_BIAS_MAX_ROWS, "a row per (level, outer round)");
int unet_bias_apply(const float* v, int sw, int sh, int sd, const int32_t* B, int g, float* out, float* gain, void* stream) {
    const std::string w = "unet_bias_apply: ";
    if (std::string e = opt_ptr_error(w, v, "v", 4); !e.empty()) return fail(e);
    if (std::string e = grid_dims_error(w, "volume", sw, sh, sd); !e.empty()) return fail(e);
    if (std::string e = ptr_error(w, B, "B", 4); !e.empty()) return fail(e);
    if (std::string e = warp_g_error(w, g); !e.empty()) return fail(e);
    if (std::string e = opt_ptr_error(w, out, "out", 4); !e.empty()) return fail(e);
    if (std::string e = opt_ptr_error(w, gain, "gain", 4); !e.empty()) return fail(e);
    if (!out && !gain) return fail(w + "null out and null gain: nothing to form");
    if (!v != !out) return fail(w + "v and out go together: both or neither");
    return run_on_device_of(B, stream, [&](hipStream_t s) { launch_bias_apply(v, sw, sh, sd, B, g, out, gain, s); });
}

// ---- the tables of a label map (include/unet_table.h) ----
static std::string table_common_error(const std::string& w, int64_t voxels, int n_labels, const int64_t* rows, int impl, const void* scratch,
                                      size_t scratch_bytes) {
    if (voxels >= ((int64_t)1 << 31)) return w + "the grid must stay below 2^31 voxels";
    if (n_labels < 1 || n_labels > UNET_TABLE_MAX_LABELS) return w + "n_labels must be in [1, 65535], got " + std::to_string(n_labels);
    if (std::string e = ptr_error(w, rows, "rows", 8); !e.empty()) return e;
    if (impl < UNET_TABLE_IMPL_DEFAULT || impl > UNET_TABLE_IMPL_GLOBAL) return w + "unknown impl " + std::to_string(impl);
    if (!scratch) return w + "null scratch";
    if (scratch_bytes < table_scratch_bytes(n_labels)) return w + "scratch too small (see unet_table_scratch_bytes)";
    return std::string();
}
int unet_table_scratch_bytes(int64_t voxels, int n_labels, size_t* bytes) {
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail("unet_table: voxels must be in [1, 2^31)");
    if (n_labels < 1 || n_labels > UNET_TABLE_MAX_LABELS) return fail("unet_table: n_labels must be in [1, 65535], got " + std::to_string(n_labels));
    if (!bytes) return fail("unet_table_scratch_bytes: null output");
    *bytes = table_scratch_bytes(n_labels);   // the running table: nothing per voxel
    return 0;
}
int unet_table_regions(const void* labels, int label_bytes, int w, int h, int d, int n_labels, int64_t* rows, int impl, void* scratch,
                       size_t scratch_bytes, void* stream) {
    const std::string who = "unet_table_regions: ";
    if (!labels) return fail(who + "null labels");
    if (label_bytes != 1 && label_bytes != 2) return fail(who + "label_bytes must be 1 or 2, got " + std::to_string(label_bytes));
    if (w <= 0 || h <= 0 || d <= 0) return fail(who + "dimensions must be positive");
    const std::string e = table_common_error(who, (int64_t)w * h * d, n_labels, rows, impl, scratch, scratch_bytes);
    if (!e.empty()) return fail(e);
    return run_on_device_of(labels, stream, [&](hipStream_t s) {
        launch_table_regions(labels, label_bytes, w, h, d, n_labels, rows, impl, scratch, s);
    });
}
int unet_table_overlap(const void* a, int a_bytes, const void* b, int b_bytes, int64_t voxels, int n_labels, int64_t* rows, int impl,
                       void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_table_overlap: ";
    if (!a) return fail(who + "null a");
    if (!b) return fail(who + "null b");
    if (a_bytes != 1 && a_bytes != 2) return fail(who + "a_bytes must be 1 or 2, got " + std::to_string(a_bytes));
    if (b_bytes != 1 && b_bytes != 2) return fail(who + "b_bytes must be 1 or 2, got " + std::to_string(b_bytes));
    if (voxels <= 0) return fail(who + "voxels must be positive");
    const std::string e = table_common_error(who, voxels, n_labels, rows, impl, scratch, scratch_bytes);
    if (!e.empty()) return fail(e);
    return run_on_device_of(a, stream, [&](hipStream_t s) {
        launch_table_overlap(a, a_bytes, b, b_bytes, voxels, n_labels, rows, impl, scratch, s);
    });
}

// ---- the per-region intensity statistics (include/unet_stats.h) ----
// everything the three calls share, in the order the header lists it; scale: 65536.0f / (hi - lo) in fp32, one subtraction, one division
static std::string stats_common_error(const std::string& w, const void* labels, int label_bytes, const float* image, int64_t voxels,
                                      int n_labels, int max_labels, float lo, float hi, const void* rows, const char* rows_name, int rows_align,
                                      int impl, float* scale) {
    if (std::string e = ptr_error(w, image, "image", 4); !e.empty()) return e;
    if (!labels && n_labels != 0) return w + "n_labels must be 0 when labels is null, got " + std::to_string(n_labels);
    if (labels && (n_labels < 1 || n_labels > max_labels))
        return w + "n_labels must be in [1, " + std::to_string(max_labels) + "] when labels is given, got " + std::to_string(n_labels);
    if (labels && label_bytes != 1 && label_bytes != 2) return w + "label_bytes must be 1 or 2, got " + std::to_string(label_bytes);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return w + "voxels must be in [1, 2^31)";
    if (!std::isfinite(lo) || !std::isfinite(hi)) return w + "lo and hi must be finite";
    if (!(lo < hi)) return w + "lo must be below hi";
    const float diff = hi - lo;
    *scale = 65536.0f / diff;
    if (!std::isfinite(diff) || !std::isfinite(*scale) || !(*scale > 0.f)) return w + "the scale 65536 / (hi - lo) must be finite";
    if (std::string e = ptr_error(w, rows, rows_name, rows_align); !e.empty()) return e;
    if (impl < UNET_STATS_IMPL_DEFAULT || impl > UNET_STATS_IMPL_GLOBAL) return w + "unknown impl " + std::to_string(impl);
    return std::string();
}
static std::string stats_scratch_error(const std::string& w, const void* scratch, size_t scratch_bytes, int n_labels, int n_quantiles) {
    if (!scratch) return w + "null scratch";
    if (scratch_bytes < stats_scratch_bytes(n_labels, n_quantiles)) return w + "scratch too small (see unet_stats_scratch_bytes)";
    return std::string();
}
int unet_stats_scratch_bytes(int64_t voxels, int n_labels, int n_quantiles, size_t* bytes) {
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail("unet_stats: voxels must be in [1, 2^31)");
    if (n_quantiles < 0 || n_quantiles > UNET_STATS_MAX_QUANTILES) return fail("unet_stats: n_quantiles must be in [0, 8], got " + std::to_string(n_quantiles));
    const int max_labels = n_quantiles ? UNET_STATS_MAX_QUANTILE_LABELS : UNET_STATS_MAX_LABELS;
    if (n_labels < 0 || n_labels > max_labels)
        return fail("unet_stats: n_labels must be in [0, " + std::to_string(max_labels) + "], got " + std::to_string(n_labels));
    if (!bytes) return fail("unet_stats_scratch_bytes: null output");
    *bytes = stats_scratch_bytes(n_labels, n_quantiles);   // the running tables: nothing per voxel
    return 0;
}
int unet_stats_moments(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                       int64_t* rows, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_stats_moments: ";
    float scale = 0.f;
    std::string e = stats_common_error(who, labels, label_bytes, image, voxels, n_labels, UNET_STATS_MAX_LABELS, lo, hi, rows, "rows", 8, impl, &scale);
    if (e.empty()) e = stats_scratch_error(who, scratch, scratch_bytes, n_labels, 0);
    if (!e.empty()) return fail(e);
    return run_on_device_of(image, stream, [&](hipStream_t s) {
        launch_stats_moments(labels, label_bytes, image, voxels, n_labels, lo, hi, scale, rows, impl, scratch, s);
    });
}
int unet_stats_hist(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                    int64_t* rows, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_stats_hist: ";
    float scale = 0.f;
    std::string e = stats_common_error(who, labels, label_bytes, image, voxels, n_labels, UNET_STATS_MAX_QUANTILE_LABELS, lo, hi, rows, "rows", 8,
                                       impl, &scale);
    if (e.empty()) e = stats_scratch_error(who, scratch, scratch_bytes, n_labels, 0);
    if (!e.empty()) return fail(e);
    return run_on_device_of(image, stream, [&](hipStream_t s) {
        launch_stats_hist(labels, label_bytes, image, voxels, n_labels, lo, hi, scale, rows, impl, scratch, s);
    });
}
int unet_stats_quantiles(const void* labels, int label_bytes, const float* image, int64_t voxels, int n_labels, float lo, float hi,
                         const int* permille, int n_quantiles, int32_t* out, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_stats_quantiles: ";
    float scale = 0.f;
    if (!permille) return fail(who + "null permille");
    if (n_quantiles < 1 || n_quantiles > UNET_STATS_MAX_QUANTILES) return fail(who + "n_quantiles must be in [1, 8], got " + std::to_string(n_quantiles));
    for (int k = 0; k < n_quantiles; ++k)
        if (permille[k] < 0 || permille[k] > 1000)
            return fail(who + "permille[" + std::to_string(k) + "] must be in [0, 1000], got " + std::to_string(permille[k]));
    std::string e = stats_common_error(who, labels, label_bytes, image, voxels, n_labels, UNET_STATS_MAX_QUANTILE_LABELS, lo, hi, out, "out", 4,
                                       impl, &scale);
    if (e.empty()) e = stats_scratch_error(who, scratch, scratch_bytes, n_labels, n_quantiles);
    if (!e.empty()) return fail(e);
    return run_on_device_of(image, stream, [&](hipStream_t s) {   // permille is consumed inside the launcher
        launch_stats_quantiles(labels, label_bytes, image, voxels, n_labels, lo, hi, scale, permille, n_quantiles, out, impl, scratch, s);
    });
}

// ---- the calibration tables (include/unet_calib.h) ----
static std::string calib_size_error(const std::string& w, int out_c, int64_t voxels) {
    if (out_c < 2 || out_c > UNET_CALIB_MAX_CLASSES)
        return w + "out_c must be in [2, " + std::to_string(UNET_CALIB_MAX_CLASSES) + "], got " + std::to_string(out_c);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return w + "voxels must be in [1, 2^31), got " + std::to_string(voxels);
    return std::string();
}
int unet_calib_table_len(int out_c, size_t* count) {
    const std::string who = "unet_calib_table_len: ";
    if (std::string e = calib_size_error(who, out_c, 1); !e.empty()) return fail(e);
    if (!count) return fail(who + "null count");
    *count = calib_table_len(out_c);
    return 0;
}
int unet_calib_scratch_bytes(int out_c, int64_t voxels, size_t* bytes) {
    const std::string who = "unet_calib_scratch_bytes: ";
    if (std::string e = calib_size_error(who, out_c, voxels); !e.empty()) return fail(e);
    if (!bytes) return fail(who + "null bytes");
    *bytes = calib_scratch_bytes(out_c);   // the running table: nothing per voxel
    return 0;
}
int unet_calib_tables(const float* src, int src_kind, int out_c, int64_t voxels, const float* label, const uint8_t* mask, int accumulate,
                      int64_t* tables, uint8_t* wrong, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_calib_tables: ";
    std::string e = ptr_error(who, src, "src", 4);
    if (e.empty() && src_kind != UNET_CALIB_SRC_LOGITS && src_kind != UNET_CALIB_SRC_PROBS) e = who + "unknown src_kind " + std::to_string(src_kind);
    if (e.empty()) e = calib_size_error(who, out_c, voxels);
    if (e.empty()) e = ptr_error(who, label, "label", 4);
    if (e.empty()) e = ptr_error(who, tables, "tables", 8);
    if (e.empty() && (impl < UNET_CALIB_IMPL_DEFAULT || impl > UNET_CALIB_IMPL_GLOBAL)) e = who + "unknown impl " + std::to_string(impl);
    if (e.empty() && !scratch) e = who + "null scratch";
    if (e.empty() && scratch_bytes < calib_scratch_bytes(out_c)) e = who + "scratch too small (see unet_calib_scratch_bytes)";
    if (!e.empty()) return fail(e);
    return run_on_device_of(src, stream, [&](hipStream_t s) {
        launch_calib_tables(src, src_kind, out_c, voxels, label, mask, accumulate, tables, wrong, impl, scratch, s);
    });
}

// ---- the recalibration pass (include/unet_recal.h) ----
static std::string recal_size_error(const std::string& w, int out_c, int64_t voxels) {
    if (out_c < 2 || out_c > UNET_RECAL_MAX_CLASSES)
        return w + "out_c must be in [2, " + std::to_string(UNET_RECAL_MAX_CLASSES) + "], got " + std::to_string(out_c);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return w + "voxels must be in [1, 2^31), got " + std::to_string(voxels);
    return std::string();
}
int unet_recal_scratch_bytes(int out_c, int64_t voxels, size_t* bytes) {
    const std::string who = "unet_recal_scratch_bytes: ";
    if (std::string e = recal_size_error(who, out_c, voxels); !e.empty()) return fail(e);
    if (!bytes) return fail(who + "null bytes");
    *bytes = recal_scratch_bytes();   // the running table: nothing per voxel or class
    return 0;
}
int unet_recal_eval(const float* logits, int out_c, int64_t voxels, const float* label, const uint8_t* mask, const float* betas, int n_betas,
                    int accumulate, int64_t* tables, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_recal_eval: ";
    std::string e = ptr_error(who, logits, "logits", 4);
    if (e.empty()) e = recal_size_error(who, out_c, voxels);
    if (e.empty()) e = ptr_error(who, label, "label", 4);
    if (e.empty() && !betas) e = who + "null betas";
    if (e.empty() && (n_betas < 1 || n_betas > UNET_RECAL_MAX_BETAS))
        e = who + "n_betas must be in [1, " + std::to_string(UNET_RECAL_MAX_BETAS) + "], got " + std::to_string(n_betas);
    for (int k = 0; e.empty() && k < n_betas; ++k)
        if (!std::isfinite(betas[k]) || !(betas[k] > 0.f))
            e = who + "betas[" + std::to_string(k) + "] must be finite and positive, got " + std::to_string(betas[k]);
    if (e.empty()) e = ptr_error(who, tables, "tables", 8);
    if (e.empty() && !scratch) e = who + "null scratch";
    if (e.empty() && scratch_bytes < recal_scratch_bytes()) e = who + "scratch too small (see unet_recal_scratch_bytes)";
    if (!e.empty()) return fail(e);
    return run_on_device_of(logits, stream, [&](hipStream_t s) {   // betas is consumed inside the launcher
        launch_recal_eval(logits, out_c, voxels, label, mask, betas, n_betas, accumulate, tables, scratch, s);
    });
}

// ---- the boundary distances of label maps (include/unet_distance.h) ----
static std::string dist_grid_error(const std::string& w_, const void* map, const char* name, int bytes, int w, int h, int d) {
    if (!map) return w_ + "null " + name;
    if (bytes != 1 && bytes != 2) return w_ + name + "_bytes must be 1 or 2, got " + std::to_string(bytes);
    if (w <= 0 || h <= 0 || d <= 0) return w_ + "dimensions (w, h, d) must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return w_ + "the grid (w, h, d) must stay below 2^31 voxels";
    return std::string();
}
static std::string dist_label_error(const std::string& w_, const char* name, int label) {
    if (label < 1 || label > UNET_DIST_MAX_LABEL) return w_ + name + " must be in [1, 65535], got " + std::to_string(label);
    return std::string();
}
int unet_dist_scratch_bytes(int w, int h, int d, size_t* bytes) {
    if (w <= 0 || h <= 0 || d <= 0) return fail("unet_dist_scratch_bytes: dimensions (w, h, d) must be positive");
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return fail("unet_dist_scratch_bytes: the grid (w, h, d) must stay below 2^31 voxels");
    if (!bytes) return fail("unet_dist_scratch_bytes: null bytes");
    *bytes = dist_scratch_bytes((int64_t)w * h * d);   // one int32 per voxel between the passes
    return 0;
}
int unet_dist_transform(const void* labels, int label_bytes, int w, int h, int d, int label, int of, int wx, int wy, int wz, int32_t* out,
                        int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_dist_transform: ";
    std::string e = dist_grid_error(who, labels, "label", label_bytes, w, h, d);
    if (!labels) e = who + "null labels";
    if (e.empty()) e = dist_label_error(who, "label", label);
    if (!e.empty()) return fail(e);
    if (of != UNET_DIST_OF_SURFACE && of != UNET_DIST_OF_LABEL) return fail(who + "unknown of " + std::to_string(of));
    if (wx <= 0 || wy <= 0 || wz <= 0)
        return fail(who + "weights (wx, wy, wz) must be positive, got " + std::to_string(wx) + ", " + std::to_string(wy) + ", " + std::to_string(wz));
    // the largest squared distance of the grid, in 128 bits: each term stays below 2^31 * 2^62
    const auto sq = [](int n) { return (unsigned __int128)((uint64_t)(n - 1) * (uint64_t)(n - 1)); };
    if (sq(w) * (unsigned)wx + sq(h) * (unsigned)wy + sq(d) * (unsigned)wz >= (unsigned __int128)UNET_DIST_INF)
        return fail(who + "weights (wx, wy, wz): wx (w-1)^2 + wy (h-1)^2 + wz (d-1)^2 must stay below 2^31 - 1");
    e = ptr_error(who, out, "out", 4);
    if (!e.empty()) return fail(e);
    if (impl < UNET_DIST_IMPL_DEFAULT || impl > UNET_DIST_IMPL_GLOBAL) return fail(who + "unknown impl " + std::to_string(impl));
    if (!scratch) return fail(who + "null scratch");
    if (scratch_bytes < dist_scratch_bytes((int64_t)w * h * d)) return fail(who + "scratch too small (see unet_dist_scratch_bytes)");
    return run_on_device_of(labels, stream, [&](hipStream_t s) {
        launch_dist_transform(labels, label_bytes, w, h, d, label, of, wx, wy, wz, out, impl, scratch, s);
    });
}
int unet_dist_surface_counts(const void* a, int a_bytes, const void* b, int b_bytes, int w, int h, int d, int n_labels, int64_t* rows,
                             void* stream) {
    const std::string who = "unet_dist_surface_counts: ";
    std::string e = dist_grid_error(who, a, "a", a_bytes, w, h, d);
    if (e.empty()) e = dist_grid_error(who, b, "b", b_bytes, w, h, d);
    if (e.empty()) e = dist_label_error(who, "n_labels", n_labels);
    if (e.empty()) e = ptr_error(who, rows, "rows", 8);
    if (!e.empty()) return fail(e);
    return run_on_device_of(a, stream, [&](hipStream_t s) { launch_dist_surface_counts(a, a_bytes, b, b_bytes, w, h, d, n_labels, rows, s); });
}
int unet_dist_gather(const void* at, int at_bytes, int w, int h, int d, int label, const int32_t* dist, int32_t* values, int64_t capacity,
                     unsigned long long* cursor, void* stream) {
    const std::string who = "unet_dist_gather: ";
    std::string e = dist_grid_error(who, at, "at", at_bytes, w, h, d);
    if (e.empty()) e = dist_label_error(who, "label", label);
    if (e.empty()) e = ptr_error(who, dist, "dist", 4);
    if (e.empty()) e = ptr_error(who, values, "values", 4);
    if (e.empty() && capacity < 0) e = who + "capacity must not be negative, got " + std::to_string(capacity);
    if (e.empty()) e = ptr_error(who, cursor, "cursor", 8);
    if (!e.empty()) return fail(e);
    return run_on_device_of(at, stream, [&](hipStream_t s) { launch_dist_gather(at, at_bytes, w, h, d, label, dist, values, capacity, cursor, s); });
}

// ---- the instances of a label map (include/unet_instances.h) ----
static std::string inst_size_error(const std::string& w, int64_t voxels, int n_classes, int64_t max_instances) {
    const std::string e = labelling_size_error(w, voxels, n_classes);
    if (!e.empty()) return e;
    if (max_instances < 0 || max_instances > UNET_INST_MAX_INSTANCES)
        return w + "max_instances must be in [0, 2147483646], got " + std::to_string(max_instances);
    return std::string();
}
// unet_inst_scratch_bytes and unet_conn_label_scratch_bytes
static int inst_scratch_query(const std::string& who, int64_t voxels, int n_classes, int64_t max_instances, size_t* bytes) {
    const std::string e = inst_size_error(who, voxels, n_classes, max_instances);
    if (!e.empty()) return fail(e);
    if (!bytes) return fail(who + "null bytes");
    *bytes = inst_scratch_bytes(voxels, n_classes, max_instances);
    return 0;
}
// unet_inst_label (connectivity 6: that check cannot fire) and unet_conn_label; sizes: the scratch-size call the text names
static int inst_label_call(const std::string& who, const char* sizes, int w, int h, int d, const uint16_t* label, int n_classes,
                           const uint32_t* listed, int n_listed, int32_t* inst, int64_t* rows, int64_t max_instances, int64_t* info,
                           int connectivity, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    if (w <= 0 || h <= 0 || d <= 0) return fail(who + "dimensions (w, h, d) must be positive");
    std::string e = inst_size_error(who, (int64_t)w * h * d, n_classes, max_instances);
    if (e.empty() && !label) e = who + "null label";
    if (e.empty() && n_listed < 0) e = who + "n_listed must not be negative, got " + std::to_string(n_listed);
    if (e.empty() && n_listed > 0 && !listed) e = who + "null listed";
    if (e.empty()) e = ptr_error(who, inst, "inst", 4);
    if (e.empty()) e = ptr_error(who, rows, "rows", 8);
    if (e.empty()) e = ptr_error(who, info, "info", 8);
    if (e.empty()) e = conn_error(who, connectivity, impl);
    if (e.empty() && !scratch) e = who + "null scratch";
    if (e.empty() && scratch_bytes < inst_scratch_bytes((int64_t)w * h * d, n_classes, max_instances))
        e = who + "scratch too small (see " + sizes + ")";
    if (e.empty()) e = listed_range_error(who, listed, n_listed, n_classes);
    if (!e.empty()) return fail(e);
    const std::vector<uint32_t> classes = listed_classes(listed, n_listed);
    return run_on_device_of(label, stream, [&](hipStream_t s) {
        launch_inst_label(w, h, d, label, n_classes, classes.data(), (int)classes.size(), inst, rows, max_instances, info, impl, connectivity,
                          scratch, s);
    });
}
int unet_inst_scratch_bytes(int64_t voxels, int n_classes, int64_t max_instances, size_t* bytes) {
    return inst_scratch_query("unet_inst_scratch_bytes: ", voxels, n_classes, max_instances, bytes);
}
int unet_inst_label(int w, int h, int d, const uint16_t* label, int n_classes, const uint32_t* listed, int n_listed, int32_t* inst,
                    int64_t* rows, int64_t max_instances, int64_t* info, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    return inst_label_call("unet_inst_label: ", "unet_inst_scratch_bytes", w, h, d, label, n_classes, listed, n_listed, inst, rows,
                           max_instances, info, 6, impl, scratch, scratch_bytes, stream);
}
int unet_inst_match_scratch_bytes(int64_t max_pairs, size_t* bytes) {
    if (max_pairs < 0 || max_pairs > UNET_INST_MAX_PAIRS)
        return fail("unet_inst_match_scratch_bytes: max_pairs must be in [0, 2^30], got " + std::to_string(max_pairs));
    if (!bytes) return fail("unet_inst_match_scratch_bytes: null bytes");
    *bytes = inst_match_scratch_bytes(max_pairs);
    return 0;
}
int unet_inst_match(const int32_t* ia, const int32_t* ib, int64_t voxels, uint64_t* keys, int64_t* counts, int64_t max_pairs, int64_t* info,
                    int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_inst_match: ";
    std::string e = ptr_error(who, ia, "ia", 4);
    if (e.empty()) e = ptr_error(who, ib, "ib", 4);
    if (!e.empty()) return fail(e);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail(who + "voxels must be in [1, 2^31), got " + std::to_string(voxels));
    if (max_pairs < 0 || max_pairs > UNET_INST_MAX_PAIRS) return fail(who + "max_pairs must be in [0, 2^30], got " + std::to_string(max_pairs));
    // keys and counts may be null only when they hold nothing
    if (max_pairs > 0 || keys) e = ptr_error(who, keys, "keys", 8);
    if (e.empty() && (max_pairs > 0 || counts)) e = ptr_error(who, counts, "counts", 8);
    if (e.empty()) e = ptr_error(who, info, "info", 8);
    if (!e.empty()) return fail(e);
    if (impl < UNET_INST_IMPL_DEFAULT || impl > UNET_INST_IMPL_GLOBAL) return fail(who + "unknown impl " + std::to_string(impl));
    if (!scratch) return fail(who + "null scratch");
    if (scratch_bytes < inst_match_scratch_bytes(max_pairs)) return fail(who + "scratch too small (see unet_inst_match_scratch_bytes)");
    return run_on_device_of(ia, stream, [&](hipStream_t s) {
        launch_inst_match(ia, ib, voxels, (unsigned long long*)keys, counts, max_pairs, info, impl, scratch, s);
    });
}
int unet_inst_remove_small(uint16_t* label, const int32_t* inst, int64_t voxels, const int64_t* rows, int64_t max_instances,
                           int64_t min_voxels, uint32_t* removed, int n_classes, void* stream) {
    const std::string who = "unet_inst_remove_small: ";
    std::string e = ptr_error(who, label, "label", 2);
    if (e.empty()) e = ptr_error(who, inst, "inst", 4);
    if (e.empty()) e = ptr_error(who, rows, "rows", 8);
    if (!e.empty()) return fail(e);
    if (voxels <= 0 || voxels >= ((int64_t)1 << 31)) return fail(who + "voxels must be in [1, 2^31), got " + std::to_string(voxels));
    if (max_instances < 0 || max_instances > UNET_INST_MAX_INSTANCES)
        return fail(who + "max_instances must be in [0, 2147483646], got " + std::to_string(max_instances));
    if (removed) {
        if ((uintptr_t)removed & 3) return fail(who + "removed must be 4-byte aligned");
        if (n_classes < 1 || n_classes > 65536) return fail(who + "n_classes must be in [1, 65536], got " + std::to_string(n_classes));
    }
    return run_on_device_of(label, stream, [&](hipStream_t s) {
        launch_inst_remove_small(label, inst, voxels, rows, max_instances, min_voxels, removed, n_classes, s);
    });
}

// ---- binary morphology on bit-packed masks (include/unet_morph.h) ----
static std::string morph_grid_error(const std::string& w_, int w, int h, int d) {
    if (w <= 0 || h <= 0 || d <= 0) return w_ + "dimensions (w, h, d) must be positive";
    if ((int64_t)w * h * d >= ((int64_t)1 << 31)) return w_ + "voxels must be in [1, 2^31), got " + std::to_string((int64_t)w * h * d);
    return std::string();
}
static std::string morph_scratch_error(const std::string& w_, int w, int h, int d, const void* scratch, size_t scratch_bytes) {
    if (!scratch) return w_ + "null scratch";
    if (scratch_bytes < morph_scratch_bytes(w, h, d)) return w_ + "scratch too small (see unet_morph_scratch_bytes)";
    return std::string();
}
// unet_morph_scratch_bytes and unet_conn_holes_scratch_bytes
static int morph_scratch_query(const std::string& who, int w, int h, int d, size_t* bytes) {
    const std::string e = morph_grid_error(who, w, h, d);
    if (!e.empty()) return fail(e);
    if (!bytes) return fail(who + "null bytes");
    *bytes = morph_scratch_bytes(w, h, d);
    return 0;
}
int unet_morph_scratch_bytes(int w, int h, int d, size_t* bytes) { return morph_scratch_query("unet_morph_scratch_bytes: ", w, h, d, bytes); }
int unet_morph_pack(int w, int h, int d, const void* labels, int label_bytes, int n_classes, const uint32_t* listed, int n_listed,
                    uint64_t* bits, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_morph_pack: ";
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty() && !labels) e = who + "null labels";
    if (e.empty() && label_bytes != 1 && label_bytes != 2) e = who + "label_bytes must be 1 or 2, got " + std::to_string(label_bytes);
    if (e.empty() && (n_classes < 1 || n_classes > 65536)) e = who + "n_classes must be in [1, 65536], got " + std::to_string(n_classes);
    if (e.empty() && n_listed < 0) e = who + "n_listed must not be negative, got " + std::to_string(n_listed);
    if (e.empty() && n_listed > 0 && !listed) e = who + "null listed";
    if (e.empty()) e = ptr_error(who, bits, "bits", 8);
    if (e.empty()) e = morph_scratch_error(who, w, h, d, scratch, scratch_bytes);
    if (e.empty()) e = listed_range_error(who, listed, n_listed, n_classes);
    if (!e.empty()) return fail(e);
    std::vector<uint32_t> classes(listed, listed + n_listed);   // the caller's list is consumed here, in its order
    return run_on_device_of(labels, stream, [&](hipStream_t s) {
        launch_morph_pack(w, h, d, labels, label_bytes, n_classes, classes.data(), (int)classes.size(), bits, scratch, s);
    });
}
int unet_morph_unpack(int w, int h, int d, const uint64_t* bits, uint8_t* mask, void* stream) {
    const std::string who = "unet_morph_unpack: ";
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty()) e = ptr_error(who, bits, "bits", 8);
    if (e.empty() && !mask) e = who + "null mask";
    if (!e.empty()) return fail(e);
    return run_on_device_of(bits, stream, [&](hipStream_t s) { launch_morph_unpack(w, h, d, bits, mask, s); });
}
int unet_morph_count(int w, int h, int d, const uint64_t* bits, int64_t* count, void* stream) {
    const std::string who = "unet_morph_count: ";
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty()) e = ptr_error(who, bits, "bits", 8);
    if (e.empty()) e = ptr_error(who, count, "count", 8);
    if (!e.empty()) return fail(e);
    return run_on_device_of(bits, stream, [&](hipStream_t s) { launch_morph_count(w, h, d, bits, count, s); });
}
int unet_morph_step(int w, int h, int d, const uint64_t* in, uint64_t* out, int op, int connectivity, int iterations, int border, int impl,
                    void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_morph_step: ";
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty()) e = ptr_error(who, in, "in", 8);
    if (e.empty()) e = ptr_error(who, out, "out", 8);
    if (e.empty() && in == out) e = who + "in and out must not be the same mask";
    if (e.empty() && op != UNET_MORPH_DILATE && op != UNET_MORPH_ERODE) e = who + "unknown op " + std::to_string(op);
    if (e.empty() && connectivity != 6 && connectivity != 18 && connectivity != 26)
        e = who + "connectivity must be 6, 18 or 26, got " + std::to_string(connectivity);
    if (e.empty() && (iterations < 0 || iterations > UNET_MORPH_MAX_ITERATIONS))
        e = who + "iterations must be in [0, 255], got " + std::to_string(iterations);
    if (e.empty() && border != 0 && border != 1) e = who + "border must be 0 or 1, got " + std::to_string(border);
    if (e.empty() && (impl < UNET_MORPH_IMPL_DEFAULT || impl > UNET_MORPH_IMPL_GLOBAL)) e = who + "unknown impl " + std::to_string(impl);
    if (e.empty()) e = morph_scratch_error(who, w, h, d, scratch, scratch_bytes);
    if (!e.empty()) return fail(e);
    if (impl == UNET_MORPH_IMPL_DEFAULT) impl = UNET_MORPH_IMPL_GLOBAL;   // the faster as measured
    return run_on_device_of(in, stream, [&](hipStream_t s) {
        launch_morph_step(w, h, d, in, out, op, connectivity, iterations, border, impl, scratch, s);
    });
}
// unet_morph_holes (connectivity 6: that check cannot fire) and unet_conn_holes; impl is checked as the caller's header gives it,
// labelling is what the caller mapped it to; sizes: the scratch-size call the text names
static int holes_call(const std::string& who, const char* sizes, int w, int h, int d, const uint64_t* in, uint64_t* out, int64_t* info,
                      int connectivity, int impl, int labelling, void* scratch, size_t scratch_bytes, void* stream) {
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty()) e = ptr_error(who, in, "in", 8);
    if (e.empty()) e = ptr_error(who, out, "out", 8);
    if (e.empty() && info) e = ptr_error(who, info, "info", 8);
    if (e.empty()) e = conn_error(who, connectivity, impl);
    if (e.empty() && !scratch) e = who + "null scratch";
    if (e.empty() && scratch_bytes < morph_scratch_bytes(w, h, d)) e = who + "scratch too small (see " + sizes + ")";
    if (!e.empty()) return fail(e);
    return run_on_device_of(in, stream, [&](hipStream_t s) { launch_morph_holes(w, h, d, in, out, info, labelling, connectivity, scratch, s); });
}
int unet_morph_holes(int w, int h, int d, const uint64_t* in, uint64_t* out, int64_t* info, int impl, void* scratch, size_t scratch_bytes,
                     void* stream) {
    // this header's impls onto the labelling's: the tiled union-find in LDS, or every voxel hooked in global memory
    return holes_call("unet_morph_holes: ", "unet_morph_scratch_bytes", w, h, d, in, out, info, 6, impl,
                      impl == UNET_MORPH_IMPL_GLOBAL ? UNET_COMPONENTS_IMPL_GLOBAL : UNET_COMPONENTS_IMPL_TILED, scratch, scratch_bytes, stream);
}
int unet_morph_apply(int w, int h, int d, uint16_t* labels, const uint64_t* bits, int value, int mode, int64_t* changed, void* stream) {
    const std::string who = "unet_morph_apply: ";
    std::string e = morph_grid_error(who, w, h, d);
    if (e.empty()) e = ptr_error(who, labels, "labels", 2);
    if (e.empty()) e = ptr_error(who, bits, "bits", 8);
    if (e.empty() && (value < 1 || value > 65535)) e = who + "value must be in [1, 65535], got " + std::to_string(value);
    if (e.empty() && mode != UNET_MORPH_SET && mode != UNET_MORPH_KEEP) e = who + "unknown mode " + std::to_string(mode);
    if (e.empty() && changed) e = ptr_error(who, changed, "changed", 8);
    if (!e.empty()) return fail(e);
    return run_on_device_of(labels, stream, [&](hipStream_t s) { launch_morph_apply(w, h, d, labels, bits, value, mode, changed, s); });
}

// ---- connected components with a chosen connectivity (include/unet_connectivity.h) ----
// keep-largest, instance labelling and hole filling with a connectivity of 6, 18 or 26: each call runs the one body of its operation
// above (keep_largest_call, inst_label_call, holes_call) under its own name, as its sibling does with a connectivity of 6; the impl
// values are those of the labelling stage (DEFAULT and TILED: the tile's union-find in LDS, GLOBAL: every voxel in global memory)
int unet_conn_scratch_bytes(int64_t voxels, int n_classes, size_t* bytes) {
    const std::string e = labelling_size_error("unet_conn_scratch_bytes: ", voxels, n_classes);
    if (!e.empty()) return fail(e);
    if (!bytes) return fail("unet_conn_scratch_bytes: null bytes");
    *bytes = components_scratch_bytes(voxels, n_classes);
    return 0;
}
int unet_conn_keep_largest(int w, int h, int d, uint16_t* label, int n_classes, const uint32_t* listed, int n_listed, uint32_t* removed,
                           int connectivity, int impl, void* scratch, size_t scratch_bytes, void* stream) {
    const std::string who = "unet_conn_keep_largest: ";
    if (w <= 0 || h <= 0 || d <= 0) return fail(who + "dimensions (w, h, d) must be positive");
    std::string e = labelling_size_error(who, (int64_t)w * h * d, n_classes);
    if (e.empty() && !label) e = who + "null label";
    if (e.empty() && n_listed < 0) e = who + "n_listed must not be negative, got " + std::to_string(n_listed);
    if (e.empty() && n_listed > 0 && !listed) e = who + "null listed";
    if (e.empty()) e = conn_error(who, connectivity, impl);
    if (e.empty() && !scratch) e = who + "null scratch";
    if (e.empty() && scratch_bytes < components_scratch_bytes((int64_t)w * h * d, n_classes))
        e = who + "scratch too small (see unet_conn_scratch_bytes)";
    if (!e.empty()) return fail(e);
    return keep_largest_call(who, w, h, d, label, n_classes, listed, n_listed, removed, connectivity, impl, scratch, stream);
}
int unet_conn_label_scratch_bytes(int64_t voxels, int n_classes, int64_t max_instances, size_t* bytes) {
    return inst_scratch_query("unet_conn_label_scratch_bytes: ", voxels, n_classes, max_instances, bytes);
}
int unet_conn_label(int w, int h, int d, const uint16_t* label, int n_classes, const uint32_t* listed, int n_listed, int32_t* inst,
                    int64_t* rows, int64_t max_instances, int64_t* info, int connectivity, int impl, void* scratch, size_t scratch_bytes,
                    void* stream) {
    return inst_label_call("unet_conn_label: ", "unet_conn_label_scratch_bytes", w, h, d, label, n_classes, listed, n_listed, inst, rows,
                           max_instances, info, connectivity, impl, scratch, scratch_bytes, stream);
}
int unet_conn_holes_scratch_bytes(int w, int h, int d, size_t* bytes) {
    return morph_scratch_query("unet_conn_holes_scratch_bytes: ", w, h, d, bytes);
}
int unet_conn_holes(int w, int h, int d, const uint64_t* in, uint64_t* out, int64_t* info, int connectivity, int impl, void* scratch,
                    size_t scratch_bytes, void* stream) {
    return holes_call("unet_conn_holes: ", "unet_conn_holes_scratch_bytes", w, h, d, in, out, info, connectivity, impl,
                      impl == UNET_CONN_IMPL_GLOBAL ? UNET_COMPONENTS_IMPL_GLOBAL : UNET_COMPONENTS_IMPL_TILED, scratch, scratch_bytes, stream);
}

}  // extern "C"
