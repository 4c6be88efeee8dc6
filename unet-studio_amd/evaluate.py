"""Inference loop of the reference over the engine: `evaluate_unet::start()` -> `prepare_for_inference`, then
`evaluate_unet::evaluate()` (evaluate.cpp:386-399, 211-246) for host buffers that are either already at the model's grid or
`space.NativeVolume`s on the scan's own grid (reading files and file output are TIPL code and out of scope).

One `model_io` buffer is a float32 host array of shape (in_count*D, H, W): the input channels stacked along z
(evaluate.cpp:226-227).  After the forward it holds (out_count*D, H, W): the full-resolution logits [0] of the network, copied
back to the host (evaluate.cpp:228-229).  Errors do not propagate: like the reference's thread they set `error_msg` and `aborted`
(evaluate.cpp:234-242).

With `postproc` (a chain string, or "model" for model.postproc; postproc.py) the chain runs on the device after every forward
(evaluate.cpp:274) and each buffer is replaced by a dict of the wanted `outputs` instead: "label" uint16 (D, H, W), "fg_prob"
float32 (D, H, W), "label_prob" float32 ((out_count-1)*D, H, W).  Only those are copied back.  An empty chain returns logits.

An entry may be a `space.NativeVolume` (in_count*d, h, w) with its voxel size instead: it is uploaded, brought to model.dim on the
device (space.to_model_space: read_image_and_label, train.cpp:13-40), run through the forward, and the results come back on ITS grid,
in the reference's order, handle_fov_post then run_postproc (evaluate.cpp:274): without a chain the logits resampled linear,
(out_count*d, h, w); with one, the chain on the native grid, its fused softmax / create_mask / argmax group interpolating the
logits it reads (include/unet_space.h) and every later command unchanged.  Plain arrays take the path above unchanged.

With `preproc` / `orientation` (chain strings, or "model" for model.preproc / model.orientation; preproc.py) a NativeVolume runs the
reference's full order (evaluate.cpp:201-204, 274): run_preproc on the device on its own grid, then the model -> image map of the
preprocessed grid composed with the orientation's map (handle_orientation costs no pass in either direction), the forward, and
the way back through the inverse of preproc geometry o model -> image o orientation, so the results land on the scan's ORIGINAL
grid and orientation.  A plain array is already past the read stage: with a preproc or orientation in force it ends the run.

With `single_component` (a list of classes, or "model" for model.single_component_label, which the reference hands to every
evaluation set before the forward, evaluate.cpp:199; components.py) every listed class of the `label` output keeps its largest
connected component, after the chain and on the grid the chain ran on (the scan's own for a NativeVolume).  It acts on the label
output only: without a chain (logits) or without "label" among the outputs it changes nothing.  `single_component_connectivity` (6,
18 or 26; connectivity.py) says what joins the voxels of a component; any other value ends the run before any forward.

With `morphology` (a list of morph.run's ops: ("dilate" | "erode" | "open" | "close", value, connectivity, iterations) and
("fill_holes", classes, value[, connectivity]); morph.py) the `label` output is repaired on the device after single_component, on the grid the chain
ran on and before the atlas stage.  A bad op ends the run before any forward, like a bad chain.  Without it nothing changes.

With `fov_strategy="tiles"` (or "model" for a model whose fov_strategy says so; None and "align_top" are the path above) a volume
larger than the model's field of view is no longer cropped: it is covered by overlapping windows of model.dim whose logits are
blended (tiles.py, include/unet_tiles.h; the definitions are this project's).  A NativeVolume is preprocessed as above, resampled
ONCE, with normalize, to the canvas -- the grid at the model's voxel size that covers it -- so the normalisation is global over the
scan; each tile is an integer crop of the canvas and one forward (the filter packs are reused from the second on); the blended
canvas logits then take the way back exactly as if the model's grid were the canvas.  A plain array is its own canvas: every dim
must be at least the model's, and a chain's leading softmax / create_mask / argmax group blends the logits it reads without
storing them.  `tile_overlap` in [0, 0.5) is the fraction of a tile shared with its neighbour.  A volume that fits the model takes
today's path bit for bit.  The stack of tile logits costs tiles * out_count * tile_voxels * 4 bytes on the device (27 tiles of
6 x 128^3: 1.36 GB); the forwards run one tile at a time.

With `atlas` (a register.Atlas: atlas.prepare_atlas's products on the device) the loop ends where `--template ... --atlas ...` is
meant to (evaluate.cpp:488-496): `outputs` may also name "atlas" and "regions".  When one is wanted, for every buffer, after the chain and
single_component and on the grid the chain ran on, register.parcellate carries the atlas onto the final label (the voxel size is
the NativeVolume's, model.voxel_size for a plain array, tiled or not; `atlas_options` holds parcellate's keywords, `init` among
them) and table.regions tabulates the result, in the stream the chain ran in.  "atlas" comes back uint16 (d, h, w); "regions" as a
dict: table int64 {n_regions + 1, 10} (table.py's columns), volume_mm3 float64, report (parcellate's) and tissue_dice, float64
2 * agree / (subject foreground + sampled template foreground) from one register.joint_hist at the map found, so that a failed
registration is visible.  The label is produced for the stage whether or not it is among the wanted outputs and copied back only
when it is.  parcellate synchronises with the host twice per buffer (the map, then its reports): the copy of the previous
buffer's results still runs under the forward, but the host does not run ahead of this stage.  Without `atlas` nothing changes.
`atlas_starts` (a start.Plan; None: the search from centre_init, unchanged) lets parcellate begin from image moments and ranked
rotated starts: one more host wait per buffer, for the label's moments; the template's come from atlas.moments().
`atlas_warp` (a warp.Plan; None: the affine map alone, unchanged) lets parcellate refine its map by a lattice field before the carry
(DESIGN.md §34): no further host wait.

With `mirror_axes` (a string of the letters x, y, z; None and "" are the paths above with no extra launch) every window is run
under each combination of flips of those axes, K = 2^|axes| forwards on inputs flipped on the device, and the members' logits are
flipped back and averaged before softmax / argmax (mirror.py, include/unet_mirror.h; the definitions are this project's).  The axes
are the MODEL GRID's, i.e. after `orientation`.  `mirror_swap` = (axis letter, [(a, b), ...]), in the same frame, names the channel
pairs a model with lateralised classes exchanges under a flip of that axis (left / right hippocampus): those members' channels are
swapped back as well as their voxels.  A plain array with a chain does not store the mean logits: the chain's leading softmax /
create_mask / argmax group combines the logits it reads, and `outputs` may then also name "agreement", uint8 (D, H, W): how many
of the K members voted for the mean's top class (with it, from 4 members on, the mean is stored once: that measured faster).  A NativeVolume, a run without a chain and every tile take the mean logits
(one gather pass) and then today's path unchanged; "agreement" is refused for a NativeVolume and under tiles.  The member stack
costs K * out_count * voxels * 4 bytes on the device (8 members of 6 x 128^3: 403 MB), is reused across volumes, and the time is K
forwards per window (the filter packs are reused from the second on).

With `ensemble` (a list of further models; `self.model` is member 0) every volume is run through each member in order and the
members' softmax probabilities are averaged per voxel (ensemble.py, include/unet_ensemble.h; the definitions are this project's).
All members must share in_count, out_count, dim and voxel_size; the "model" options (postproc, preproc, orientation, fov_strategy,
single_component) are member 0's.  `ensemble_weights` (one positive number per member, member 0 first; None: equal) are normalised
to sum to 1.  Each member's logits are made exactly as the paths above make them on the grid the chain runs on -- the forward, the
mirrored members' mean with `mirror_axes`, the blended canvas under tiles, the linear resample onto a NativeVolume's grid -- and
folded into one state of (out_count + 2) * voxels * 4 bytes that is reused across volumes and does not grow with the number of
members; the chain then starts from that state (its leading softmax / create_mask / argmax group reads the mean probabilities;
softmax may not recur later), and single_component, morphology and the atlas stage follow unchanged.  `outputs` may then also name
"entropy" and "mutual_info", float32 (d, h, w), for plain arrays, NativeVolumes and tiles alike: the entropy of the mean prediction
in nats (the members disagree, or every member is unsure) and that entropy minus the members' mean entropy (the members disagree).
"entropy" without further models runs the same path with one member; "mutual_info" needs more than one; both need a chain;
"agreement" is refused with either.  The time is one forward (K with mirroring, one per tile) per member.  With `ensemble=None`
and neither output wanted nothing changes."""
import collections

import numpy as np
import torch

from . import components as CMP
from . import connectivity as CN
from . import engine as E
from . import ensemble as EN
from . import mirror as MR
from . import morph as MO
from . import postproc as P
from . import preproc as PRE
from . import register as REG
from . import space as SP
from . import table as TAB
from . import tiles as TL


# what _check hands the loop: the parsed options of one start()
_Checked = collections.namedtuple("_Checked", "steps chain_outputs staged masks swap pre ori ori_map listed cmp_conn tiled overlap ops atl "
                                             "members weights uncertainty")
# one entry past the input stage: x on the device ({1, in_count, d, h, w}; {in_count, cd, ch, cw} with a plan), the map `back` from a
# voxel of a NativeVolume's grid `native` (d, h, w) to the grid the forward runs on (None for a plain array), the tile plan and canvas
# (w, h, d) when it runs in more than one tile, and `size`, the entry's own grid (d, h, w), where its results land
_Entry = collections.namedtuple("_Entry", "x back native plan canvas size")


class _Run:
    """What one start() carries from volume to volume: the uint8 scratch buffers by stage (normalize's reduction, the chain's, the
    component labelling's, the morphology's, the region table's, the ensemble's state), per model of the ensemble the volume sizes
    whose filter packs this run has already made (the weights are frozen; the packs are the model's), and the mirrored members'
    logits, reused across windows and volumes."""

    def __init__(self, device, n_models=1):
        self.device, self.buffers, self.member_stack = device, {}, None
        self.packed_sizes = [set() for _ in range(n_models)]

    def scratch(self, stage, need):
        buf = self.buffers[stage] = E.scratch(self.buffers.get(stage), need, self.device)
        return buf


def _land(out, pending):
    """waits for the copies of one entry's results and puts them into out"""
    fi, bi, hosts, ev, extra = pending
    ev.synchronize()
    # views of the pinned buffers the copies landed in (owned by the arrays)
    res = {k: host.numpy().reshape(shape) for k, (host, shape) in hosts.items()}
    if "regions" in res:                           # the host arithmetic on the table and on the histogram at the map found
        hist = res.pop("tissue_hist").view(np.uint32)[0].astype(np.int64)
        agree = int(np.trace(hist)) - int(hist[0, 0])
        both = int(hist[1:].sum()) + int(hist[:, 1:].sum())
        res["regions"] = dict(table=res["regions"], volume_mm3=TAB.volumes_mm3(res["regions"], extra["voxel_size"]),
                              report=extra["report"], tissue_dice=np.float64(2.0 * agree / both) if both else np.float64("nan"))
    out[fi][bi] = res[None] if None in res else res


class EvaluateUNet:
    def __init__(self, model, device=None, postproc=None, outputs=("label",), params=None, preproc=None, orientation=None,
                 single_component=None, fov_strategy=None, tile_overlap=0.25, atlas=None, atlas_options=None, morphology=None,
                 single_component_connectivity=6, mirror_axes=None, mirror_swap=None, ensemble=None, ensemble_weights=None,
                 atlas_starts=None, atlas_warp=None):
        self.model = model
        self.ensemble = ensemble               # a list of further models (self.model is member 0), None: one model
        self.ensemble_weights = ensemble_weights   # one positive weight per member, member 0 first; None: equal
        self.postproc = postproc
        self.preproc = preproc                 # a chain string, "model" for model.preproc, None / "": no pre-processing
        self.orientation = orientation         # a flip / swap chain, "model" for model.orientation, None / "": none
        self.single_component = single_component   # a list of classes, "model" for model.single_component_label, None: none
        self.single_component_connectivity = single_component_connectivity   # 6, 18 or 26: what joins a component's voxels
        self.fov_strategy = fov_strategy       # None / "align_top": one window; "tiles": blended tiles; "model": model.fov_strategy
        self.tile_overlap = tile_overlap       # the fraction of a tile shared with its neighbour, in [0, 0.5)
        self.atlas = atlas                     # a register.Atlas: the outputs "atlas" and "regions" become available
        self.atlas_options = atlas_options     # register.parcellate's keywords (init, step, stages, max_iterations, ...)
        self.atlas_starts = atlas_starts       # a start.Plan: parcellate searches from ranked starts; None: centre_init
        self.atlas_warp = atlas_warp           # a warp.Plan: parcellate refines the map by a lattice field; None: affine
        self.morphology = morphology           # a list of morph.run's ops on the label output, None / []: none
        self.mirror_axes = mirror_axes         # letters of the model grid's axes to mirror over, None / "": no mirroring
        self.mirror_swap = mirror_swap         # (axis letter, [(a, b), ...]): channel pairs exchanged under a flip of that axis
        self.params = params                   # the chain's parameters (postproc.parse_chain; postproc.txt in the reference GUI)
        self.outputs = tuple(outputs)
        self.device = torch.device(device) if device is not None else model.device()
        self.error_msg = ""
        self.aborted = False
        self.running = False
        self.cur_prog = 0
        self.status = ""

    def start(self, model_io):
        """model_io: list (one entry per input file) of lists of host buffers (evaluate.hpp:18: eval[i].model_io).
        Returns the same structure with every buffer replaced by its (out_count*D, H, W) result."""
        self.status = "initiating"
        self.model.prepare_for_inference(self.device)     # evaluate.cpp:391
        self.aborted, self.running, self.error_msg, self.cur_prog = False, True, "", 0
        out = [list(ios) for ios in model_io]
        pending = None      # (file index, buffer index, {name: (pinned host tensor, shape)}, event, extra): the previous result, in flight
        copy_stream = torch.cuda.Stream(self.device)
        try:
            try:                                           # a bad option ends the run as run_postproc's failure does (evaluate.cpp:274)
                cfg = self._check(out)
            except E.UNetError as e:
                self.error_msg, self.aborted, self.running = str(e), True, False
                return out
            for member in cfg.members[1:]:                 # each member once; member 0 above
                member.prepare_for_inference(self.device)
            run = _Run(self.device, len(cfg.members))
            with torch.no_grad():                          # evaluate.cpp:221
                while self.cur_prog < len(out) and not self.aborted:
                    self.status = "inferencing"
                    for i, io in enumerate(out[self.cur_prog]):
                        entry = self._input(cfg, run, io)
                        state = result = stack = members = size = None
                        if cfg.weights is not None:                # every member's probabilities folded into one state
                            state = self._ensemble_state(cfg, run, entry)
                        else:
                            result, stack, members, size = self._forward(cfg, run, entry.x, entry.plan,
                                                                         fused=entry.native is None and cfg.steps is not None)
                        extra = {}
                        if cfg.steps is not None:
                            results = self._chain(cfg, run, entry, result, stack, members, size, state)
                            if cfg.atl is not None and cfg.staged:
                                extra = self._atlas_stage(cfg, run, io, entry, results)
                            h, w = entry.size[1:]
                            results = {k: (v, (v.numel() // (h * w), h, w) if k in EN.OUTPUTS or k in ("atlas", "agreement") else tuple(v.shape))
                                       for k, v in results.items() if k in self.outputs or k == "tissue_hist"}
                        else:
                            if entry.native is not None:                                 # handle_fov_post alone: the logits on the native grid
                                result = SP.resample(result.view(self.model.out_count, *size), entry.native, entry.back, "linear")
                            results = {None: (result, (self.model.out_count * entry.size[0],) + entry.size[1:])}
                        landing = self._copy_back(results, copy_stream)
                        if pending is not None:
                            _land(out, pending)
                        pending = (self.cur_prog, i) + landing + (extra,)
                    self.cur_prog += 1
                if pending is not None:
                    _land(out, pending)
        except Exception as e:                                                           # evaluate.cpp:234-242
            self.error_msg = "error during evaluation:" + str(e)
            self.aborted = True
        self.running = False
        return out

    def _check(self, out):
        """Everything that ends the run before the first upload, in this order; raises UNetError.  Returns what the loop needs."""
        m = self.model
        chain = m.postproc if self.postproc == "model" else self.postproc
        staged = tuple(o for o in self.outputs if o in ("atlas", "regions"))              # the atlas stage's outputs
        want_agr = "agreement" in self.outputs                                            # the mirror stage's output
        uncertainty = tuple(o for o in self.outputs if o in EN.UNCERTAINTY)               # the ensemble's outputs
        chain_outputs = tuple(o for o in self.outputs if o not in staged and o != "agreement" and o not in uncertainty)
        members, weights = self._check_ensemble(chain, uncertainty, want_agr)
        masks = MR.parse_axes(self.mirror_axes)
        mirrored = len(masks) > 1
        swap = None
        if self.mirror_swap is not None:
            if not mirrored:
                raise E.UNetError("mirror_swap needs mirror_axes")
            swap = MR._swap(self.mirror_swap, m.out_count, masks)
            swap = ("xyz"[swap[0]], swap[1]) if swap[0] >= 0 else None
        if want_agr and not mirrored:
            raise E.UNetError("output agreement needs mirror_axes")
        if want_agr and not chain:
            raise E.UNetError("output agreement needs a postproc chain")
        atl = self.atlas
        if atl is not None and "label" not in chain_outputs:
            chain_outputs += ("label",)                    # the stage reads it; it is copied back only when wanted
        if staged and atl is None:
            raise E.UNetError("output %s needs an atlas" % staged[0])
        if atl is not None and not chain:
            raise E.UNetError("an atlas needs a postproc chain that produces a label")
        steps = None
        if chain:
            steps = P.parse_chain(chain, self.params)
            P.check_chain(steps)
            P.check_outputs(steps, chain_outputs)
            if weights is not None:
                P.check_ensemble_chain(steps)
            if atl is not None and not isinstance(atl, REG.Atlas):
                raise E.UNetError("atlas must be a register.Atlas")
        # run_preproc / handle_orientation's failure (evaluate.cpp:201-204)
        pre = PRE.active(PRE.parse_chain(m.preproc if self.preproc == "model" else self.preproc))
        ori = PRE.parse_orientation(m.orientation if self.orientation == "model" else self.orientation)
        ori_map = PRE.orientation_map(ori, m.dim, m.voxel_size) if ori else (None, None, None)
        listed = CMP.resolve(self.single_component, m)
        cmp_conn = CN.check(self.single_component_connectivity, "single_component")
        fov = m.fov_strategy if self.fov_strategy == "model" else self.fov_strategy
        if fov not in (None, "", "align_top", "tiles"):
            raise E.UNetError("unknown fov_strategy %s" % (fov,))
        tiled = fov == "tiles"
        if tiled and want_agr:
            raise E.UNetError("output agreement is not available with fov_strategy tiles")
        if want_agr and any(isinstance(io, SP.NativeVolume) for ios in out for io in ios):
            raise E.UNetError("output agreement is not available for a NativeVolume")
        overlap = TL.check_overlap(self.tile_overlap) if tiled else 0.0
        ops = MO.check_ops(self.morphology, m.out_count) if self.morphology else []
        if steps is None or "label" not in chain_outputs:  # both act on the label output only
            listed, ops = [], []
        return _Checked(steps, chain_outputs, staged, masks, swap, pre, ori, ori_map, listed, cmp_conn, tiled, overlap, ops, atl,
                        members, weights, uncertainty)

    def _check_ensemble(self, chain, uncertainty, want_agr):
        """The ensemble's options: ([member 0, further models ...], the normalised weights).  The weights are None when this run
        takes the one-model paths: no further model and neither entropy nor mutual_info wanted."""
        m = self.model
        further = self.ensemble if self.ensemble is not None else []
        if not isinstance(further, (list, tuple)):
            raise E.UNetError("ensemble must be a list of further models, got %r" % (further,))
        members = [m] + list(further)
        for k, other in enumerate(members[1:], 1):
            for what in ("in_count", "out_count", "dim", "voxel_size"):
                if not hasattr(other, what):
                    raise E.UNetError("ensemble: member %d is not a model (it has no %s)" % (k, what))
                a, b = getattr(other, what), getattr(m, what)
                a, b = (tuple(a), tuple(b)) if what in ("dim", "voxel_size") else (a, b)
                if a != b:
                    raise E.UNetError("ensemble: member %d has %s %s, member 0 has %s" % (k, what, a, b))
        if len(members) == 1 and not uncertainty:
            if self.ensemble_weights is not None:
                raise E.UNetError("ensemble_weights needs ensemble")
            return members, None
        weights = EN.normalize_weights(self.ensemble_weights, len(members))
        if "mutual_info" in uncertainty and len(members) == 1:
            raise E.UNetError("output mutual_info needs more than one member (ensemble)")
        if want_agr:
            raise E.UNetError("output agreement is not available with ensemble (it counts one model's mirrored views)")
        if not chain:
            raise E.UNetError("%s needs a postproc chain" % ("output " + uncertainty[0] if uncertainty else "ensemble"))
        return members, weights

    def _input(self, cfg, run, io):
        """one entry of model_io -> _Entry: the input on the device, the way back and the grids"""
        m = self.model
        model_dim = mW, mH, mD = tuple(int(v) for v in m.dim)
        nv = io if isinstance(io, SP.NativeVolume) else None
        if nv is not None:
            nv.check()
            io = nv.data
        elif cfg.pre or cfg.ori:
            raise E.UNetError("a plain model_io array is already at the model's grid: preproc / orientation need a "
                              "NativeVolume")
        io = np.ascontiguousarray(io, dtype=np.float32)
        if io.ndim != 3 or io.shape[0] % m.in_count:
            raise E.UNetError("model_io buffer must be (in_count*D, H, W), got %s" % (io.shape,))
        size = (io.shape[0] // m.in_count, io.shape[1], io.shape[2])
        plan = canvas = None                                                 # set when this entry runs in more than one tile
        if cfg.tiled and nv is None:                                         # the array is its own canvas
            canvas = size[::-1]
            if canvas[0] < mW or canvas[1] < mH or canvas[2] < mD:
                raise E.UNetError("fov_strategy tiles: a model_io array (w, h, d) = %s is smaller than the model's %s"
                                  % (canvas, model_dim))
        elif cfg.tiled:                                                      # the grid at the model's voxel size that covers the scan
            if nv.map is not None:
                raise E.UNetError("a caller's map and tiles do not combine")
            pdims, pvs, G = PRE.geometry(cfg.pre, size[::-1], nv.voxel_size)
            canvas = TL.canvas_dims(m.dim, m.voxel_size, pdims, pvs, orientation=cfg.ori)
        if cfg.tiled and canvas != model_dim:                                # a volume that fits takes the paths below
            plan = TL.plan_tiles(canvas, model_dim, cfg.overlap)
        if plan is not None and nv is None:
            x = torch.from_numpy(io).view(m.in_count, *size).to(self.device)
            return _Entry(x, None, None, plan, canvas, size)
        if nv is None:
            x = torch.from_numpy(io).view(1, m.in_count, *size).to(self.device)
            return _Entry(x, None, None, plan, canvas, size)
        if plan is not None:                                                 # run_preproc, then ONE resample to the canvas
            x = self._preprocessed(cfg, run, io, size, pdims)
            cD0, cvs0, cM = PRE.orientation_map(cfg.ori, canvas, m.voxel_size) if cfg.ori else (canvas, m.voxel_size, None)
            fwd = SP.model_to_image_map(cD0, cvs0, pdims, pvs)               # canvas voxel -> preprocessed-grid position
            if cfg.ori:
                fwd = SP.compose_map(fwd, cM)
            back = SP.invert_map(SP.compose_map(G, fwd))                     # original native voxel -> canvas position
            x = SP.resample(x, canvas[::-1], fwd, "linear", normalize=True)  # one normalisation over the whole scan
            return _Entry(x, back, size, plan, canvas, size)
        if cfg.pre or cfg.ori:
            D0, vs0, M = cfg.ori_map
            pdims, pvs, G = PRE.geometry(cfg.pre, size[::-1], nv.voxel_size)
            x = self._preprocessed(cfg, run, io, size, pdims)
            if nv.map is not None:
                fwd = nv.map
            else:
                fwd = SP.model_to_image_map(D0 or m.dim, vs0 or m.voxel_size, pdims, pvs)
            if cfg.ori:
                fwd = SP.compose_map(fwd, M)                                 # model voxel -> preprocessed-grid position
            back = SP.invert_map(SP.compose_map(G, fwd))                     # original native voxel -> model position
            x = SP.to_model_space(m, x, pvs, map=fwd)[0].unsqueeze(0)
        else:                                                                # read_image_and_label, on the compute stream
            fwd = nv.map if nv.map is not None else SP.model_to_image_map(m.dim, m.voxel_size, size[::-1], nv.voxel_size)
            back = SP.invert_map(fwd)                                        # native voxel -> model position
            x = torch.from_numpy(io).view(m.in_count, *size).to(self.device)
            x = SP.to_model_space(m, x, nv.voxel_size, map=fwd)[0].unsqueeze(0)
        return _Entry(x, back, size, plan, canvas, size)

    def _preprocessed(self, cfg, run, io, size, pdims):
        """the upload of a NativeVolume's data, then run_preproc on its own grid, on the compute stream (evaluate.cpp:201-204)"""
        x = torch.from_numpy(io).view(self.model.in_count, *size).to(self.device)
        scratch = None
        if PRE.needs_scratch(cfg.pre):                     # normalize's reduction scratch
            scratch = run.scratch("preproc", PRE.preproc_scratch_bytes(self.model.in_count * pdims[0] * pdims[1] * pdims[2]))
        return PRE.run_preproc(x, cfg.pre, scratch=scratch)

    def _forward_mirrored(self, cfg, run, x1, k=0):
        """x1 {1, in_count, d, h, w} on the device -> the stack {K, out_count, d, h, w} of the mirrored members' level-0 logits
        from model k of the ensemble"""
        m = cfg.members[k]
        need = MR.stack_bytes(cfg.masks, m.out_count, x1[0, 0].numel()) // 4
        if run.member_stack is None or run.member_stack.numel() < need:
            run.member_stack = torch.empty(need, dtype=torch.float32, device=self.device)
        return MR.forward_members(m, x1[0], cfg.masks, run.packed_sizes[k], out=run.member_stack)

    def _forward_tiles(self, cfg, run, xc, plan, k=0):
        """xc {in_count, cd, ch, cw} on the device -> the stack {tiles, out_count, D, H, W} of level-0 logits, one forward
        of model k of the ensemble per integer crop in tile-index order"""
        m = cfg.members[k]
        mW, mH, mD = (int(v) for v in m.dim)
        origins = TL.tile_origins(plan)
        stack = torch.empty((len(origins), m.out_count, mD, mH, mW), dtype=torch.float32, device=self.device)
        for t, (ox, oy, oz) in enumerate(origins):
            crop = xc[:, oz:oz + mD, oy:oy + mH, ox:ox + mW].contiguous().unsqueeze(0)
            size = tuple(crop.shape[2:])
            if len(cfg.masks) > 1:                         # the members' mean, straight into the tile's slot
                MR.combine(self._forward_mirrored(cfg, run, crop, k), cfg.masks, cfg.swap, out={"mean": stack[t]})
                continue
            stack[t].copy_(m.forward(crop, packs_current=size in run.packed_sizes[k])[0].view(m.out_count, mD, mH, mW))
            run.packed_sizes[k].add(size)
        return stack

    def _forward(self, cfg, run, x, plan, fused, k=0):
        """The input on the device -> (result, stack, members, size): model k's logits on the grid `size` the forward ran on, or,
        when the chain's leading group reads them itself (fused), the tile stack or the mirrored members' stack in their place."""
        size = tuple(x.shape[-3:])
        result = stack = members = None
        if plan is not None:                               # one forward per tile (evaluate.cpp:223-230)
            stack = self._forward_tiles(cfg, run, x, plan, k)
            if not fused:                                  # the canvas logits, as if the model's grid were the canvas
                result, stack = TL.blend(stack, plan, size), None
        elif len(cfg.masks) > 1:                           # one forward per member
            members = self._forward_mirrored(cfg, run, x, k)
            if not fused:                                  # the mean logits, then today's path
                result, members = MR.combine(members, cfg.masks, cfg.swap)[0], None
        else:
            result = cfg.members[k].forward(x, packs_current=size in run.packed_sizes[k])[0]     # evaluate.cpp:226-227
            run.packed_sizes[k].add(size)
        return result, stack, members, size

    def _ensemble_state(self, cfg, run, entry):
        """Every member's logits, made as the one-model paths make them on the grid the chain runs on (the forward, the mirrored
        members' mean, the blended canvas, the linear resample onto a NativeVolume's grid), folded in member order into the run's
        one state, which is returned"""
        out_c = self.model.out_count
        d, h, w = entry.size
        state = run.scratch("ensemble", EN.state_bytes(out_c, d * h * w))
        for k, weight in enumerate(cfg.weights):
            logits, _, _, size = self._forward(cfg, run, entry.x, entry.plan, fused=False, k=k)
            logits = logits.view(out_c, *size)
            if entry.native is not None:                                                 # handle_fov_post: onto the scan's grid
                logits = SP.resample(logits, entry.native, entry.back, "linear")
            EN.accumulate(logits, state, weight, k == 0)
        return state

    def _chain(self, cfg, run, entry, result, stack, members, size, state=None):
        """run_postproc on the grid the results come back on (evaluate.cpp:274), on the compute stream: {output: device tensor}.
        state: the ensemble's, already on that grid, in place of everything a one-model run reads"""
        m = self.model
        d, h, w = entry.size
        voxels = d * h * w if entry.native is not None or entry.plan is not None or result is None else result.numel() // m.out_count
        want_agr = "agreement" in self.outputs
        return P.run_postproc(
            result if stack is None else None, cfg.steps,
            outputs=cfg.chain_outputs + (("agreement",) if want_agr else ()) + (cfg.uncertainty if state is not None else ()),
            scratch=run.scratch("chain", P.postproc_scratch_bytes(m.out_count, voxels)) if P.needs_scratch(cfg.steps) else None,
            mirror=None if members is None else (members, cfg.masks, cfg.swap),
            native=None if entry.native is None or state is not None else (entry.back, entry.native),
            tiles=None if stack is None else (stack, entry.plan, size),
            ensemble=None if state is None else (state, m.out_count, entry.size),
            single_component=cfg.listed or None, single_component_connectivity=cfg.cmp_conn,
            component_scratch=run.scratch("components", CMP.components_scratch_bytes(voxels, m.out_count)) if cfg.listed else None,
            morphology=cfg.ops or None,
            morphology_scratch=run.scratch("morphology", MO.morph_scratch_bytes(entry.size)) if cfg.ops else None)

    def _atlas_stage(self, cfg, run, io, entry, results):
        """register.parcellate on the final label and table.regions on its result, on the compute stream: adds "atlas", "regions" and
        "tissue_hist" to results and returns what the host arithmetic on them needs"""
        atl = cfg.atl
        label = results["label"].view(entry.size)
        vs = io.voxel_size if isinstance(io, SP.NativeVolume) else self.model.voxel_size
        opts = dict(self.atlas_options or {})
        if self.atlas_starts is not None:
            opts.update(starts=self.atlas_starts, template_moments=atl.moments())
        if self.atlas_warp is not None:
            opts.update(warp=self.atlas_warp)
        parc, report = REG.parcellate(label, vs, atl.template, atl.template_vs, atl.regions, atl.n_tissues, **opts)
        if "atlas" in cfg.staged:
            results["atlas"] = parc
        if "regions" not in cfg.staged:
            return {}
        scratch = run.scratch("table", TAB.table_scratch_bytes(label.numel(), atl.n_regions))
        results["regions"] = TAB.regions(parc, atl.n_regions, scratch=scratch)
        results["tissue_hist"] = REG.joint_hist(label, atl.template, atl.n_tissues, [np.concatenate(report["map"])]).view(torch.int32)
        return dict(report=report, voxel_size=tuple(float(v) for v in vs))

    def _copy_back(self, results, copy_stream):
        """evaluate.cpp:228-229 copies the logits to the host before the next forward starts; here the copy runs on its own stream
        into pinned memory under the next buffer's upload + forward (same bytes, same order of results).  Returns
        ({name: (pinned host tensor, shape)}, the event after the copies)."""
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        # (pinning costs ~2.6 ms per 50 MB result whether it is done per volume or in one arena for the whole run:
        # measured 4.5 vs 7.1 ms per volume, profiles/bench_evaluate.py)
        hosts = {}
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(done)
            for k, (r, shape) in results.items():
                host = torch.empty(r.shape, dtype=r.dtype, pin_memory=True)
                host.copy_(r, non_blocking=True)
                r.record_stream(copy_stream)
                hosts[k] = (host, shape)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        return hosts, ev
