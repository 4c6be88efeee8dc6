"""The inference post-processing chain of the reference (postproc, unet.cpp:112; evaluate.cpp:274,303-376) on the device.

A chain is commands separated by '+', run left to right (the model's default: "softmax+create_mask+argmax").  The definitions are in
include/unet_postproc.h; they are this project's, and parity with TIPL's run_postproc / softmax / argmax / defragment_by_size_ratio
/ normalize is not pinned.  Out of scope (TIPL): soft_max, anisotropic_smoothing, defragment_smoothing.  The
pre-processing and orientation handling around the chain are preproc.py's, the FOV handling space.py's.

A result holds up to three outputs: `label_prob` {C-1, D, H, W} fp32 (softmax), `fg_prob` {D, H, W} fp32 (create_mask) and `label`
{D, H, W} uint16 (argmax).  create_mask and argmax need a softmax earlier in the chain; defragment needs a create_mask before it.
argmax reads the current state: right after the fused pass that is the logits' probabilities, after a command that changed
label_prob or fg_prob (defragment, defragment_each, a per-plane command) it is label_prob and fg_prob as they now are, so such an
argmax needs a create_mask before it.  create_mask always sums the exponentials of the logits, so it may not follow such a command.
The per-plane commands and defragment_each act on label_prob.  A wanted output the chain does not produce is refused.
Adjacent softmax / create_mask / argmax run as one fused kernel, and an output nobody asked for and no later command reads is
never written (the default chain with outputs=("label",) reads the logits once and writes 2 bytes per voxel).
run_postproc(morphology=...) repairs the `label` output afterwards (morph.py: dilate / erode / open / close / fill_holes)."""
import collections
import ctypes as C

import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_postproc_scratch_bytes", C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_postproc_softmax", C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
E._sig("unet_postproc_argmax_planes", C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p)
E._sig("unet_postproc_defragment", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_postproc_plane_op", C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
       C.c_void_p)
# every symbol include/unet_postproc.h declares
EXPORTS = ["unet_postproc_scratch_bytes", "unet_postproc_softmax", "unet_postproc_argmax_planes", "unet_postproc_defragment",
           "unet_postproc_plane_op"]

# the ops of unet_postproc_plane_op (include/unet_postproc.h)
PP_UPPER_THRESHOLD, PP_LOWER_THRESHOLD, PP_MINUS, PP_BINARIZE, PP_NORMALIZE, PP_SMOOTH = 1, 2, 3, 4, 5, 6
PLANE_OPS = {"upper_threshold": PP_UPPER_THRESHOLD, "lower_threshold": PP_LOWER_THRESHOLD, "minus": PP_MINUS,
             "binarize": PP_BINARIZE, "normalize_each": PP_NORMALIZE, "gaussian_smoothing": PP_SMOOTH}

# command -> its parameters and their defaults, in order
COMMANDS = {
    "softmax": (),
    "create_mask": (),
    "argmax": (("threshold", 0.5),),
    "defragment": (("threshold", 0.5), ("size_ratio", 0.05)),
    "defragment_each": (("threshold", 0.5), ("size_ratio", 0.05)),
    "upper_threshold": (("t", 1.0),),
    "lower_threshold": (("t", 0.0),),
    "minus": (("v", 0.5),),
    "binarize": (("t", 0.5),),
    "normalize_each": (),
    "gaussian_smoothing": (),
}
OUTPUTS = ("label_prob", "fg_prob", "label")
MUTATORS = ("defragment", "defragment_each") + tuple(PLANE_OPS)   # commands that change label_prob / fg_prob / label in place
PRODUCER = {"label_prob": "softmax", "fg_prob": "create_mask", "label": "argmax"}
MIRROR_PAIR_FROM = 4   # run_postproc(mirror=) with agreement wanted: members from which combine + softmax replaces the fused pass


def parse_chain(text, params=None):
    """'softmax+create_mask+argmax' -> [(command, {parameter: value}), ...].  Host only.
    params: {command: value, a tuple of values in the order of COMMANDS, or a {parameter: value} dict}, applied to every use of
    that command (postproc.txt's role in the reference GUI).  Raises UNetError("unknown command <name>") (evaluate.cpp:375)."""
    params = dict(params or {})
    steps = []
    for name in (s.strip() for s in (text or "").split("+")):
        if not name:
            continue
        if name not in COMMANDS:
            raise UNetError("unknown command " + name)
        steps.append((name, {k: float(v) for k, v in COMMANDS[name]}))
    for name, p in params.items():
        if name not in COMMANDS:
            raise UNetError("unknown command " + name)
        spec = COMMANDS[name]
        if isinstance(p, dict):
            vals = dict(p)
        else:
            seq = p if isinstance(p, (tuple, list)) else (p,)
            if len(seq) > len(spec):
                raise UNetError("%s takes %d parameter(s), got %d" % (name, len(spec), len(seq)))
            vals = {spec[i][0]: v for i, v in enumerate(seq)}
        for k, v in vals.items():
            if k not in dict(spec):
                raise UNetError("%s has no parameter %s" % (name, k))
            for step_name, sp in steps:
                if step_name == name:
                    sp[k] = float(v)
    return steps


def check_chain(steps):
    """The order rules of this project's definitions (module docstring); raises UNetError.  Host only."""
    seen, changed = set(), None
    for name, _ in steps:
        if name in ("create_mask", "argmax", "defragment_each") or name in PLANE_OPS:
            if "softmax" not in seen:
                raise UNetError("%s needs softmax before it" % name)
        if name == "defragment" and "create_mask" not in seen:
            raise UNetError("defragment needs create_mask before it")
        if name == "create_mask" and changed:
            raise UNetError("create_mask after %s is not supported (create_mask sums the exponentials of the logits)" % changed)
        if name == "argmax" and changed and "create_mask" not in seen:
            raise UNetError("argmax after %s needs create_mask before it" % changed)
        if name in MUTATORS:
            changed = name
        seen.add(name)


def check_outputs(steps, outputs):
    """every wanted output must be one the chain produces; raises UNetError.  Host only."""
    names = [n for n, _ in steps]
    for o in outputs:
        if o not in OUTPUTS:
            raise UNetError("unknown output %s (one of %s)" % (o, ", ".join(OUTPUTS)))
        if PRODUCER[o] not in names:
            raise UNetError("output %s is not produced by the chain (it needs %s)" % (o, PRODUCER[o]))


def argmax_after_change(steps):
    """True when some argmax of the chain follows a command that changed the state (it then reads label_prob and fg_prob)"""
    changed = False
    for name, _ in steps:
        changed = changed or name in MUTATORS
        if name == "argmax" and changed:
            return True
    return False


def needs_scratch(steps):
    return any(n in MUTATORS for n, _ in steps)


def postproc_scratch_bytes(out_c, voxels):
    return E.size_query(E.lib.unet_postproc_scratch_bytes, int(out_c), int(voxels))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def softmax_call(logits, out_c, voxels, threshold=0.5, label_prob=None, fg_prob=None, label=None, stream=None):
    """unet_postproc_softmax on device pointers / tensors (None: not wanted); stream: the current one when None"""
    st = E.stream(logits, stream)
    E.check(E.lib.unet_postproc_softmax(_ptr(logits), int(out_c), int(voxels), float(threshold), _ptr(label_prob), _ptr(fg_prob),
                                        _ptr(label), st))


def argmax_planes_call(label_prob, n_planes, voxels, fg_prob, threshold, label, stream=None):
    """unet_postproc_argmax_planes"""
    st = E.stream(label_prob, stream)
    E.check(E.lib.unet_postproc_argmax_planes(_ptr(label_prob), int(n_planes), int(voxels), _ptr(fg_prob), float(threshold), _ptr(label),
                                              st))


def defragment_call(dims, each, threshold, size_ratio, fg_prob, label_prob, n_planes, label, scratch, stream=None):
    """unet_postproc_defragment; dims = (W, H, D)"""
    any_t = label_prob if each else fg_prob
    dev = any_t.device if any_t is not None else torch.device("cuda", torch.cuda.current_device())
    st = E.stream(dev, stream)
    E.check(E.lib.unet_postproc_defragment(int(dims[0]), int(dims[1]), int(dims[2]), int(bool(each)), float(threshold), float(size_ratio),
                                           _ptr(fg_prob), _ptr(label_prob), int(n_planes), _ptr(label), _ptr(scratch),
                                           scratch.nbytes if scratch is not None else 0, st))


def plane_op_call(op, param, dims, label_prob, n_planes, scratch, stream=None):
    """unet_postproc_plane_op; dims = (W, H, D)"""
    dev = label_prob.device if label_prob is not None else torch.device("cuda", torch.cuda.current_device())
    st = E.stream(dev, stream)
    E.check(E.lib.unet_postproc_plane_op(int(op), float(param), int(dims[0]), int(dims[1]), int(dims[2]), _ptr(label_prob), int(n_planes),
                                         _ptr(scratch), scratch.nbytes if scratch is not None else 0, st))


# where one volume's logits come from: head(thr, wanted) is the fused pass that reads a stack without storing logits (it returns the
# outputs it made beyond `wanted`), logits() the materialised logits, made once; agreement() the mirror's vote map on its own
Source = collections.namedtuple("Source", "out_c shape device head logits agreement")


def _tensor_source(logits):
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous()):
        raise UNetError("run_postproc: logits must be a contiguous float32 device tensor")
    if logits.dim() == 5:
        if logits.shape[0] != 1:
            raise UNetError("run_postproc: one volume at a time, got a batch of %d" % logits.shape[0])
        logits = logits[0]
    if logits.dim() != 4:
        raise UNetError("run_postproc: logits must be {C, D, H, W}, got %s" % (tuple(logits.shape),))
    out_c, D, H, W = (int(v) for v in logits.shape)
    return Source(out_c, (D, H, W), logits.device, None, lambda: logits, None)


def _tile_source(tiles, logits, native):
    from . import space as SP
    from . import tiles as TL
    if logits is not None or native is not None:
        raise UNetError("run_postproc: tiles come in place of logits and do not combine with native")
    stack, plan, canvas_shape = tiles
    canvas_shape = SP._shape3(canvas_shape, "canvas shape")
    out_c = TL._stack(stack, TL._plan_struct(plan))[0]
    blended = None

    def canvas_logits():
        nonlocal blended
        if blended is None:
            blended = TL.blend(stack, plan, canvas_shape)
        return blended

    def head(thr, wanted):
        TL.postproc_tiles(stack, plan, canvas_shape, thr, tuple(wanted), out=wanted)
        return {}
    return Source(out_c, canvas_shape, stack.device, head, canvas_logits, None)


def _mirror_source(mirror, logits, native, want_agr):
    from . import mirror as MR
    if logits is not None or native is not None:
        raise UNetError("run_postproc: mirror comes in place of logits and does not combine with tiles or native")
    stack, masks, swap = mirror
    masks = MR._masks(masks)
    out_c, D, H, W = MR._stack(stack, masks)
    MR._swap(swap, out_c, masks)                       # a bad swap is refused before any device work
    mean = None

    def mean_logits():
        nonlocal mean
        if mean is None:
            mean = MR.combine(stack, masks, swap)[0]
        return mean

    def head(thr, wanted):
        nonlocal mean
        if want_agr and len(masks) >= MIRROR_PAIR_FROM:
            # the fused pass with the K + 1 running amax beside the softmax state runs at 2 waves per SIMD: from 4
            # members on, combine (where the agreement is free) + softmax measured faster, same bits
            mean, agr = MR.combine(stack, masks, swap, True, True)
            softmax_call(mean, out_c, D * H * W, thr, wanted.get("label_prob"), wanted.get("fg_prob"), wanted.get("label"))
            return {"agreement": agr}
        # otherwise the same pass counts the votes
        extra = {"agreement": torch.empty((D, H, W), dtype=torch.uint8, device=stack.device)} if want_agr else {}
        MR.postproc_mirror(stack, masks, swap, thr, tuple(wanted) + tuple(extra), out={**wanted, **extra})
        return extra
    return Source(out_c, (D, H, W), stack.device, head, mean_logits,
                  lambda: MR.combine(stack, masks, swap, want_mean=False, want_agreement=True)[1])


def check_ensemble_chain(steps):
    """An accumulated ensemble has probabilities, no logits: only the softmax / create_mask / argmax group that starts the chain
    may read it; raises UNetError.  Host only."""
    group = ("softmax", "create_mask", "argmax")
    if not steps or steps[0][0] not in group:
        raise UNetError("with ensemble the chain must start with its softmax / create_mask / argmax group")
    j = 0
    while j < len(steps) and steps[j][0] in group:
        j += 1
    if any(n == "softmax" for n, _ in steps[j:]):
        raise UNetError("with ensemble softmax may not recur after %s (an accumulated ensemble has no logits)" % steps[j][0])


def _ensemble_source(ensemble, logits, native, tiles, mirror, steps, uncertainty):
    from . import ensemble as EN
    from . import space as SP
    if logits is not None or native is not None or tiles is not None or mirror is not None:
        raise UNetError("run_postproc: ensemble comes in place of logits and does not combine with native, tiles or mirror "
                        "(apply those per member before accumulating)")
    try:
        state, out_c, shape = ensemble
    except (TypeError, ValueError):
        raise UNetError("run_postproc: ensemble must be (state, out_c, (d, h, w)), got %r" % (ensemble,))
    out_c = int(out_c)
    D, H, W = SP._shape3(shape, "ensemble shape")
    check_ensemble_chain(steps)
    EN._state(state, out_c, D * H * W)

    def no_logits():
        raise UNetError("run_postproc: an accumulated ensemble has no logits")

    def head(thr, wanted):
        extra = {o: torch.empty((D, H, W), dtype=torch.float32, device=state.device) for o in uncertainty}
        EN.finalize(state, out_c, (D, H, W), thr, tuple(wanted) + tuple(extra), out={**wanted, **extra})
        return extra
    return Source(out_c, (D, H, W), state.device, head, no_logits, None)


def run_postproc(logits, chain, params=None, outputs=OUTPUTS, scratch=None, native=None, single_component=None,
                 component_scratch=None, tiles=None, morphology=None, morphology_scratch=None, single_component_connectivity=6,
                 mirror=None, ensemble=None):
    """Runs the chain on one volume's logits ({1, C, D, H, W} or {C, D, H, W}, contiguous fp32 device tensor) on the current stream.
    chain: a string (parse_chain) or parsed steps.  Returns {output: device tensor} for the wanted outputs the chain produces.
    scratch: a uint8 device tensor of at least postproc_scratch_bytes(C, D*H*W) bytes to reuse (one is made when needed).
    native: (map, (d, h, w)) runs the chain on that grid instead, map taking a native voxel to its position in the logits' grid
    (handle_fov_post before run_postproc, evaluate.cpp:274): every fused softmax / create_mask / argmax group interpolates the logits
    it reads (space.postproc_native), the other commands run unchanged on the native planes, and the scratch is the native grid's.
    check_chain lets no command read the logits outside a fused group, so they are never stored on the native grid.
    single_component: a list of classes (a model's single_component_label, components.py): after the chain every listed class of
    the `label` output keeps its largest connected component, on the grid the chain ran on; fg_prob and label_prob are not
    touched.  single_component_connectivity: 6, 18 or 26, what joins the voxels of a component (connectivity.py).  None or an empty list, or a chain whose wanted outputs hold no label, make no extra call.  component_scratch: a
    uint8 device tensor of components.components_scratch_bytes(voxels, C) bytes to reuse.
    tiles: (stack, plan, (D, H, W)) in place of logits (pass None): the volume is the blend of a stack of tile logits (tiles.py,
    include/unet_tiles.h).  A fused group that starts the chain blends the logits it reads and never stores them
    (tiles.postproc_tiles); a later group reads the blended canvas logits, made once when first needed.  Not with native.
    morphology: a list of morph.run's ops, run in place on the `label` output after single_component, on the grid the chain ran on;
    fg_prob and label_prob are not touched.  None or an empty list, or a chain whose wanted outputs hold no label, make no extra
    call.  morphology_scratch: a uint8 device tensor of morph.morph_scratch_bytes((D, H, W)) bytes to reuse.
    mirror: (stack, masks, swap) in place of logits (pass None): the volume's logits are the combine of a stack of mirrored members'
    logits (mirror.py, include/unet_mirror.h).  A fused group that starts the chain combines the logits it reads and never stores
    them (mirror.postproc_mirror), except when agreement is wanted from MIRROR_PAIR_FROM members on, where the stored mean measured
    faster; a later group reads the mean logits, made once when first needed.  Not with tiles or native.
    Only with mirror may `outputs` name "agreement", the uint8 {D, H, W} map of how many members voted for the mean's top class.
    ensemble: (state, out_c, (D, H, W)) in place of logits (pass None): the volume is an accumulated ensemble of several models'
    probabilities (ensemble.py, include/unet_ensemble.h).  The chain must start with its softmax / create_mask / argmax group, which
    is ensemble.finalize into the wanted planes; an accumulated ensemble has no logits, so softmax may not recur after a command
    that changed the state (a later lone argmax reads the current planes as ever).  Not with native, tiles or mirror: the caller
    applies those per member before accumulating.  Only with ensemble may `outputs` name "entropy" and "mutual_info", float32
    {D, H, W}; "agreement" is refused with it."""
    steps = parse_chain(chain, params) if isinstance(chain, str) else list(chain)
    check_chain(steps)
    outputs = tuple(outputs)
    want_agr = "agreement" in outputs                  # not a chain output (OUTPUTS): the mirror call produces it
    if want_agr and ensemble is not None:
        raise UNetError("output agreement is not available with ensemble (it counts one model's mirrored views)")
    if want_agr and mirror is None:
        raise UNetError("output agreement needs mirror")
    uncertainty = tuple(o for o in outputs if o in ("entropy", "mutual_info"))   # not chain outputs: the ensemble's finalize makes them
    if uncertainty and ensemble is None:
        raise UNetError("output %s needs ensemble" % uncertainty[0])
    outputs = tuple(o for o in outputs if o != "agreement" and o not in uncertainty)
    check_outputs(steps, outputs)
    from . import connectivity as CN
    CN.check(single_component_connectivity, "single_component")   # refused before any device work
    if tiles is not None and mirror is not None:
        raise UNetError("run_postproc: mirror does not combine with tiles or native")
    if ensemble is not None:
        src = _ensemble_source(ensemble, logits, native, tiles, mirror, steps, uncertainty)
    elif tiles is not None:
        src = _tile_source(tiles, logits, native)
    elif mirror is not None:
        src = _mirror_source(mirror, logits, native, want_agr)
    else:
        src = _tensor_source(logits)
    out_c, (D, H, W), dev = src.out_c, src.shape, src.device
    if native is not None:
        from . import space as SP
        native_map, (D, H, W) = native[0], SP._shape3(native[1], "native shape")
    S = D * H * W
    postproc_scratch_bytes(out_c, S)   # the class / size checks, before any device work
    listed = [int(v) for v in single_component] if single_component is not None else []
    for v in listed:
        if v <= 0 or v >= out_c:
            raise UNetError("single_component: class %d is not in [1, %d]" % (v, out_c - 1))
    if morphology:
        from . import morph as MO
        morphology = MO.check_ops(morphology, out_c)   # a bad op is refused before any device work
    names = [n for n, _ in steps]
    from_state = argmax_after_change(steps) and "label" in outputs
    want_lp = ("label_prob" in outputs or from_state) and "softmax" in names
    want_fg = "create_mask" in names and ("fg_prob" in outputs or "defragment" in names or from_state)
    want_lab = "argmax" in names and "label" in outputs
    changed = False
    res = {}

    def get_scratch():
        nonlocal scratch
        scratch = E.scratch(scratch, postproc_scratch_bytes(out_c, S), dev)
        return scratch

    i = 0
    while i < len(steps):
        name, p = steps[i]
        if name in ("softmax", "create_mask", "argmax"):
            j, run = i, {}
            while j < len(steps) and steps[j][0] in ("softmax", "create_mask", "argmax"):
                run[steps[j][0]] = steps[j][1]
                j += 1
            lp = fg = lab = None
            if "softmax" in run and want_lp:
                lp = res["label_prob"] = torch.empty((out_c - 1, D, H, W), dtype=torch.float32, device=dev)
            if "create_mask" in run and want_fg:
                fg = res["fg_prob"] = torch.empty((D, H, W), dtype=torch.float32, device=dev)
            if "argmax" in run and want_lab:
                lab = res["label"] = res.get("label", torch.empty((D, H, W), dtype=torch.uint16, device=dev))
            thr = run.get("argmax", {}).get("threshold", 0.5)
            fused_lab = lab if not changed else None      # after a change argmax reads the current planes, below
            if lp is not None or fg is not None or fused_lab is not None:
                wanted = {k: v for k, v in (("label_prob", lp), ("fg_prob", fg), ("label", fused_lab)) if v is not None}
                if native is not None:
                    SP.postproc_native(src.logits(), native_map, (D, H, W), thr, tuple(wanted), out=wanted)
                elif i == 0 and src.head is not None:
                    res.update(src.head(thr, wanted))
                else:
                    softmax_call(src.logits(), out_c, S, thr, lp, fg, fused_lab)
            if lab is not None and changed:
                argmax_planes_call(res["label_prob"], out_c - 1, S, res["fg_prob"], thr, lab)
            i = j
            continue
        changed = True   # every command below changes the state in place
        lp = res.get("label_prob")
        if name == "defragment":
            defragment_call((W, H, D), False, p["threshold"], p["size_ratio"], res["fg_prob"], lp, out_c - 1 if lp is not None else 0,
                            res.get("label"), get_scratch())
        elif name == "defragment_each":
            if lp is not None:
                defragment_call((W, H, D), True, p["threshold"], p["size_ratio"], None, lp, out_c - 1, None, get_scratch())
        elif lp is not None:   # a per-plane command: it only changes label_prob
            param = next(iter(p.values())) if p else 0.0
            plane_op_call(PLANE_OPS[name], param, (W, H, D), lp, out_c - 1, get_scratch())
        i += 1
    if want_agr and "agreement" not in res:            # no fused group at the head of the chain wrote it
        res["agreement"] = src.agreement()
    if want_agr:
        outputs += ("agreement",)
    missing = tuple(o for o in uncertainty if o not in res)
    if missing:                                        # the leading group had nothing to write: the maps alone
        from . import ensemble as EN
        res.update(EN.finalize(ensemble[0], out_c, (D, H, W), 0.5, missing))
    outputs += uncertainty
    if listed and "label" in outputs:
        from . import components as CMP
        CMP.keep_largest(res["label"], listed, out_c, scratch=component_scratch, connectivity=single_component_connectivity)
    if morphology and "label" in outputs:
        MO.run(res["label"], morphology, out_c, scratch=morphology_scratch)
    return {k: v for k, v in res.items() if k in outputs}
