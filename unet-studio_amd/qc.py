"""Quality control of the reference (qc.cpp) over the engine: per case, the share of voxels of every class whose argmax disagrees
with the label, written to `<model stem>.error_report.tsv` beside the model.

calculate_qc is qc.cpp:55-160: an eval forward that asks the engine for the full-resolution logits only, then ONE kernel
(include/unet_qc.h) for the subject-label shift (train.cpp:248-256), cast, collapse, argmax and the two per-class histograms.
run_qc / qc are qc.cpp:164-376.  Reading NIfTI / BIDS and resampling to model.dim are TIPL and out of scope (as in evaluate.py):
a case is (image_name, label_name, image, label, is_template) with image {in_count, D, H, W} and label {D, H, W} arrays (numpy or
fp32 device tensors) already at model.dim = (W, H, D).

The host rules (label information, shift predicate, bin mapping, report bytes) are plain functions that need no device."""
import ctypes as C
import os
import threading
import warnings

import numpy as np
import torch

from . import engine as E
from . import nz
from .engine import UNetError

E._sig("unet_qc_scratch_bytes", C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_qc_counts", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
       C.c_size_t, C.c_void_p)
# every symbol include/unet_qc.h declares
EXPORTS = ["unet_qc_scratch_bytes", "unet_qc_counts"]

DEFAULT_MAX_TEMPLATE_LABEL = 5   # qc.cpp:231-235


class QcStat:
    """qc_stat (qc.cpp:14-28)"""

    def __init__(self, voxels=0, wrong=0):
        self.voxels, self.wrong = int(voxels), int(wrong)

    def __iadd__(self, r):
        self.voxels += r.voxels
        self.wrong += r.wrong
        return self

    def ratio(self):
        return self.wrong / self.voxels if self.voxels else 0.0

    def __eq__(self, r):
        return isinstance(r, QcStat) and (self.voxels, self.wrong) == (r.voxels, r.wrong)

    def __repr__(self):
        return "QcStat(%d, %d)" % (self.voxels, self.wrong)


# ---- the device half ----------------------------------------------------------------------------------------------------------
def qc_scratch_bytes(out_c, voxels, collapse_before=0):
    return E.size_query(E.lib.unet_qc_scratch_bytes, int(out_c), int(voxels), int(collapse_before))


def _device_f32(a, name, device=None):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
        raise UNetError("qc_counts: %s must be a contiguous float32 device tensor" % name)
    if device is not None and a.device != device:
        raise UNetError("qc_counts: %s is on %s, the logits on %s" % (name, a.device, device))
    return a


def qc_counts(logits, label, collapse_before=0, image0=None, shift_by=0, scratch=None):
    """unet_qc_counts on the current stream.  logits: {1, C, D, H, W} or {C, ...} fp32 device tensor; label: fp32, one value per voxel;
    image0: input channel 0 (needed when shift_by > 0).  Returns the uint64 device tensor [voxels[0..C'), wrong[0..C')]."""
    _device_f32(logits, "logits")
    dev = logits.device
    _device_f32(label, "label", dev)
    out_c = int(logits.shape[1] if logits.dim() == 5 else logits.shape[0])
    S = label.numel()
    if logits.numel() != out_c * S:
        raise UNetError("qc_counts: logits hold %d values, not %d classes x %d voxels" % (logits.numel(), out_c, S))
    if image0 is not None:
        _device_f32(image0, "image0", dev)
        if image0.numel() < S:
            raise UNetError("qc_counts: image0 holds fewer than %d voxels" % S)
    need = qc_scratch_bytes(out_c, S, collapse_before)
    scratch = E.scratch(scratch, need, dev)
    cp = out_c - collapse_before + 1 if collapse_before else out_c
    counts = torch.empty(2 * cp, dtype=torch.uint64, device=dev)
    E.check(E.lib.unet_qc_counts(logits.data_ptr(), label.data_ptr(), image0.data_ptr() if image0 is not None else None, out_c, S,
                                 int(collapse_before), int(shift_by), counts.data_ptr(), scratch.data_ptr(),
                                 scratch.nbytes, E.stream(dev)))
    return counts


def stats_from_counts(counts, out_count, collapse_before=0):
    """qc.cpp:137-155: the kernel's bins -> (stats[out_count], overall).  With collapse, bin 0 (the merged classes 0..k-1) goes into
    overall only and stats[0..k) stay empty."""
    counts = [int(v) for v in counts]
    cp = out_count - collapse_before + 1 if collapse_before else out_count
    if len(counts) != 2 * cp:
        raise UNetError("qc: %d counts, expected %d" % (len(counts), 2 * cp))
    stats, overall = [QcStat() for _ in range(out_count)], QcStat()
    for c in range(cp):
        s = QcStat(counts[c], counts[cp + c])
        overall += s
        if not collapse_before:
            stats[c] = s
        elif c:
            stats[collapse_before + c - 1] = s
    return stats, overall


def _to_device(a, device):
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def calculate_qc(model, image, label, collapse_before=0, shift_by=0, scratch=None):
    """qc.cpp:55-160 (with shift_subject_label applied to the label on the device when shift_by > 0) -> (stats[out_count], overall).
    Raises UNetError with the reference's messages."""
    W, H, D = (int(v) for v in model.dim)
    S = D * H * W
    if int(np.prod(image.shape)) != S * model.in_count or int(np.prod(label.shape)) != S:
        raise UNetError("training data dimension mismatch")
    if not 0 <= collapse_before < model.out_count:
        raise UNetError("invalid collapse_before")
    dev = model.device()
    x = _to_device(image, dev).view(1, model.in_count, D, H, W)
    t = _to_device(label, dev).view(-1)
    with torch.no_grad():
        logits = model._forward_level0(x)
    if logits is None or tuple(logits.shape) != (1, model.out_count, D, H, W):
        raise UNetError("model output dimension mismatch")
    counts = qc_counts(logits, t, collapse_before, x.view(-1)[:S] if shift_by > 0 else None, shift_by, scratch)
    return stats_from_counts(counts.cpu().tolist(), model.out_count, collapse_before)


# ---- the host half --------------------------------------------------------------------------------------------------------
def max_label_of(label):
    """max value of the label read as int (read_label_info, train.cpp:229-246: tipl::image<3,int>, truncation toward zero)"""
    if torch.is_tensor(label):
        return int(torch.trunc(label.to(torch.float32)).max())
    return int(np.trunc(np.asarray(label, dtype=np.float32)).max())


def label_plan(cases, out_count, warn=True, max_of=max_label_of):
    """qc.cpp:200-253 -> (max_template_label, shift flag per case).  The label information is read once per distinct label name;
    max_of(label) reads it (feed.py passes the maxima it took on the device)."""
    info = {}
    mtl = 0
    for case in cases:
        name, is_template = case[1], bool(case[4])
        if name not in info:
            info[name] = (is_template, max_of(case[3]))
        if info[name][0]:
            mtl = max(mtl, info[name][1])
    if not mtl:
        if warn:
            warnings.warn("no template label found; use default %d" % DEFAULT_MAX_TEMPLATE_LABEL)
        mtl = DEFAULT_MAX_TEMPLATE_LABEL
    shift = []
    for case in cases:
        is_template, max_label = info[case[1]]
        shift.append(not is_template and max_label < mtl and max_label + mtl < out_count)
    return mtl, shift


def case_settings(shifted, max_template_label):
    """(collapse_before, shift_by) of one case (qc.cpp:268,297)"""
    return (max_template_label + 1, max_template_label) if shifted else (0, 0)


def report_path(model_path):
    d, f = os.path.split(model_path)
    return os.path.join(d, os.path.splitext(f)[0] + ".error_report.tsv")


def format_report(out_count, rows):
    """the report text (qc.cpp:35-52,341-360, std::setprecision(9)); rows: (image, label, stats, overall, unavailable_before)"""
    lines = ["image\tground_truth\twrong_ratio" + "".join("\twrong_ratio%d" % c for c in range(out_count))]
    for image, label, stats, overall, unavailable in rows:
        cols = [os.path.basename(image), os.path.basename(label), "%.9g" % overall.ratio()]
        cols += ["N/A" if c < unavailable else "%.9g" % s.ratio() for c, s in enumerate(stats)]
        lines.append("\t".join(cols))
    return "\n".join(lines) + "\n"


def write_report(model_path, out_count, rows):
    """through <report>.tmp, then the old report removed and the new one renamed into place (qc.cpp:334-372) -> (0, report) or
    (1, message)"""
    report = report_path(model_path)
    tmp = report + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(format_report(out_count, rows).encode())
    except OSError as e:
        return 1, "failed writing %s: %s" % (tmp, e)
    try:
        if os.path.lexists(report):
            os.remove(report)
        os.rename(tmp, report)
    except OSError as e:
        return 1, "cannot create %s: %s" % (report, e)
    return 0, report


def run_qc(model, model_path, cases, thread_count=4):
    """qc.cpp:200-376 on a loaded, prepared model -> (0, report path) or (1, message).  Up to 4 worker threads share the model;
    each has its own stream, QC scratch and (unet3d.py:_workspace, per host thread) workspace.  The first failure stops the others
    and no report is written."""
    cases = list(cases)
    if not cases:
        return 1, "no image/label pairs found"
    mtl, shift = label_plan(cases, model.out_count)
    W, H, D = (int(v) for v in model.dim)
    dev = model.device()
    model.plan_for((D, H, W))                     # made here: the workers only look it up
    n_workers = min(4, max(1, int(thread_count)), len(cases))
    stats, errors = [None] * len(cases), [""] * len(cases)
    lock, failed, nxt = threading.Lock(), threading.Event(), [0]

    def worker():
        with torch.cuda.device(dev), torch.no_grad():
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                scratch = torch.empty(qc_scratch_bytes(model.out_count, D * H * W), dtype=torch.uint8, device=dev)
                while not failed.is_set():
                    with lock:
                        i = nxt[0]
                        nxt[0] += 1
                    if i >= len(cases):
                        break
                    try:
                        collapse, shift_by = case_settings(shift[i], mtl)
                        stats[i] = calculate_qc(model, cases[i][2], cases[i][3], collapse, shift_by, scratch)
                        continue
                    except Exception as e:   # qc.cpp:300-309
                        errors[i] = str(e) or "unknown QC error"
                    failed.set()
                    break

    if n_workers == 1:
        worker()
    else:
        threads = [threading.Thread(target=worker) for _ in range(n_workers)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    if failed.is_set():
        for i, e in enumerate(errors):
            if e:
                return 1, "%s: %s" % (cases[i][0], e)
        return 1, "QC failed"
    rows = [(c[0], c[1], s[0], s[1], case_settings(sh, mtl)[0]) for c, s, sh in zip(cases, stats, shift)]
    return write_report(model_path, model.out_count, rows)


# ---- boundary distances per class (this project's: the reference's QC stops at the wrong-voxel ratios) ------------------------------
def surface_report_path(model_path):
    d, f = os.path.split(model_path)
    return os.path.join(d, os.path.splitext(f)[0] + ".surface_report.tsv")


def format_surface_report(out_count, rows):
    """the report text; rows: (image, label, summary) with summary the float64 {out_count, 3} of distance.summary (hd, hd95, assd in
    mm per class), or None for a case whose classes are not the model's (a shifted label): N/A in every column"""
    lines = ["image\tground_truth" + "".join("\thd%d\thd95%d\tassd%d" % (c, c, c) for c in range(1, out_count))]
    for image, label, summary in rows:
        cols = [os.path.basename(image), os.path.basename(label)]
        for c in range(1, out_count):
            cols += ["N/A"] * 3 if summary is None else ["%.9g" % v for v in summary[c]]
        lines.append("\t".join(cols))
    return "\n".join(lines) + "\n"


def surface_qc(model, model_path, cases, labels=None):
    """Per case and class 1..out_count-1, the Hausdorff distance, its 95th percentile and the average symmetric surface distance in mm
    between the argmax of the model's output and the label (distance.py, include/unet_distance.h), written to
    `<model stem>.surface_report.tsv` beside the model -> (0, report path) or (1, message).  labels: the classes to measure (None:
    all; the others read nan).  A case that label_plan marks as shifted gets N/A in every column: its classes are not the model's."""
    from . import distance as DS
    cases = list(cases)
    if not cases:
        return 1, "no image/label pairs found"
    if model.out_count < 2:
        return 1, "QC requires a categorical model"
    W, H, D = (int(v) for v in model.dim)
    S = D * H * W
    dev = model.device()
    rows = []
    try:
        _, shift = label_plan(cases, model.out_count)
        weights, unit_mm2 = DS.metric(model.voxel_size, (W, H, D))
        scratch = torch.empty(DS.distance_scratch_bytes((W, H, D)), dtype=torch.uint8, device=dev)
        for case, shifted in zip(cases, shift):
            summary = None
            if not shifted:
                image, label = case[2], case[3]
                if int(np.prod(image.shape)) != S * model.in_count or int(np.prod(label.shape)) != S:
                    raise UNetError("%s: training data dimension mismatch" % case[0])
                x = _to_device(image, dev).view(1, model.in_count, D, H, W)
                with torch.no_grad():
                    logits = model._forward_level0(x)
                if logits is None or tuple(logits.shape) != (1, model.out_count, D, H, W):
                    raise UNetError("%s: model output dimension mismatch" % case[0])
                got = torch.argmax(logits[0], dim=0).to(torch.int32).to(torch.uint16).contiguous()
                want = torch.trunc(_to_device(label, dev)).clamp_(0, 65535).to(torch.int32).to(torch.uint16).view(D, H, W).contiguous()
                res = DS.surface_distances(got, want, model.out_count - 1, weights, labels=labels, scratch=scratch)
                summary = DS.summary(res, unit_mm2)
            rows.append((case[0], case[1], summary))
    except UNetError as e:
        return 1, str(e)
    report = surface_report_path(model_path)
    tmp = report + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(format_surface_report(model.out_count, rows).encode())
    except OSError as e:
        return 1, "failed writing %s: %s" % (tmp, e)
    try:
        if os.path.lexists(report):
            os.remove(report)
        os.rename(tmp, report)
    except OSError as e:
        return 1, "cannot create %s: %s" % (report, e)
    return 0, report


# ---- lesion-wise detection per class (this project's: the reference's QC stops at the wrong-voxel ratios) ----------------------------
LESION_COLUMNS = ("n_ref", "n_pred", "detected", "false_pos", "sensitivity", "precision", "f1")


def lesion_report_path(model_path):
    d, f = os.path.split(model_path)
    return os.path.join(d, os.path.splitext(f)[0] + ".lesion_report.tsv")


def format_lesion_report(out_count, rows):
    """the report text; rows: (image, label, scores) with scores the dict of instances.detection (arrays of out_count entries), or
    None for a case whose classes are not the model's (a shifted label): N/A in every column"""
    lines = ["image\tground_truth" + "".join("\t%s%d" % (k, c) for c in range(1, out_count) for k in LESION_COLUMNS)]
    for image, label, scores in rows:
        cols = [os.path.basename(image), os.path.basename(label)]
        for c in range(1, out_count):
            cols += ["N/A"] * len(LESION_COLUMNS) if scores is None else [
                "%d" % scores[k][c] if scores[k].dtype.kind == "i" else "%.9g" % scores[k][c] for k in LESION_COLUMNS]
        lines.append("\t".join(cols))
    return "\n".join(lines) + "\n"


def lesion_qc(model, model_path, cases, labels=None, rule="any", threshold=0.0, min_voxels=1, connectivity=6):
    """Per case and class 1..out_count-1, the lesion-wise detection scores (instances.py, include/unet_instances.h) of the argmax of
    the model's output against the label: the `connectivity`-connected (6, 18 or 26) instances of both maps with at least min_voxels voxels, a reference
    instance detected and a predicted one true when a pair of one class overlaps (rule "any") or reaches the IoU `threshold` (rule
    "iou").  Written to `<model stem>.lesion_report.tsv` beside the model -> (0, report path) or (1, message).  labels: the classes
    to score (None: all; the others count nothing and read nan).  A case that label_plan marks as shifted gets N/A in every column.
    The report's format does not depend on the connectivity; a bad one gives (1, message)."""
    from . import connectivity as CN
    from . import instances as IN
    try:
        CN.check(connectivity, "lesion_qc")
    except UNetError as e:
        return 1, str(e)
    cases = list(cases)
    if not cases:
        return 1, "no image/label pairs found"
    if model.out_count < 2:
        return 1, "QC requires a categorical model"
    W, H, D = (int(v) for v in model.dim)
    S = D * H * W
    dev = model.device()
    rows = []
    try:
        _, shift = label_plan(cases, model.out_count)
        scratch = torch.empty(IN.inst_scratch_bytes(S, model.out_count, IN.DEFAULT_MAX_INSTANCES), dtype=torch.uint8, device=dev)
        for case, shifted in zip(cases, shift):
            scores = None
            if not shifted:
                image, label = case[2], case[3]
                if int(np.prod(image.shape)) != S * model.in_count or int(np.prod(label.shape)) != S:
                    raise UNetError("%s: training data dimension mismatch" % case[0])
                x = _to_device(image, dev).view(1, model.in_count, D, H, W)
                with torch.no_grad():
                    logits = model._forward_level0(x)
                if logits is None or tuple(logits.shape) != (1, model.out_count, D, H, W):
                    raise UNetError("%s: model output dimension mismatch" % case[0])
                got = torch.argmax(logits[0], dim=0).to(torch.int32).to(torch.uint16).contiguous()
                want = torch.trunc(_to_device(label, dev)).clamp_(0, 65535).to(torch.int32).to(torch.uint16).view(D, H, W).contiguous()
                scores = IN.lesion_scores(got, want, model.out_count, classes=labels, rule=rule, threshold=threshold,
                                          min_voxels=min_voxels, scratch=scratch, connectivity=connectivity)
            rows.append((case[0], case[1], scores))
    except UNetError as e:
        return 1, str(e)
    report = lesion_report_path(model_path)
    tmp = report + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(format_lesion_report(model.out_count, rows).encode())
    except OSError as e:
        return 1, "failed writing %s: %s" % (tmp, e)
    try:
        if os.path.lexists(report):
            os.remove(report)
        os.rename(tmp, report)
    except OSError as e:
        return 1, "cannot create %s: %s" % (report, e)
    return 0, report


# ---- calibration of the probabilities (this project's: the only family that judges the probabilities, not the label map) --------------
CALIBRATION_COLUMNS = ("voxels", "accuracy", "ece", "mce", "brier", "nll")
CALIBRATION_MASKS = ("all", "foreground")


def calibration_report_path(model_path):
    d, f = os.path.split(model_path)
    return os.path.join(d, os.path.splitext(f)[0] + ".calibration_report.tsv")


def calibration_scores(table, out_count, bins=10, hists=None):
    """The scores of one calibration table (calib.py) as a dict: voxels (the valid ones), accuracy, ece, mce, brier (summed over the
    classes), nll (the estimate of calib.nll_bounds), cw_ece and brier_c (arrays of out_count entries), and with hists = (h_correct,
    h_wrong) of calib.uncertainty_hists also auroc_entropy and aurc_entropy."""
    from . import calib as CB
    head, top, cls, logh = CB.split(table, out_count)
    per, total = CB.brier(cls)
    s = {"voxels": int(head[CB.VALID]), "accuracy": CB.accuracy(top), "ece": CB.ece(top, bins), "mce": CB.mce(top, bins), "brier": total,
         "nll": CB.nll_bounds(logh)[1], "cw_ece": CB.classwise_ece(cls, bins), "brier_c": per}
    if hists is not None:
        s["auroc_entropy"] = CB.auroc(*hists)
        s["aurc_entropy"] = CB.risk_coverage(*hists)[2]
    return s


def format_calibration_report(out_count, rows, with_entropy=False):
    """the report text; rows: (image, label, scores) with scores the dict of calibration_scores, or None for a case whose classes are
    not the model's (a shifted label): N/A in every column.  The last row, named total, has an empty ground_truth."""
    extra = ("auroc_entropy", "aurc_entropy") if with_entropy else ()
    lines = ["image\tground_truth\t" + "\t".join(CALIBRATION_COLUMNS) + "".join("\tcw_ece%d" % c for c in range(out_count))
             + "".join("\tbrier%d" % c for c in range(out_count)) + "".join("\t" + k for k in extra)]
    width = len(CALIBRATION_COLUMNS) + 2 * out_count + len(extra)
    for image, label, s in rows:
        cols = [os.path.basename(image), os.path.basename(label)]
        if s is None:
            cols += ["N/A"] * width
        else:
            cols += ["%d" % s["voxels"]] + ["%.9g" % s[k] for k in CALIBRATION_COLUMNS[1:]]
            cols += ["%.9g" % v for v in s["cw_ece"]] + ["%.9g" % v for v in s["brier_c"]] + ["%.9g" % s[k] for k in extra]
        lines.append("\t".join(cols))
    return "\n".join(lines) + "\n"


def calibration_qc(model, model_path, cases, bins=10, ensemble=None, ensemble_weights=None, mask="all"):
    """Per case, whether the model's probabilities mean anything (calib.py, include/unet_calib.h): the valid voxels, the accuracy, the
    expected and the maximum calibration error over `bins` confidence bins (a divisor of 20), the Brier score, the negative
    log-likelihood, and per class the class-wise ECE and the Brier score, written to `<model stem>.calibration_report.tsv` beside
    the model with a last row `total` over all cases -> (0, report path) or (1, message).  ensemble: a list of further models
    (`model` is member 0; ensemble_weights as in ensemble.normalize_weights): the mean probabilities are judged, and
    auroc_entropy / aurc_entropy say whether the wrong voxels are the high-entropy ones.  mask: "all", or "foreground" for the
    voxels whose truth or whose prediction is not the background.  A case that label_plan marks as shifted gets N/A in every column."""
    from . import calib as CB
    from . import ensemble as EN
    cases = list(cases)
    if not cases:
        return 1, "no image/label pairs found"
    if model.out_count < 2:
        return 1, "QC requires a categorical model"
    if mask not in CALIBRATION_MASKS:
        return 1, "calibration_qc: mask must be one of %s, got %r" % (", ".join(CALIBRATION_MASKS), mask)
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 1 or CB.BINS % bins:
        return 1, "calibration_qc: bins must divide %d, got %r" % (CB.BINS, bins)
    if ensemble is None and ensemble_weights is not None:
        return 1, "ensemble_weights needs ensemble"
    if ensemble is not None and not isinstance(ensemble, (list, tuple)):
        return 1, "ensemble must be a list of further models, got %r" % (ensemble,)
    members = [model] + list(ensemble or [])
    out_c = model.out_count
    for k, other in enumerate(members[1:], 1):
        for what in ("in_count", "out_count", "dim"):
            if not hasattr(other, what):
                return 1, "ensemble: member %d is not a model (it has no %s)" % (k, what)
            a, b = getattr(other, what), getattr(model, what)
            a, b = (tuple(a), tuple(b)) if what == "dim" else (a, b)
            if a != b:
                return 1, "ensemble: member %d has %s %s, member 0 has %s" % (k, what, a, b)
    W, H, D = (int(v) for v in model.dim)
    S = D * H * W
    dev = model.device()
    rows = []
    try:
        weights = EN.normalize_weights(ensemble_weights, len(members)) if ensemble is not None else None
        _, shift = label_plan(cases, out_c)
        n = CB.table_len(out_c)
        total, table = torch.zeros(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        scratch = torch.empty(CB.scratch_bytes(out_c, S), dtype=torch.uint8, device=dev)
        wrong = torch.empty(S, dtype=torch.uint8, device=dev) if ensemble is not None else None
        state = EN.new_state(out_c, S, dev) if ensemble is not None else None
        hist_total = torch.zeros(2, 256, dtype=torch.int64, device=dev)
        ln_c = float(np.log(out_c))
        for case, shifted in zip(cases, shift):
            scores = None
            if not shifted:
                image, label = case[2], case[3]
                if int(np.prod(image.shape)) != S * model.in_count or int(np.prod(label.shape)) != S:
                    raise UNetError("%s: training data dimension mismatch" % case[0])
                x = _to_device(image, dev).view(1, model.in_count, D, H, W)
                t = _to_device(label, dev).view(-1)
                with torch.no_grad():
                    for k, member in enumerate(members):
                        logits = member._forward_level0(x)
                        if logits is None or tuple(logits.shape) != (1, out_c, D, H, W):
                            raise UNetError("%s: model output dimension mismatch" % case[0])
                        if state is not None:
                            EN.accumulate(logits, state, weights[k], k == 0)
                planes = logits[0].view(out_c, S) if state is None else state[:out_c * S * 4].view(torch.float32).view(out_c, S)
                region = None
                if mask == "foreground":
                    region = ((torch.trunc(t) != 0) | (torch.argmax(planes, dim=0) != 0)).to(torch.uint8).contiguous()
                hists = None
                if state is None:
                    CB.tables(logits[0], t, mask=region, out=table, scratch=scratch)
                else:
                    CB.tables_from_probs(state, out_c, S, t, mask=region, out=table, wrong=wrong, scratch=scratch)
                    entropy = EN.finalize(state, out_c, (D, H, W), outputs=("entropy",))["entropy"]
                    hc, hw = CB.uncertainty_hists(wrong, entropy, 0.0, ln_c)
                    hist_total[0] += hc
                    hist_total[1] += hw
                    hists = (hc.cpu(), hw.cpu())
                total += table
                scores = calibration_scores(table, out_c, bins, hists)
            rows.append((case[0], case[1], scores))
        if not all(shift):
            rows.append(("total", "", calibration_scores(total, out_c, bins, tuple(hist_total.cpu()) if state is not None else None)))
        else:
            rows.append(("total", "", None))
    except UNetError as e:
        return 1, str(e)
    report = calibration_report_path(model_path)
    tmp = report + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(format_calibration_report(out_c, rows, ensemble is not None).encode())
    except OSError as e:
        return 1, "failed writing %s: %s" % (tmp, e)
    try:
        if os.path.lexists(report):
            os.remove(report)
        os.rename(tmp, report)
    except OSError as e:
        return 1, "cannot create %s: %s" % (report, e)
    return 0, report


def recalibration_qc(model, model_path, cases, mask="all", u_range=(-4.0, 4.0), rounds=3, apply=False):
    """Fits one temperature to the model's level-0 logits over the cases (recal.py, include/unet_recal.h) and says what it buys: per
    case the valid voxels and the mean negative log-likelihood before (beta = 1) and after (the fitted beta = 1 / T), written to
    `<model stem>.recalibration_report.tsv` beside the model with a last row `total` that also carries beta, temperature, the
    bracket, at_bound and the impossible and saturated voxels -> (0, report path) or (1, message).  u_range: the octaves of
    log2 beta that are searched, rounds: of 8 candidates each (every round re-runs the forwards).  mask as in calibration_qc.  A case
    that label_plan marks as shifted gets N/A and takes no part in the fit.  apply: fold beta into the model's level-0 head after
    the closing pass (recal.fold: the head must be a bare conv); the caller saves the model."""
    from . import recal as RC
    cases = list(cases)
    if not cases:
        return 1, "no image/label pairs found"
    if model.out_count < 2:
        return 1, "QC requires a categorical model"
    if mask not in CALIBRATION_MASKS:
        return 1, "recalibration_qc: mask must be one of %s, got %r" % (", ".join(CALIBRATION_MASKS), mask)
    try:
        u_lo, u_hi = (float(v) for v in u_range)
    except (TypeError, ValueError):
        return 1, "recalibration_qc: u_range must be (u_lo, u_hi), got %r" % (u_range,)
    try:
        solver = RC.Solver(u_lo, u_hi, rounds)
    except UNetError as e:
        return 1, "recalibration_qc: %s" % e
    if apply and not RC.head_is_bare_conv(model.architecture):
        return 1, "recalibration_qc: the level-0 head %r is not a bare conv: beta cannot be folded in" % RC.head_token(model.architecture)
    out_c = model.out_count
    W, H, D = (int(v) for v in model.dim)
    S = D * H * W
    dev = model.device()
    try:
        _, shift = label_plan(cases, out_c)

        def batches():
            for case, shifted in zip(cases, shift):
                if shifted:
                    continue
                image, label = case[2], case[3]
                if int(np.prod(image.shape)) != S * model.in_count or int(np.prod(label.shape)) != S:
                    raise UNetError("%s: training data dimension mismatch" % case[0])
                x = _to_device(image, dev).view(1, model.in_count, D, H, W)
                t = _to_device(label, dev).view(-1)
                with torch.no_grad():
                    logits = model._forward_level0(x)
                if logits is None or tuple(logits.shape) != (1, out_c, D, H, W):
                    raise UNetError("%s: model output dimension mismatch" % case[0])
                region = None
                if mask == "foreground":
                    region = ((torch.trunc(t) != 0) | (torch.argmax(logits[0].view(out_c, S), dim=0) != 0)).to(torch.uint8).contiguous()
                yield logits[0], t, region

        rows, fitted, total = [], None, None
        if not all(shift):
            fitted = RC.fit(batches, solver=solver)
            total = torch.zeros(RC.TABLE_LEN, dtype=torch.int64, device=dev)
            table = torch.empty(RC.TABLE_LEN, dtype=torch.int64, device=dev)
            closing = iter(batches())
        for case, shifted in zip(cases, shift):
            if shifted:
                rows.append((case[0], case[1], None))
                continue
            logits, t, region = next(closing)
            RC.eval_betas(logits, t, (1.0, fitted["beta"]), mask=region, out=table)
            total += table
            rows.append((case[0], case[1], table.cpu()))
        if fitted is not None:
            fitted["table"] = total.cpu()
        text = RC.format_report(rows, fitted)
        if apply and fitted is not None:
            RC.fold(model, fitted["beta"])
    except UNetError as e:
        return 1, str(e)
    report = RC.report_path(model_path)
    tmp = report + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(text.encode())
    except OSError as e:
        return 1, "failed writing %s: %s" % (tmp, e)
    try:
        if os.path.lexists(report):
            os.remove(report)
        os.rename(tmp, report)
    except OSError as e:
        return 1, "cannot create %s: %s" % (report, e)
    return 0, report


def qc(model_path, cases, device="cuda:0", dtype="bf16", thread_count=4):
    """int qc(void) (qc.cpp:164-376) for cases already read -> (0, report path) or (1, message)"""
    from .unet3d import UNet3d
    if not os.path.exists(model_path):
        return 1, "cannot find model %s" % model_path
    try:
        model = nz.load_from_file(model_path, lambda i, o, a: UNet3d(i, o, a, device=device, dtype=dtype))
    except (nz.NzError, UNetError) as e:
        return 1, "cannot load model %s: %s" % (model_path, e)
    if model.out_count < 2:
        return 1, "QC requires a categorical model"
    model.prepare_for_inference(device)
    return run_qc(model, model_path, cases, thread_count)
