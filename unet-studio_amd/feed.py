"""The reference's template/subject training feed (train.cpp:259-486) over the engine: a sample source for `Trainer`.

What the reader thread (train.cpp:267-435) and the augmentation threads (:437-480) do per sample, on the device:
  schedule   seed_id -> a template or a subject case: std::mt19937(seed) and two std::uniform_int_distribution<int> (train.cpp:
             391-401), run by the library's own C++ (include/unet_feed.h unet_feed_schedule), so the order is the reference's
  prepare    tipl::normalize when !is_label, shift_subject_label for a shifted subject (:415-419; unet_feed_prepare).  Templates are
             prepared once and kept on the device, as the reference caches train_image / train_label (:421-425)
  simulate   simulate_modality: with the label and max_label = out_count for a template, without for a subject (:459-462)
  augment    visual_perception_augmentation with seed = seed_id (:472)
  target     .to(torch::kLong) (:615-617; unet_feed_target)
and the bookkeeping the step needs (label plan, has_subject_data, the test set of :345-380).  `sample_info(i)` tells the trainer
where sample i came from: it then trains a shifted subject with collapse_before = max_template_label + 1 (:673-674) and counts
training errors over subject samples only when subject data exist (:676-682).

A case is (image_name, label_name, image {in_count, D, H, W}, label {D, H, W}, is_template), numpy or fp32 device arrays already at
model.dim = (W, H, D), as in qc.py; reading NIfTI / BIDS stays out of scope.  The caller's arrays are never written."""
import ctypes as C
import os

import numpy as np
import torch

from . import augment as G
from . import engine as E
from . import qc as Q
from .engine import UNetError

E._sig("unet_feed_scratch_bytes", C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_feed_label_max", C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_feed_prepare", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
       C.c_void_p)
E._sig("unet_feed_target", C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_feed_schedule", C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
       C.POINTER(C.c_int32))
# every symbol include/unet_feed.h declares
EXPORTS = ["unet_feed_scratch_bytes", "unet_feed_label_max", "unet_feed_prepare", "unet_feed_target", "unet_feed_schedule"]


# ---- the device calls ----------------------------------------------------------------------------------------------------------
def feed_scratch_bytes(voxels):
    return E.size_query(E.lib.unet_feed_scratch_bytes, int(voxels))


def _f32(a, name):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
        raise UNetError("feed: %s must be a contiguous float32 device tensor" % name)
    return a


def _scratch(voxels, device, scratch):
    need = feed_scratch_bytes(voxels)
    return E.scratch(scratch, need, device)


def label_max(label, out=None, scratch=None):
    """unet_feed_label_max on the current stream -> int32 device tensor {1}: max of the label read as int (read_label_info)"""
    _f32(label, "label")
    out = out if out is not None else torch.empty(1, dtype=torch.int32, device=label.device)
    sc = _scratch(label.numel(), label.device, scratch)
    E.check(E.lib.unet_feed_label_max(label.data_ptr(), label.numel(), out.data_ptr(), sc.data_ptr(), sc.numel(), E.stream(label)))
    return out


def prepare(label, image0=None, normalize=False, shift_by=0, label_max_out=None, scratch=None):
    """unet_feed_prepare in place on `label` (train.cpp:415-419): l / max(l) when normalize, then the subject shift when shift_by > 0
    (image0: input channel 0).  label_max_out (int32 device tensor, optional) receives the max of the label as it was."""
    _f32(label, "label")
    S = label.numel()
    if shift_by > 0 and (image0 is None or _f32(image0, "image0").numel() < S or image0.device != label.device):
        raise UNetError("feed: a shifted label needs input channel 0 of at least %d voxels on the label's device" % S)
    sc = _scratch(S, label.device, scratch)
    E.check(E.lib.unet_feed_prepare(image0.data_ptr() if shift_by > 0 else None, label.data_ptr(), S, int(bool(normalize)),
                                    int(shift_by), label_max_out.data_ptr() if label_max_out is not None else None, sc.data_ptr(),
                                    sc.numel(), E.stream(label)))
    return label


def target(label, normalize=False, out=None, scratch=None):
    """unet_feed_target -> int64 device tensor of the label's shape: (int64)l toward zero, after l / max(l) when normalize"""
    _f32(label, "label")
    if out is None:
        out = torch.empty(label.shape, dtype=torch.int64, device=label.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != label.numel() or out.device != label.device:
        raise UNetError("feed: target must be a contiguous int64 tensor of the label's size and device")
    sc = _scratch(label.numel(), label.device, scratch)
    E.check(E.lib.unet_feed_target(label.data_ptr(), label.numel(), int(bool(normalize)), out.data_ptr(), sc.data_ptr(), sc.numel(),
                                   E.stream(label)))
    return out


# ---- the host rules --------------------------------------------------------------------------------------------------------------
def schedule(seed, batch_size, n_template, n_subject, first, count):
    """unet_feed_schedule -> (case position int32[count], is_template bool[count]) for seed_id in [first, first + count)"""
    case = np.zeros(max(0, int(count)), dtype=np.int32)
    tpl = np.zeros_like(case)
    E.check(E.lib.unet_feed_schedule(int(seed) & 0xFFFFFFFFFFFFFFFF, int(batch_size), int(n_template), int(n_subject), int(first),
                                     int(count), case.ctypes.data_as(C.POINTER(C.c_int32)), tpl.ctypes.data_as(C.POINTER(C.c_int32))))
    return case, tpl.astype(bool)


def _byte_size(a):
    return a.numel() * a.element_size() if torch.is_tensor(a) else np.asarray(a).nbytes


def choose_test_cases(cases):
    """train.cpp:345-352: up to 2 template cases by descending (size, index); size = the image file's size when it exists, the
    image's byte count otherwise"""
    cand = []
    for i, case in enumerate(cases):
        if case[4]:
            name = case[0]
            size = os.path.getsize(name) if isinstance(name, str) and os.path.isfile(name) else _byte_size(case[2])
            cand.append((int(size), i))
    cand.sort(reverse=True)
    return [i for _, i in cand[:2]]


class TrainingFeed:
    """Sample source of train_unet::read_file (train.cpp:259-486): `feed(i)` -> (x fp32 {1,in,D,H,W}, t int64 {1,D,H,W}) of
    seed_id i, a pure function of i (a trainer resumed at cur_epoch > 0 gets the samples a fresh one would).

    param: TrainingParam (seed, batch_size); options: the augmentation options (augment.DEFAULT_OPTIONS for missing keys);
    is_label: param.is_label (False: labels are normalized, train.cpp:415-416).  Templates and the test set live on the model's
    device from construction on; subject cases are copied there too and prepared per sample."""

    def __init__(self, model, cases, param, options=None, is_label=True):
        self.model, self.param, self.options, self.is_label = model, param, options, bool(is_label)
        cases = list(cases)
        if not cases:
            raise UNetError("no image/label pairs found")
        W, H, D = (int(v) for v in model.dim)
        self.size, self.voxels = (D, H, W), D * H * W
        dev = model.device()
        self.device = dev
        self.cases = cases
        images, labels = [], []
        for case in cases:
            if int(np.prod(case[2].shape)) != self.voxels * model.in_count or int(np.prod(case[3].shape)) != self.voxels:
                raise UNetError("training data dimension mismatch: %s" % case[0])
            images.append(Q._to_device(case[2], dev).view(1, model.in_count, D, H, W))
            labels.append(Q._to_device(case[3], dev).view(D, H, W))
        self.templates = [i for i, c in enumerate(cases) if c[4]]
        self.subjects = [i for i, c in enumerate(cases) if not c[4]]
        self.has_subject_data = bool(self.subjects)
        if self.templates and model.out_count >= G.SIM_MAX_LABELS:
            raise UNetError("feed: simulate_modality takes labels up to %d; out_count is %d" % (G.SIM_MAX_LABELS - 1, model.out_count))
        self._sc = {}

        # the label information (train.cpp:270-336), read once per distinct label name; templates are prepared in the same call
        with torch.cuda.device(dev):
            sc = self._scratch("feed", feed_scratch_bytes(self.voxels))
            first = {}
            for i, case in enumerate(cases):
                first.setdefault(case[1], i)
            dev_max = torch.empty(len(cases), dtype=torch.int32, device=dev)
            self._tpl_label = {}
            for i, case in enumerate(cases):
                if case[4]:
                    lab = labels[i].clone()
                    prepare(lab, normalize=not self.is_label, label_max_out=dev_max[i:i + 1], scratch=sc)
                    self._tpl_label[i] = lab
                elif first[case[1]] == i:
                    label_max(labels[i], out=dev_max[i:i + 1], scratch=sc)
            host_max = dev_max.cpu().tolist()   # the one host read of the label plan
        by_name = {case[1]: host_max[first[case[1]]] for case in cases}
        plan_cases = [(c[0], c[1], None, c[1], c[4]) for c in cases]   # the label slot carries the name: max_of looks it up
        self.max_template_label, self.shifted = Q.label_plan(plan_cases, model.out_count, max_of=by_name.__getitem__)
        self._images, self._labels = images, labels
        self._test = choose_test_cases(cases)
        self._sched_case = np.zeros(0, np.int32)
        self._sched_tpl = np.zeros(0, bool)

    def _scratch(self, what, nbytes):
        """scratch per (kind, stream): samples made on two streams never share it"""
        key = (what, E.stream(self.device))
        sc = self._sc[key] = E.scratch(self._sc.get(key), nbytes, self.device)
        return sc

    def _case_of(self, index):
        if index < 0:
            raise UNetError("feed: sample index must not be negative")
        if index >= len(self._sched_case):
            n = max(1024, 2 * len(self._sched_case), index + 1)
            self._sched_case, self._sched_tpl = schedule(self.param.seed, self.param.batch_size, len(self.templates),
                                                         len(self.subjects), 0, n)
        is_template = bool(self._sched_tpl[index])
        pos = int(self._sched_case[index])
        return (self.templates if is_template else self.subjects)[pos], is_template

    def case_index(self, index):
        """the position in `cases` of sample `index` (read_id, train.cpp:401)"""
        return self._case_of(index)[0]

    def sample_info(self, index):
        """(is_template, is_shifted) of sample `index`; host only"""
        i, is_template = self._case_of(index)
        return is_template, bool(self.shifted[i])

    def __call__(self, index):
        i, is_template = self._case_of(index)
        D, H, W = self.size
        S = self.voxels
        x = self._images[i].clone()
        t1w = x.view(-1)[:S]
        if is_template:
            lab = self._tpl_label[i].clone()
        else:
            lab = self._labels[i].clone()
            shift = self.max_template_label if self.shifted[i] else 0
            if shift or not self.is_label:
                prepare(lab, t1w, normalize=not self.is_label, shift_by=shift, scratch=self._scratch("feed", feed_scratch_bytes(S)))
        return self._finish(index, is_template, x, lab)

    def _finish(self, index, is_template, x, lab):
        """the tail of a sample, in place on x {1,in,D,H,W} / lab {D,H,W} at model.dim (also patches.WindowFeed's): simulate_modality,
        augmentation, target"""
        D, H, W = self.size
        S = self.voxels
        t1w = x.view(-1)[:S]
        # simulate_modality (train.cpp:459-462), seed = seed_id as an unsigned int
        r = G.sim_to_struct(G.make_simulate_recipe((W, H, D), self.model.out_count if is_template else None, index))
        need = E.size_query(E.lib.unet_simulate_modality_scratch_bytes, C.byref(r))
        G.simulate(r, t1w, lab.view(-1) if is_template else None, self._scratch("sim", need))
        # visual_perception_augmentation(param.options, ..., param.is_label, model->dim, seed_id) (train.cpp:472)
        a = G.to_struct(G.make_recipe(self.options, (W, H, D), self.model.in_count, self.is_label, index, label_depth=D))
        G.augment(a, x.view(-1), lab.view(-1), self._scratch("aug", G.scratch_bytes(a)))
        t = target(lab, scratch=self._scratch("feed", feed_scratch_bytes(S)))
        return x, t.view(1, D, H, W)

    def test_set(self):
        """(test_in, test_out) of train.cpp:345-380 for Trainer.validate: the up to 2 largest templates, as read (no augmentation),
        the label normalized when out_count == 1, cast to int64"""
        D, H, W = self.size
        with torch.cuda.device(self.device):
            sc = self._scratch("feed", feed_scratch_bytes(self.voxels))
            test_in = [self._images[i].clone() for i in self._test]
            test_out = [target(self._labels[i], normalize=self.model.out_count == 1, scratch=sc).view(1, D, H, W) for i in self._test]
        return test_in, test_out
