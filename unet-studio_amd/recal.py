"""Recalibration on the device (include/unet_recal.h): temperature scaling of a model's level-0 logits, fitted and folded in.

  eval_betas   one fused pass over the level-0 logits of a volume, the truth label and an optional mask -> one int64 table: six head
               counts, then the negative log-likelihood under softmax(beta * x) and its slope in beta, summed over the valid voxels
               as integers, for up to 8 candidate beta at once
  sums         that table as exact Python numbers
  Solver       brackets the minimiser of the (convex) likelihood from those tables, 8 candidates a round, in u = log2 beta: host
               arithmetic on integers
  fit          Solver over a set of cases: per round the cases accumulate on the device and the table is read back once
  head_is_bare_conv, fold   beta * logits equals the level-0 head's weight and bias times beta when that head is a bare conv: the
               recalibrated model is an ordinary model, and every consumer of its probabilities sees the new ones

A term (nll or g of one voxel and one candidate) is clamped to +-4096 and added as llrintf(term * 2^20), so only integers are summed
and a table does not depend on the order of the sum.  The reference has no counterpart, so these are this project's definitions
(parity NOT pinned); tests/test_recal_host.py restates them in fp64."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_recal_scratch_bytes", C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_recal_eval", C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int,
       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_recal.h declares
EXPORTS = ["unet_recal_scratch_bytes", "unet_recal_eval"]

MAX_CLASSES, MAX_BETAS, HEAD, TABLE_LEN = 256, 8, 6, 22
SCALE_BITS, CLAMP = 20, 4096
CACHE, UNIT, BLOCK_UNITS, GRID_UNITS = 8, 4, 256, 131072
# head
VALID, BAD, INVALID_LABEL, SKIPPED, IMPOSSIBLE, SATURATED = range(6)


# ---- the device call ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(out_c, voxels):
    """bytes of the scratch of an eval_betas call: the running table, nothing per voxel"""
    return E.size_query(E.lib.unet_recal_scratch_bytes, int(out_c), int(voxels))


def _dev(a, dtype, name, device=None):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == dtype and a.is_contiguous()):
        raise UNetError("recal: %s must be a contiguous %s device tensor" % (name, str(dtype).replace("torch.", "")))
    if device is not None and a.device != device:
        raise UNetError("recal: %s is on %s, the logits on %s" % (name, a.device, device))
    return a


def eval_betas(logits, label, betas, mask=None, out=None, accumulate=False, scratch=None):
    """unet_recal_eval on the current stream.  logits: {C, d, h, w} or {1, C, d, h, w} (any {C, ...}), a contiguous fp32 device
    tensor; label: fp32, one value per voxel; betas: 1 to 8 finite positive numbers, passed as float32; mask: uint8 per voxel or None
    (0: the voxel is skipped); out: the int64 table of 22 entries to write (or, with accumulate, to add to).  Returns the device
    table (sums reads it).  No host synchronisation."""
    _dev(logits, torch.float32, "logits")
    if logits.dim() == 5 and logits.shape[0] == 1:
        logits = logits[0]
    if logits.dim() < 2:
        raise UNetError("recal: logits must be {C, ...}, got %s" % (tuple(logits.shape),))
    dev = logits.device
    out_c = int(logits.shape[0])
    voxels = logits.numel() // max(out_c, 1)
    need = scratch_bytes(out_c, voxels)                 # the class / size checks first
    _dev(label, torch.float32, "label", dev)
    if label.numel() != voxels:
        raise UNetError("recal: label holds %d voxels, the logits %d" % (label.numel(), voxels))
    if mask is not None:
        _dev(mask, torch.uint8, "mask", dev)
        if mask.numel() != voxels:
            raise UNetError("recal: mask holds %d voxels, the logits %d" % (mask.numel(), voxels))
    try:
        values = [float(b) for b in betas]
    except (TypeError, ValueError):
        raise UNetError("recal: betas must be a sequence of numbers, got %r" % (betas,))
    if out is None:
        if accumulate:
            raise UNetError("recal: accumulate needs the table to add to (out)")
        out = torch.empty(TABLE_LEN, dtype=torch.int64, device=dev)
    else:
        _dev(out, torch.int64, "out", dev)
        if out.numel() != TABLE_LEN:
            raise UNetError("recal: out must hold %d entries, got %d" % (TABLE_LEN, out.numel()))
    scratch = E.scratch(scratch, need, dev)
    arr = (C.c_float * max(1, len(values)))(*values)
    E.check(E.lib.unet_recal_eval(logits.data_ptr(), out_c, voxels, label.data_ptr(), mask.data_ptr() if mask is not None else None, arr,
                                  len(values), int(bool(accumulate)), out.data_ptr(), scratch.data_ptr(), scratch.nbytes, E.stream(logits)))
    return out


# ---- host arithmetic on the tables: Python ints ---------------------------------------------------------------------------------------
def _ints(table):
    if torch.is_tensor(table):
        table = table.cpu().numpy()
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.size != TABLE_LEN:
        raise UNetError("recal: a table holds %d integers, got %s of %d" % (TABLE_LEN, t.dtype, t.size))
    return [int(v) for v in t.reshape(-1)]


def sums(table, n_betas):
    """-> (head, nll, g): head the six counts as ints, nll and g the sums of the first n_betas candidates as exact Fractions
    (integer / 2^20)"""
    n_betas = int(n_betas)
    if not 1 <= n_betas <= MAX_BETAS:
        raise UNetError("recal.sums: n_betas must be in [1, %d], got %d" % (MAX_BETAS, n_betas))
    t = _ints(table)
    one = 1 << SCALE_BITS
    return (t[:HEAD], [Fraction(t[HEAD + 2 * k], one) for k in range(n_betas)], [Fraction(t[HEAD + 2 * k + 1], one) for k in range(n_betas)])


class Solver:
    """The minimiser of the summed nll over beta, bracketed in u = log2 beta from the sign of G = sum g (increasing in beta).
    Round 1 sends 8 candidates evenly over [u_lo, u_hi], ends included; the bracket is the adjacent pair with G_lo < 0 <= G_hi.  G >= 0
    at u_lo ends the search with beta = 2^u_lo and at_bound -1, G < 0 at u_hi with beta = 2^u_hi and at_bound +1.  Every later round
    sends 8 interior points evenly into the bracket, which therefore is (u_hi - u_lo) / 7 / 9^(rounds - 1) octaves wide at the end.
    The candidates are float32, and those exact values are the ones interpolated between."""

    def __init__(self, u_lo=-4.0, u_hi=4.0, rounds=3):
        u_lo, u_hi = float(u_lo), float(u_hi)
        if not (math.isfinite(u_lo) and math.isfinite(u_hi) and -100.0 <= u_lo < u_hi <= 100.0):
            raise UNetError("recal.Solver: u_lo < u_hi within [-100, 100] octaves, got %r, %r" % (u_lo, u_hi))
        if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 1:
            raise UNetError("recal.Solver: rounds must be a positive integer, got %r" % (rounds,))
        self.u_lo, self.u_hi, self.rounds = u_lo, u_hi, rounds
        self.round, self.at_bound = 0, 0
        self.lo = self.hi = None         # (u, beta as sent, G) of the bracket's ends
        self.valid = 0

    def width(self, rounds=None):
        """octaves between the bracket's ends after `rounds` rounds (all of them by default) of a search that met no bound"""
        rounds = self.rounds if rounds is None else int(rounds)
        return (self.u_hi - self.u_lo) / 7.0 / 9.0 ** (rounds - 1)

    @property
    def done(self):
        return self.at_bound != 0 or self.round >= self.rounds

    def _us(self):
        if self.round == 0:
            return [self.u_lo + (self.u_hi - self.u_lo) * k / 7.0 for k in range(8)]
        a, b = self.lo[0], self.hi[0]
        return [a + (b - a) * (k + 1) / 9.0 for k in range(8)]

    def betas(self):
        """this round's 8 candidates, float32"""
        if self.done:
            raise UNetError("recal.Solver: the rounds are over")
        return [np.float32(2.0 ** u) for u in self._us()]

    def update(self, table):
        """narrows the bracket with the table of this round's candidates (betas())"""
        us, sent = self._us(), self.betas()
        head, _, g = sums(table, MAX_BETAS)
        if head[VALID] <= 0:
            raise UNetError("recal.Solver: the table holds no valid voxel")
        self.valid = head[VALID]
        pts = [(u, float(b), gk) for u, b, gk in zip(us, sent, g)]
        if self.round == 0:
            if pts[0][2] >= 0:
                self.at_bound, self.lo, self.hi = -1, pts[0], pts[0]
            elif pts[-1][2] < 0:
                self.at_bound, self.lo, self.hi = 1, pts[-1], pts[-1]
        else:
            pts = [self.lo] + pts + [self.hi]
        if not self.at_bound:
            k = next(i for i, p in enumerate(pts) if p[2] >= 0)   # the first candidate at or above the zero: k >= 1
            self.lo, self.hi = pts[k - 1], pts[k]
        self.round += 1

    def result(self):
        """-> dict: beta, temperature = 1 / beta, bracket = (beta_lo, beta_hi), at_bound in {-1, 0, +1}, rounds (those run)"""
        if self.lo is None:
            raise UNetError("recal.Solver: no round has run")
        (_, b0, g0), (_, b1, g1) = self.lo, self.hi
        beta = b0 if self.at_bound or g1 == g0 else float(b0 - g0 * (Fraction(b1) - Fraction(b0)) / (g1 - g0))
        return {"beta": beta, "temperature": 1.0 / beta, "bracket": (b0, b1), "at_bound": self.at_bound, "rounds": self.round}


def fit(batches, mask=None, solver=None):
    """Fits beta over a set of cases.  batches: a callable that yields (logits, label) or (logits, label, mask) per case, as
    eval_betas takes them; it is called once per round, so the caller re-runs its forwards.  mask: a uint8 device tensor for the
    cases that yield none of their own.  Per round the cases accumulate into one device table, which is read back once: no other host
    synchronisation.  -> Solver.result(), with `valid` (the voxels of a round) added."""
    solver = Solver() if solver is None else solver
    table = scratch = None
    while not solver.done:
        betas = solver.betas()
        n = 0
        for case in batches():
            logits, label = case[0], case[1]
            m = case[2] if len(case) > 2 and case[2] is not None else mask
            if table is None:
                table = torch.empty(TABLE_LEN, dtype=torch.int64, device=logits.device)
            table = eval_betas(logits, label, betas, mask=m, out=table, accumulate=n > 0, scratch=scratch)
            n += 1
        if not n:
            raise UNetError("recal.fit: batches yielded no case")
        solver.update(table.cpu())
    r = solver.result()
    r["valid"] = solver.valid
    return r


# ---- folding beta into the level-0 head ---------------------------------------------------------------------------------------------
def head_token(architecture):
    """the level-0 head's token: the last token of the DSL's last line (unet.cpp:138,148-153)"""
    lines = [l.strip() for l in str(architecture).replace("\r", "").split("\n") if l.strip()]
    if not lines:
        raise UNetError("recal: the architecture is empty")
    return lines[-1].split("+")[-1]


def head_is_bare_conv(architecture):
    """whether the level-0 head is a single conv<N> with only ks / stride parts: no norm, no activation, nothing else"""
    keys = []
    for part in head_token(architecture).split(","):
        digits = [i for i, ch in enumerate(part) if ch.isdigit()]
        keys.append((part[:digits[0]] if digits else part, part[digits[0]:] if digits else ""))
    if not keys or keys[0][0] != "conv" or not keys[0][1].isdigit():
        return False
    return all(k in ("ks", "stride") and v.isdigit() for k, v in keys[1:]) and len({k for k, _ in keys}) == len(keys)


def fold(model, beta):
    """Multiplies the weight and the bias of the model's level-0 head by float32(beta), in place on the device: the model's level-0
    logits become beta times what they were, for every consumer.  Refuses (UNetError naming the token) unless the head is a bare
    conv and the parameter names show exactly a weight and a bias for output0; the coarse heads are not touched."""
    token = head_token(model.architecture)
    if not head_is_bare_conv(model.architecture):
        raise UNetError("recal.fold: the level-0 head %r is not a bare conv (conv<N> with only ks / stride): beta cannot be folded in" % token)
    names = list(model._probe.param_names)
    mine = [i for i, nm in enumerate(names) if nm.startswith("output0.")]
    if [names[i] for i in mine] != ["output0.0.weight", "output0.0.bias"]:
        raise UNetError("recal.fold: the level-0 head %r must own exactly output0.0.weight and output0.0.bias, the model has %s"
                        % (token, [names[i] for i in mine]))
    b = float(np.float32(beta))
    if not (math.isfinite(b) and b > 0.0):
        raise UNetError("recal.fold: beta must be finite and positive, got %r" % (beta,))
    with torch.no_grad():
        for i in mine:
            model._params[i].mul_(b)
    model._params_version += 1                         # the filter packs are stale, as after load_parameters
    return b


# ---- the report of qc.recalibration_qc ---------------------------------------------------------------------------------------------------
REPORT_COLUMNS = ("voxels", "nll_before", "nll_after")
REPORT_TOTAL_COLUMNS = ("beta", "temperature", "beta_lo", "beta_hi", "at_bound", "impossible", "saturated")


def report_path(model_path):
    d, f = os.path.split(model_path)
    return os.path.join(d, os.path.splitext(f)[0] + ".recalibration_report.tsv")


def mean_nll(table, n_betas=2):
    """-> (valid, [mean nll per valid voxel of each candidate as float]); NaN without voxels"""
    head, nll, _ = sums(table, n_betas)
    return head[VALID], [float(v / head[VALID]) if head[VALID] else float("nan") for v in nll]


def format_report(rows, fitted):
    """the report text; rows: (image, label, table) with table that of the closing pass, candidates (1.0, beta), or None for a case
    that took no part (a shifted label): N/A.  fitted: the dict of fit with `table` the total of the closing pass, or None when no
    case took part.  The case rows leave the columns of the fit empty; the last row, named total, has an empty ground_truth."""
    lines = ["image\tground_truth\t" + "\t".join(REPORT_COLUMNS + REPORT_TOTAL_COLUMNS)]

    def cols(table):
        if table is None:
            return ["N/A"] * len(REPORT_COLUMNS)
        valid, (before, after) = mean_nll(table)
        return ["%d" % valid, "%.9g" % before, "%.9g" % after]

    for image, label, table in rows:
        lines.append("\t".join([os.path.basename(image), os.path.basename(label)] + cols(table) + [""] * len(REPORT_TOTAL_COLUMNS)))
    if fitted is None:
        lines.append("\t".join(["total", ""] + ["N/A"] * (len(REPORT_COLUMNS) + len(REPORT_TOTAL_COLUMNS))))
    else:
        head = sums(fitted["table"], 2)[0]
        lines.append("\t".join(["total", ""] + cols(fitted["table"]) + ["%.9g" % fitted["beta"], "%.9g" % fitted["temperature"],
                                "%.9g" % fitted["bracket"][0], "%.9g" % fitted["bracket"][1], "%d" % fitted["at_bound"],
                                "%d" % head[IMPOSSIBLE], "%d" % head[SATURATED]]))
    return "\n".join(lines) + "\n"
