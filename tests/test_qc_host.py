"""CPU: the host half of quality control (qc.cpp:164-376) -- the ABI the library exports for it, the label-information rules, the
mapping of the kernel's bins onto per-class statistics, and the bytes of the report.  No device calls."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import qc as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unet_qc_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_qc.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(Q.EXPORTS) == {"unet_qc_scratch_bytes", "unet_qc_counts"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name


def test_scratch_bytes_and_argument_errors_need_no_device():
    assert Q.qc_scratch_bytes(6, 192 * 224 * 192) == 2048 * 2 * 6 * 4        # one uint32 column per block, grid capped at 2048
    assert Q.qc_scratch_bytes(6, 1) == 1 * 2 * 6 * 4
    assert Q.qc_scratch_bytes(130, 4099, 129) == 17 * 2 * 2 * 4               # C' = 2
    with pytest.raises(U.UNetError, match="^invalid collapse_before$"):
        Q.qc_scratch_bytes(6, 100, 6)
    with pytest.raises(U.UNetError, match="^invalid collapse_before$"):
        Q.qc_scratch_bytes(6, 100, -1)
    with pytest.raises(U.UNetError, match="voxels must be positive"):
        Q.qc_scratch_bytes(6, 0)


def _case(name, label_name, max_label, is_template, n=8):
    lab = np.zeros(n, np.float32)
    lab[1] = max_label
    return (name, label_name, None, lab, is_template)


def test_label_plan_default_template_label_and_shift_rule():
    # no template: max_template_label 5, with the reference's warning
    cases = [_case("a", "la", 2, False), _case("b", "lb", 6, False)]
    with pytest.warns(UserWarning, match="no template label found; use default 5"):
        mtl, shift = Q.label_plan(cases, 12)
    assert mtl == 5 and shift == [True, False]          # 2 < 5 and 2 + 5 < 12; 6 is not below 5
    # templates set it (the largest), and are never shifted; max_label + mtl must stay below out_count
    cases = [_case("t1", "lt1", 3, True), _case("t2", "lt2", 4, True), _case("s1", "ls1", 2, False), _case("s2", "ls2", 3, False),
             _case("s3", "ls3", 4, False)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mtl, shift = Q.label_plan(cases, 7)
    assert mtl == 4 and shift == [False, False, True, False, False]   # 2 + 4 < 7; 3 + 4 == 7 is not below
    assert Q.case_settings(True, mtl) == (5, 4) and Q.case_settings(False, mtl) == (0, 0)   # collapse_before = mtl + 1, shift_by = mtl
    # the label information is read once per label name: a second case with the same label name reuses the first one's
    cases = [_case("t", "lt", 3, True), _case("x", "same", 1, False), _case("y", "same", 9, False)]
    mtl, shift = Q.label_plan(cases, 9)
    assert mtl == 3 and shift == [False, True, True]
    # labels are read as int: truncation toward zero
    assert Q.max_label_of(np.array([0.0, 2.7, -0.5], np.float32)) == 2


def test_stats_from_counts_without_and_with_collapse():
    stats, overall = Q.stats_from_counts([10, 20, 30, 1, 2, 3], 3)
    assert stats == [Q.QcStat(10, 1), Q.QcStat(20, 2), Q.QcStat(30, 3)] and overall == Q.QcStat(60, 6)
    # out_count 6, collapse_before 3: C' = 4 bins [merged 0..2, 3, 4, 5]; bin 0 only in overall, stats[0..3) stay empty
    stats, overall = Q.stats_from_counts([100, 7, 8, 9, 5, 1, 0, 2], 6, 3)
    assert stats == [Q.QcStat()] * 3 + [Q.QcStat(7, 1), Q.QcStat(8, 0), Q.QcStat(9, 2)]
    assert overall == Q.QcStat(124, 8)
    assert Q.QcStat().ratio() == 0.0 and Q.QcStat(3, 1).ratio() == 1 / 3
    s = Q.QcStat(1, 1)
    s += Q.QcStat(2, 0)
    assert s == Q.QcStat(3, 1)
    with pytest.raises(U.UNetError):
        Q.stats_from_counts([1, 2, 3], 3)


def test_report_bytes():
    rows = [("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_label.nii.gz",
             [Q.QcStat(3, 1), Q.QcStat(0, 0), Q.QcStat(7, 7)], Q.QcStat(10, 8), 0),
            ("t2.nii.gz", "t2_label.nii.gz", [Q.QcStat(), Q.QcStat(), Q.QcStat(9, 2)], Q.QcStat(40, 3), 2)]
    text = Q.format_report(3, rows)
    assert text == ("image\tground_truth\twrong_ratio\twrong_ratio0\twrong_ratio1\twrong_ratio2\n"
                    "sub-01_T1w.nii.gz\tsub-01_label.nii.gz\t0.8\t0.333333333\t0\t1\n"
                    "t2.nii.gz\tt2_label.nii.gz\t0.075\tN/A\tN/A\t0.222222222\n")
    assert "%.9g" % (1 / 7) == "0.142857143"     # std::setprecision(9)


def test_report_goes_through_tmp_and_replaces_an_existing_one(tmp_path):
    model = str(tmp_path / "net.v2.nz")
    report = str(tmp_path / "net.v2.error_report.tsv")
    assert Q.report_path(model) == report
    with open(report, "w") as f:
        f.write("old report, longer than the new one " * 10)
    rows = [("a.nii.gz", "b.nii.gz", [Q.QcStat(2, 1), Q.QcStat(2, 0)], Q.QcStat(4, 1), 0)]
    assert Q.write_report(model, 2, rows) == (0, report)
    assert open(report, "rb").read() == Q.format_report(2, rows).encode()
    assert sorted(os.listdir(tmp_path)) == ["net.v2.error_report.tsv"]     # no .tmp left behind
