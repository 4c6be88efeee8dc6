"""CPU: the host half of the template/subject training feed (train.cpp:259-401) -- the ABI the library exports for it, the sample
schedule against independent generators, the test-set order and the label-plan rules.  No device calls."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import feed as FD
from unet_studio_amd import qc as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, batch_size, n_template, n_subject, first, count)
SCHEDULES = [
    (0, 8, 3, 5, 0, 200),
    (1, 8, 3, 5, 37, 150),
    (12345, 4, 1, 1, 0, 64),
    (7, 32, 4, 0, 5, 100),          # templates only: every seed_id is a template
    (7, 32, 0, 6, 0, 100),          # subjects only
    (3, 6, 1, 0, 0, 40),            # one template: a (0, 0) distribution, still one draw per seed_id
    (3, 6, 2, 1, 11, 40),           # one subject: the (0, 0) distribution of the subjects
    (99, 5, 9, 2, 1000, 0),         # count 0
    (2**32 + 5, 16, 2, 3, 0, 50),   # a size_t seed: std::mt19937 takes it modulo 2^32
]


def test_unet_feed_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_feed.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(FD.EXPORTS) == {"unet_feed_scratch_bytes", "unet_feed_label_max", "unet_feed_prepare",
                                           "unet_feed_target", "unet_feed_schedule"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    assert U.TrainingFeed is FD.TrainingFeed


def test_scratch_bytes_and_argument_errors_need_no_device():
    assert FD.feed_scratch_bytes(1) == 256 + 4
    assert FD.feed_scratch_bytes(257) == 256 + 2 * 4
    assert FD.feed_scratch_bytes(128 ** 3) == 256 + 1024 * 4     # one float per block, grid capped at 1024
    with pytest.raises(U.UNetError, match="voxels must be positive"):
        FD.feed_scratch_bytes(0)
    with pytest.raises(U.UNetError, match="batch_size must be positive"):
        FD.schedule(0, 0, 1, 1, 0, 4)
    with pytest.raises(U.UNetError, match="no cases"):
        FD.schedule(0, 4, 0, 0, 0, 4)
    with pytest.raises(U.UNetError, match="must not be negative"):
        FD.schedule(0, 4, 1, 1, -1, 4)


_GEN_CPP = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
int main(int argc, char** argv) {
    size_t seed = std::strtoull(argv[1], 0, 10);
    int batch_size = std::atoi(argv[2]);
    size_t n_template = std::atoi(argv[3]), n_subject = std::atoi(argv[4]);
    size_t first = std::atoll(argv[5]), count = std::atoll(argv[6]);
    std::uniform_int_distribution<int> template_gen(0, std::max<int>(1, n_template) - 1);
    std::uniform_int_distribution<int> non_template_gen(0, std::max<int>(1, n_subject) - 1);
    std::mt19937 gen(seed);
    for (size_t seed_id = 0; seed_id < first + count; ++seed_id) {
        bool use_template = n_subject == 0 || seed_id % batch_size < n_template;
        int c = use_template ? template_gen(gen) : non_template_gen(gen);
        if (seed_id < first) continue;
        std::printf("%d %d\n", c, use_template ? 1 : 0);
    }
}
"""


@pytest.fixture(scope="module")
def std_generator(tmp_path_factory):
    """train.cpp:391-401 as a stand-alone program built with the host C++ compiler"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to build the independent generator"
    d = tmp_path_factory.mktemp("feed_gen")
    src, exe = d / "gen.cpp", d / "gen"
    src.write_text(_GEN_CPP)
    subprocess.check_call([cxx, "-O1", "-std=c++17", str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("seed,bs,nt,ns,first,count", SCHEDULES)
def test_schedule_equals_a_compiled_std_mt19937_program(std_generator, seed, bs, nt, ns, first, count):
    out = subprocess.check_output([std_generator] + [str(v) for v in (seed, bs, nt, ns, first, count)]).decode().split()
    want = np.array(out, dtype=np.int64).reshape(-1, 2)
    case, tpl = FD.schedule(seed, bs, nt, ns, first, count)
    assert len(case) == count and len(want) == count
    assert np.array_equal(case, want[:, 0]) and np.array_equal(tpl, want[:, 1].astype(bool))


def _mt19937(seed):
    """raw 32-bit outputs of std::mt19937(seed): numpy's MT19937 with the reference generator's init_genrand seeding"""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed) & 0xFFFFFFFF)
    while True:
        for v in bg.random_raw(256):
            yield int(v)


def _uniform_int(gen, n):
    """std::uniform_int_distribution<int>(0, n - 1) over a 32-bit engine (libstdc++: Lemire's multiply-shift with rejection); a
    one-value range still takes one draw"""
    product = next(gen) * n
    low = product & 0xFFFFFFFF
    if low < n:
        threshold = (2 ** 32 - n) % n
        while low < threshold:
            product = next(gen) * n
            low = product & 0xFFFFFFFF
    return product >> 32


@pytest.mark.parametrize("seed,bs,nt,ns,first,count", SCHEDULES)
def test_schedule_equals_a_python_restatement(seed, bs, nt, ns, first, count):
    gen = _mt19937(seed)
    want = []
    for seed_id in range(first + count):
        use_template = ns == 0 or seed_id % bs < nt
        c = _uniform_int(gen, max(1, nt if use_template else ns))
        if seed_id >= first:
            want.append((c, use_template))
    case, tpl = FD.schedule(seed, bs, nt, ns, first, count)
    assert [(int(c), bool(t)) for c, t in zip(case, tpl)] == want


def test_schedule_is_a_function_of_the_seed_id():
    # a feed resumed at epoch k (first = k * batch_size) sees the seed_ids a fresh one sees there
    full_c, full_t = FD.schedule(5, 8, 3, 4, 0, 160)
    for first in (1, 8, 64, 159):
        c, t = FD.schedule(5, 8, 3, 4, first, 160 - first)
        assert np.array_equal(c, full_c[first:]) and np.array_equal(t, full_t[first:])
    # with subjects, template samples are exactly the seed_ids with seed_id % batch_size < n_template
    assert np.array_equal(full_t, np.arange(160) % 8 < 3)
    assert full_c[full_t].max() < 3 and full_c[~full_t].max() < 4 and full_c.min() >= 0


def test_test_set_is_up_to_two_templates_by_descending_size_then_index(tmp_path):
    def arr(n):
        return np.zeros(n, np.float32)
    cases = [("a", "la", arr(10), arr(10), True),
             ("b", "lb", arr(30), arr(30), False),     # a subject: never in the test set
             ("c", "lc", arr(20), arr(20), True),
             ("d", "ld", arr(20), arr(20), True),     # ties with c on size: the larger index first
             ("e", "le", arr(5), arr(5), True)]
    assert FD.choose_test_cases(cases) == [3, 2]
    # an existing image file counts with its file size, not the array's
    f = tmp_path / "big.nii.gz"
    f.write_bytes(b"x" * 1000)
    cases[4] = (str(f), "le", arr(5), arr(5), True)
    assert FD.choose_test_cases(cases) == [4, 3]
    assert FD.choose_test_cases(cases[:2]) == [0]
    assert FD.choose_test_cases([cases[1]]) == []


def test_label_plan_with_device_maxima_follows_the_reader_thread_rules():
    # train.cpp:287-336: max template label over templates; a subject is shifted when its max < mtl and max + mtl < out_count
    maxima = {"t1": 3, "t2": 2, "s1": 1, "s2": 3, "s3": 2, "s4": 0}
    cases = [(n, n, None, n, n.startswith("t")) for n in ("t1", "s1", "t2", "s2", "s3", "s4", "s1")]
    mtl, shift = Q.label_plan(cases, 8, max_of=maxima.__getitem__)
    assert mtl == 3
    assert shift == [False, True, False, False, True, True, True]
    mtl, shift = Q.label_plan(cases, 5, max_of=maxima.__getitem__)
    assert shift == [False, True, False, False, False, True, True]      # 2 + 3 >= 5
    # no template label: the default of 5 regions
    with pytest.warns(UserWarning):
        mtl, shift = Q.label_plan([c for c in cases if not c[4]], 8, max_of=maxima.__getitem__)
    assert mtl == 5 and shift == [True, False, True, True, True]
    # the default reader is the host one, unchanged
    assert Q.label_plan([("i", "l", None, np.array([0, 2.7, -4.2], np.float32), True)], 8)[0] == 2
