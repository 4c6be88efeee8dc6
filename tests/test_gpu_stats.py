"""GPU: the per-region intensity statistics on the device (include/unet_stats.h) -- moments, hist and quantiles under IMPL_LDS,
IMPL_GLOBAL and the default against moments_ref, hist_ref and quantiles_ref (the restatements of test_stats_host.py), every case
twice into garbage-filled outputs with guard words on both sides.  Every comparison is exact equality of bytes.  The voxel counts come
from the kernel's own constants (a thread's unit, a wave's stretch of units, the capped grid's stride)."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import stats as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_stats_host import codes, hist_ref, moments_ref, quantiles_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAN, INF = float("nan"), float("inf")
IMPLS = (S.IMPL_LDS, S.IMPL_GLOBAL, S.IMPL_DEFAULT)
BOTH = (S.IMPL_LDS, S.IMPL_GLOBAL)
G = 64                                                             # guard words on each side of an output
GUARD = -0x5A3C5A3C
BLOCK = S.UNIT * S.WAVE_UNITS * 8                                  # the voxels a block of 8 waves takes at once
MID = BLOCK + 4 * S.UNIT * S.WAVE_UNITS + 5                        # more than one block, a tail that is no whole unit


def dev_map(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(dtype)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, dtype, rep):
    """a buffer of G + n + G words: guards outside, garbage inside; -> (buffer, the view a call writes)"""
    buf = torch.full((n + 2 * G,), GUARD, dtype=dtype, device=DEV)
    buf[G:G + n] = 0x7B7B7B7B if rep == 0 else -3
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:G] == GUARD).all() and (b[G + n:] == GUARD).all()


def check(labels, image, L, lo, hi, pm=(0, 500, 1000), impls=IMPLS, calls=("moments", "hist", "quantiles"), ldtype=torch.uint16):
    """the calls under every impl, twice each, against the restatements; -> the restatements' answers"""
    image = np.ascontiguousarray(image, F).reshape(-1)
    lab = None if labels is None else dev_map(labels, ldtype)
    img = torch.from_numpy(image).to(DEV)
    ref = {"moments": lambda: moments_ref(labels, image, L, lo, hi), "hist": lambda: hist_ref(labels, image, L, lo, hi),
           "quantiles": lambda: quantiles_ref(labels, image, L, lo, hi, pm)}
    cols = {"moments": 10, "hist": 256, "quantiles": len(pm)}
    want = {}
    for call in calls:
        want[call] = ref[call]()
        n, dtype = (L + 1) * cols[call], torch.int32 if call == "quantiles" else torch.int64
        for impl in impls:
            for rep in range(2):
                buf, out = guarded(n, dtype, rep)
                if call == "quantiles":
                    got = S.quantiles(lab, img, L, lo, hi, pm, impl=impl, out=out)
                else:
                    got = getattr(S, call)(lab, img, L, lo, hi, impl=impl, out=out)
                assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (L + 1, cols[call])
                g = got.cpu().numpy()
                assert same(g, want[call]), (call, impl, rep, np.argwhere(g != want[call])[:5].tolist())
                assert guards_intact(buf, n)
    if "moments" in want:
        assert int(want["moments"][:, :2].sum()) == image.size
        if "hist" in want:
            assert (want["hist"].sum(1) == want["moments"][:, 0]).all()
    return want


# ---- images and maps -----------------------------------------------------------------------------------------------------------------
def noise(rng, n, lo, hi):
    """values a little beyond both ends, the special ones planted"""
    v = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n).astype(F)
    for value, share in ((F(lo), 0.03), (F(hi), 0.03), (np.nextafter(F(lo), F(-INF)), 0.01), (np.nextafter(F(lo), F(INF)), 0.01),
                         (np.nextafter(F(hi), F(-INF)), 0.01), (np.nextafter(F(hi), F(INF)), 0.01), (F(NAN), 0.03), (F(INF), 0.01),
                         (F(-INF), 0.01), (F(-0.0), 0.01)):
        v[rng.random(n) < share] = value
    return v


def runs(rng, n, ids, mean_run):
    """the ids in runs of random length around mean_run"""
    k = 2 * n // mean_run + 2
    out = np.repeat(rng.choice(np.asarray(ids), k), rng.integers(1, 2 * mean_run, k))
    return np.resize(out, n)                                        # cut, or repeated should the lengths have come out short


# ---- the voxel counts ------------------------------------------------------------------------------------------------------------------
STRETCH = S.UNIT * S.WAVE_UNITS
COUNTS = [1, S.UNIT - 1, S.UNIT, S.UNIT + 1, STRETCH - 1, STRETCH, STRETCH + 1, BLOCK + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_voxel_counts_around_a_unit_a_stretch_and_a_block(n):
    rng = np.random.default_rng(n)
    for L, ldtype in ((5, torch.uint8), (300, torch.uint16)):
        labels = runs(rng, n, range(L + 1), 6)
        check(labels, noise(rng, n, -2.0, 5.0), L, -2.0, 5.0, ldtype=ldtype)
    check(None, noise(rng, n, 0.0, 1.0), 0, 0.0, 1.0, pm=(500,))


def test_the_capped_grid_strides_a_second_time():
    n = S.GRID_UNITS * S.UNIT + 2 * S.UNIT + 3
    assert S.GRID_UNITS * S.UNIT < n <= 1 << 25
    rng = np.random.default_rng(1)
    image = (rng.integers(0, 1000, n) / F(1000)).astype(F)          # ties everywhere
    image[-7:] = [NAN, 0.5, 2.0, -1.0, 0.25, 0.75, 1.0]             # the second stride's voxels count
    labels = np.zeros(n, np.int64)
    labels[n // 2:] = 1
    labels[-5:] = [0, 1, 1, 0, 1]
    want = check(labels, image, 1, 0.0, 1.0, pm=(500,), impls=BOTH, calls=("moments", "quantiles"), ldtype=torch.uint8)
    assert want["moments"][1, 1] == 1 and want["moments"][0, 3] == 1 and want["moments"][1, 2] == 1


# ---- the label maps --------------------------------------------------------------------------------------------------------------------
def test_no_map_one_label_and_the_background():
    rng = np.random.default_rng(2)
    v = noise(rng, MID, 0.0, 1.0)
    check(None, v, 0, 0.0, 1.0, pm=(0, 1, 250, 500, 750, 999, 1000, 500))
    check(np.ones(MID, np.int64), v, 1, 0.0, 1.0, ldtype=torch.uint8)                  # row 0 empty
    check(np.zeros(MID, np.int64), v, 1, 0.0, 1.0)                                     # row 1 empty


def test_a_uint8_map_with_255_labels_and_more_labels_than_it_can_hold():
    rng = np.random.default_rng(3)
    v = noise(rng, MID, -1000.0, 3000.0)
    labels = runs(rng, MID, range(256), 40)
    check(labels, v, 255, -1000.0, 3000.0, ldtype=torch.uint8)
    check(labels, v, 2035, -1000.0, 3000.0, ldtype=torch.uint8)
    want = check(labels, v, 100, -1000.0, 3000.0, ldtype=torch.uint8)                  # the values above 100 read 0
    assert want["moments"][0, 0] + want["moments"][0, 1] > MID // 2


def test_sparse_ids_up_to_2035():
    rng = np.random.default_rng(4)
    ids = [0, 1, 2, 77, S.LDS_ROWS - 1, S.LDS_ROWS, S.LDS_ROWS + 1, 1999, 2035]
    want = check(runs(rng, MID, ids, 300), noise(rng, MID, 0.0, 100.0), 2035, 0.0, 100.0)
    assert (want["moments"][ids, 0] > 0).all() and (want["moments"][:, 0] > 0).sum() == len(ids)


def test_the_most_labels_each_call_takes():
    rng = np.random.default_rng(5)
    v = noise(rng, MID, 0.0, 1.0)
    check(rng.integers(0, 65536, MID), v, 65535, 0.0, 1.0, calls=("moments",))
    check(runs(rng, MID, [0, 1, 65534, 65535], 50), v, 65535, 0.0, 1.0, calls=("moments",))
    check(rng.integers(0, 4096, MID), v, 4095, 0.0, 1.0, calls=("hist", "quantiles"), pm=(500, 900))
    img, lab = torch.from_numpy(v).to(DEV), dev_map(rng.integers(0, 4097, MID), torch.uint16)
    for fn in (S.hist, S.quantiles):
        with pytest.raises(U.UNetError, match="n_labels"):
            fn(lab, img, 4096, 0.0, 1.0)


def test_a_stretch_with_more_distinct_labels_than_the_slot_cache_holds():
    """every block meets far more labels than it has slots (a slot holds SLOT_BINS bins of one row; with eight quantiles the fine
    rows are many more still): the LDS path's updates that find no slot go to global memory"""
    rng = np.random.default_rng(6)
    L = 4095
    labels = runs(rng, MID, range(L + 1), 3)
    assert np.unique(labels[:BLOCK]).size > 4 * S.LDS_SLOTS
    check(labels, noise(rng, MID, 0.0, 1.0), L, 0.0, 1.0, pm=(0, 125, 250, 375, 500, 625, 750, 1000))
    # one more row than the slots hold when an image fills every bin of every row
    full = S.LDS_SLOTS * S.SLOT_BINS // S.HIST_BINS
    labels = runs(rng, MID, range(full + 1), 5)
    check(labels, noise(rng, MID, 0.0, 1.0), full, 0.0, 1.0, pm=(500,))


@pytest.mark.parametrize("nbytes", [1, 2])
def test_a_map_at_an_odd_address_and_an_image_off_16_bytes(nbytes):
    """the raw calls: the map one byte off (a uint16 map at an odd address), the image 4 bytes off a 16-byte boundary, the scratch off
    alignment too: the paths that read element by element"""
    rng = np.random.default_rng(20 + nbytes)
    n, L, lo, hi = MID, S.LDS_ROWS + 1 if nbytes == 2 else 200, -3.25, 17.5
    labels = runs(rng, n, range(min(L, 255 if nbytes == 1 else L) + 3), 20)
    image = noise(rng, n, lo, hi)
    raw = np.frombuffer(labels.astype(np.uint8 if nbytes == 1 else np.uint16).tobytes(), np.uint8)
    lbuf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    lbuf[1:1 + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
    ibuf = torch.full((n + 8,), NAN, dtype=torch.float32, device=DEV)
    ibuf[1:1 + n] = torch.from_numpy(image).to(DEV)
    lptr, iptr = lbuf.data_ptr() + 1, ibuf.data_ptr() + 4
    assert lptr % 2 == 1 and iptr % 16 == 4
    pm = (0, 500, 1000, 37)
    need = S.stats_scratch_bytes(n, L, len(pm))
    scratch = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = U.engine.lib
    want_m, want_h, want_q = moments_ref(labels, image, L, lo, hi), hist_ref(labels, image, L, lo, hi), quantiles_ref(labels, image, L, lo, hi, pm)
    for impl in IMPLS:
        for rep in range(2):
            buf, out = guarded((L + 1) * 10, torch.int64, rep)
            U.engine.check(lib.unet_stats_moments(lptr, nbytes, iptr, n, L, lo, hi, out.data_ptr(), impl, scratch.data_ptr() + 3, need, stream))
            assert same(out.cpu().numpy().reshape(L + 1, 10), want_m) and guards_intact(buf, (L + 1) * 10)
            buf, out = guarded((L + 1) * 256, torch.int64, rep)
            U.engine.check(lib.unet_stats_hist(lptr, nbytes, iptr, n, L, lo, hi, out.data_ptr(), impl, scratch.data_ptr() + 3, need, stream))
            assert same(out.cpu().numpy().reshape(L + 1, 256), want_h) and guards_intact(buf, (L + 1) * 256)
            buf, out = guarded((L + 1) * len(pm), torch.int32, rep)
            U.engine.check(lib.unet_stats_quantiles(lptr, nbytes, iptr, n, L, lo, hi, (ctypes.c_int * len(pm))(*pm), len(pm), out.data_ptr(),
                                                    impl, scratch.data_ptr() + 3, need, stream))
            assert same(out.cpu().numpy().reshape(L + 1, len(pm)), want_q) and guards_intact(buf, (L + 1) * len(pm))


# ---- the values ------------------------------------------------------------------------------------------------------------------------
def test_the_special_values_each_on_its_own_and_together():
    lo, hi = -2.0, 6.0
    special = [NAN, INF, -INF, -0.0, 0.0, lo, hi, np.nextafter(F(lo), F(-INF)), np.nextafter(F(lo), F(INF)),
               np.nextafter(F(hi), F(-INF)), np.nextafter(F(hi), F(INF))]
    v = np.asarray(special, F)
    labels = np.arange(1, v.size + 1)                               # a row each: n = 1, or 0 for the NaN
    want = check(labels, v, v.size + 1, lo, hi)                     # the last row stays empty
    m = want["moments"]
    assert m[1, :2].tolist() == [0, 1] and m[1, 6:].tolist() == [65536, -1, 0xFFFFFFFF, -1] and want["quantiles"][1].tolist() == [-1] * 3
    assert m[2, 3] == 1 and m[2, 7] == 65535 and m[3, 2] == 1 and m[3, 6] == 0                 # the infinities clamp to a code
    assert m[4, 8] == 0x7FFFFFFF and m[5, 8] == 0x80000000 and m[4, 4] == m[5, 4] == 16384     # -0.0 and 0.0: one code, two keys
    assert m[6, 2:5].tolist() == [0, 0, 0] and m[7, 2:5].tolist() == [0, 0, 65535]             # lo and hi are in range
    assert m[8, 2] == 1 and m[9, 2] == 0 and m[10, 3] == 0 and m[11, 3] == 1
    rng = np.random.default_rng(7)
    check(runs(rng, MID, range(4), 100), np.asarray(special, F)[rng.integers(0, len(special), MID)], 3, lo, hi)
    check(None, np.full(MID, NAN, F), 0, lo, hi)                    # nothing but NaNs: an empty row


def test_a_constant_image_and_a_mask_as_float():
    rng = np.random.default_rng(8)
    labels = runs(rng, MID, range(401), 500)
    want = check(labels, np.full(MID, 0.75, F), 400, 0.0, 1.0)
    some = want["moments"][:, 0] > 0
    assert (want["quantiles"][some] == 49152).all() and (want["moments"][some, 6] == want["moments"][some, 7]).all()
    mask = (runs(rng, MID, [0, 1], 200) > 0).astype(F)
    want = check(labels, mask, 400, 0.0, 1.0)
    assert set(np.unique(want["quantiles"])) <= {-1, 0, 65535}
    check(None, mask, 0, 0.0, 1.0, pm=(0, 499, 500, 501, 1000))


def test_the_coarse_bin_edge_and_a_rank_inside_a_long_tie():
    # lo 0, hi 2: a code is 1 / 32768 wide; codes 255 and 256 are the last of coarse bin 0 and the first of bin 1
    rng = np.random.default_rng(9)
    a, b = F(255.5 / 32768), F(256.5 / 32768)
    assert codes([a, b], 0, 2).tolist() == [255, 256]
    v = np.where(rng.random(MID) < 0.5, a, b).astype(F)
    labels = runs(rng, MID, range(6), 50)
    want = check(labels, v, 5, 0.0, 2.0, pm=(0, 499, 500, 501, 1000))
    assert set(np.unique(want["quantiles"])) == {255, 256} and (want["hist"][:, :2] > 0).all() and want["hist"][:, 2:].sum() == 0
    # a long tie in the middle of a row: most ranks fall inside it
    v = noise(rng, MID, 0.0, 2.0)
    v[rng.random(MID) < 0.6] = F(1.2345)
    want = check(labels, v, 5, 0.0, 2.0, pm=(200, 300, 500, 700, 800))
    tie = int(codes([F(1.2345)], 0, 2)[0])
    assert (want["quantiles"][:, 1:4] == tie).all()


# ---- the quantiles ---------------------------------------------------------------------------------------------------------------------
def test_rows_of_zero_one_and_two_voxels_and_every_shape_of_permille():
    rng = np.random.default_rng(10)
    n = MID
    labels = np.full(n, 5, np.int64)
    labels[[3, 4000, 4001, n - 1, 10, 11]] = [1, 2, 2, 3, 4, 4]     # row 1: n = 1; row 2: n = 2; row 3: a NaN only; row 4: a NaN and a value
    v = noise(rng, n, 0.0, 1.0)
    v[[3, 4000, 4001, n - 1, 10, 11]] = [0.3, 0.9, 0.1, NAN, NAN, 0.6]
    for pm in ((500,), (0,), (1000,), (0, 500, 1000), (500, 500), (250, 250, 750, 750, 250, 0, 1000, 500), (500, 501, 502, 503)):
        want = check(labels, v, 6, 0.0, 1.0, pm=pm, calls=("quantiles",), impls=BOTH)["quantiles"]
        assert (want[[0, 3, 6]] == -1).all() and (want[1] == codes([F(0.3)], 0, 1)[0]).all() and (want[4] == codes([F(0.6)], 0, 1)[0]).all()
        lo2, hi2 = int(codes([F(0.1)], 0, 1)[0]), int(codes([F(0.9)], 0, 1)[0])
        assert want[2].tolist() == [hi2 if p == 1000 else lo2 for p in pm]         # n = 2: rank p // 1000
    # two entries in one coarse bin, a third elsewhere: a narrow image, 1 / 65536 a code
    v = (F(0.5) + rng.integers(0, 200, n).astype(F) / F(65536)).astype(F)
    want = check(runs(rng, n, range(4), 30), v, 3, 0.0, 1.0, pm=(100, 900, 500, 1000))["quantiles"]
    assert (want >> 8 == 128).all() and (want[:, 0] < want[:, 2]).all() and (want[:, 2] < want[:, 1]).all()


# ---- the host arithmetic, streams ----------------------------------------------------------------------------------------------------
def test_volume_range_against_numpy():
    rng = np.random.default_rng(11)
    for v in (noise(rng, MID, -5.0, 5.0), rng.standard_normal(MID).astype(F) * F(1e20), np.asarray([NAN, 2.5, NAN], F),
              np.asarray([-0.0, -1e-30], F), np.full(9, 7.25, F)):
        lo, hi = S.volume_range(torch.from_numpy(v).to(DEV))
        assert isinstance(lo, float) and lo == float(np.nanmin(v)) and hi == float(np.nanmax(v))
    lo, hi = S.volume_range(torch.full((33,), NAN, device=DEV))
    assert np.isnan(lo) and np.isnan(hi)
    vol = rng.uniform(-3, 3, (4, 5, 6)).astype(F)                   # any shape
    assert S.volume_range(torch.from_numpy(vol).to(DEV)) == (float(vol.min()), float(vol.max()))


def test_summary_on_device_rows():
    rng = np.random.default_rng(12)
    lo, hi, L = -1000.0, 3000.0, 4
    labels = runs(rng, MID, range(L), 200)                          # row L stays empty
    v = np.clip(rng.normal(500, 400, MID), lo, hi).astype(F)
    lab, img = dev_map(labels, torch.uint8), torch.from_numpy(v).to(DEV)
    s = S.summary(S.moments(lab, img, L, lo, hi), lo, hi, S.quantiles(lab, img, L, lo, hi, (50, 500, 950)))
    width = (hi - lo) / 65536
    for l in range(L):
        x = v[labels == l].astype(np.float64)
        assert s["n"][l] == x.size and abs(s["mean"][l] - x.mean()) <= width and abs(s["std"][l] - x.std()) <= 2 * width
        assert s["min"][l] == x.min() and s["max"][l] == x.max()
        assert abs(s["quantiles"][l, 1] - np.sort(x)[(x.size - 1) // 2]) <= width
        assert s["quantiles"][l, 0] < s["quantiles"][l, 1] < s["quantiles"][l, 2]
    assert np.isnan(s["mean"][L]) and np.isnan(s["quantiles"][L]).all() and s["n"][L] == 0


def test_two_threads_on_two_streams_with_their_own_scratch():
    cases, errors = [], []
    pm = (100, 500, 900)
    for seed, L in ((1, 400), (2, 2035)):
        rng = np.random.default_rng(seed)
        labels, v = runs(rng, MID, range(L + 1), 150), noise(rng, MID, 0.0, 1.0)
        cases.append((dev_map(labels, torch.uint16), torch.from_numpy(v).to(DEV), L, moments_ref(labels, v, L, 0, 1), hist_ref(labels, v, L, 0, 1),
                      quantiles_ref(labels, v, L, 0, 1, pm)))
    torch.cuda.synchronize()

    def work(k):
        try:
            lab, img, L, want_m, want_h, want_q = cases[k]
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(S.stats_scratch_bytes(img.numel(), L, len(pm)), dtype=torch.uint8, device=DEV)
                for rep in range(3):
                    kw = dict(impl=IMPLS[rep], scratch=scratch, stream=stream.cuda_stream)
                    m = S.moments(lab, img, L, 0.0, 1.0, **kw)
                    h = S.hist(lab, img, L, 0.0, 1.0, **kw)
                    q = S.quantiles(lab, img, L, 0.0, 1.0, pm, **kw)
                    stream.synchronize()
                    assert same(m.cpu().numpy(), want_m) and same(h.cpu().numpy(), want_h) and same(q.cpu().numpy(), want_q)
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
