"""GPU: the atlas preparation on the device (include/unet_atlas.h) -- reclassify under IMPL_LDS, IMPL_GLOBAL and the default against
the transcription of evaluate.cpp in test_atlas_host.py, grow against that file's restatement of Fill and Smooth, prepare_atlas
against the two chained in the reference's order.  Every case runs twice with every report tensor pre-filled with garbage; every
comparison is exact equality of bytes."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U  # noqa: F401
from unet_studio_amd import atlas as A
from unet_studio_amd import space as SP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_atlas_host import grow_ref, reclassify_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (A.IMPL_LDS, A.IMPL_GLOBAL, A.IMPL_DEFAULT)
L = A.LDS_ENTRIES
SIZES = [1, 7, 8, 9, 255, 256, 257, 2049, 130 * 40 * 7, 97 * 113 * 91]
GUARD = 0xA5C3


def dev_int(a, dtype):
    """a numpy integer array as a device tensor of torch.uint8 / torch.uint16"""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(dtype)


def host(t):
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def garbage(spec, rep):
    """{name: (entries, dtype)} -> tensors whose every byte is set"""
    out = {}
    for k, (n, dt) in spec.items():
        size = torch.empty(0, dtype=dt).element_size()
        out[k] = torch.full((n * size,), 0x5A + rep, dtype=torch.uint8, device=DEV).view(dt)
    return out


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def check_reclassify(tissue, atlas, R, T, flags, tb=1, impls=IMPLS, place=None):
    """tissue, atlas: flat numpy arrays.  Every implementation twice against the transcription: the atlas and the five reports
    exactly (equal dtype, equal values: equal bytes); then COUNT_ONLY: the same reports and the atlas untouched.  place(tissue_dev, atlas_dev) -> (tissue view, atlas view,
    after) lets a case put them at odd addresses; after() checks its guards."""
    exp = reclassify_ref(tissue, atlas, R, T, flags)
    names = ("votes", "tissue_total", "covered", "majority", "erased")
    t_src, a_src = dev_int(tissue, torch.uint8 if tb == 1 else torch.uint16), dev_int(atlas, torch.uint16)
    spec = dict(votes=((R + 1) * T, torch.uint32), tissue_total=(T, torch.uint32), covered=(T, torch.uint32), majority=(R + 1, torch.uint8),
                erased=(R + 1, torch.uint32))
    for impl in impls:
        for rep, count_only in ((0, False), (1, False), (1, True)):
            t_dev, a_dev, after = place(t_src, a_src) if place else (t_src, a_src.clone(), None)
            out = garbage(spec, rep)                                                         # the call must fill them completely
            got = A.reclassify(t_dev, a_dev, R, T, flags=flags, count_only=count_only, impl=impl, out=out)
            assert got is out
            want_atlas = np.asarray(atlas).astype(np.uint16) if count_only else exp[0]
            assert same(host(a_dev), want_atlas), (impl, rep, count_only)
            for name, want in zip(names, exp[1:]):
                assert same(host(out[name]), want.reshape(-1)), (name, impl, rep, count_only)
            if after:
                after()
    return exp


# ---- the patterns: rng, S, R, T -> (tissue, atlas), flat ----------------------------------------------------------------------------
def runs(rng, S, lo, hi, longest):
    """random values in [lo, hi] in runs of random length 1..longest: solid stretches that cross the vector and block borders"""
    n = rng.integers(1, longest + 1, S)
    return np.repeat(rng.integers(lo, hi + 1, S), n)[:S]


def pat_solid(rng, S, R, T):
    """nested regions (long runs) on long runs of tissue, 2 % of the voxels in a random other tissue"""
    tissue = runs(rng, S, 0, T - 1, 200)
    atlas = runs(rng, S, 0, R, 60)
    stray = rng.random(S) < 0.02
    tissue[stray] = rng.integers(0, T + 2, int(stray.sum()))       # values >= T among them
    return tissue, atlas


def pat_random(rng, S, R, T):
    return rng.integers(0, T + 2, S), rng.integers(0, R + 1, S)


def pat_one_region(rng, S, R, T):
    return runs(rng, S, 0, T - 1, 50), np.full(S, min(R, 2))


def pat_absent_region(rng, S, R, T):
    tissue, atlas = pat_solid(rng, S, R, T)
    atlas[atlas == min(R, 2)] = 0                                  # region 2 does not occur: an empty row
    return tissue, atlas


def pat_above_r(rng, S, R, T):
    tissue, atlas = pat_solid(rng, S, R, T)
    high = rng.random(S) < 0.1
    atlas[high] = rng.integers(R + 1, 65536, int(high.sum()))      # never counted, never written (but PRESERVE comes first)
    return tissue, atlas


PATTERNS = dict(solid=pat_solid, random=pat_random, one_region=pat_one_region, absent_region=pat_absent_region, above_r=pat_above_r)


@pytest.mark.parametrize("S", SIZES)
def test_reclassify_sizes(S):
    rng = np.random.default_rng(S)
    for pat in (pat_solid, pat_random):
        tissue, atlas = pat(rng, S, 130, 5)
        check_reclassify(tissue, atlas, 130, 5, A.CLAMP | A.PRESERVE)
    check_reclassify(tissue, atlas, 130, 5, 0, impls=(A.IMPL_LDS, A.IMPL_GLOBAL))


@pytest.mark.parametrize("tb", [1, 2])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reclassify_patterns_under_every_flag_combination(name, tb):
    S = 130 * 40 * 7
    tissue, atlas = PATTERNS[name](np.random.default_rng(len(name) + tb), S, 130, 5)
    if tb == 2:
        tissue = np.where(tissue >= 5, tissue * 9001, tissue)      # values that need 16 bits
    for flags in (0, A.CLAMP, A.PRESERVE, A.CLAMP | A.PRESERVE):
        exp = check_reclassify(tissue, atlas, 130, 5, flags, tb)
    assert int(exp[5].sum()) > 0 or name == "one_region"


def test_reclassify_an_all_zero_atlas_with_no_region():
    rng = np.random.default_rng(0)
    for S in (9, 2049):
        tissue = rng.integers(0, 7, S)
        for flags in (0, A.CLAMP | A.PRESERVE):
            exp = check_reclassify(tissue, np.zeros(S, np.int64), 0, 5, flags)
            assert exp[1].shape == (1, 5) and not exp[1].any() and exp[4].tolist() == [0]
    # R = 0 with a non-zero atlas: every value is above R; PRESERVE still zeroes the voxels on tissue 0
    check_reclassify(tissue, rng.integers(0, 3, S), 0, 5, A.CLAMP | A.PRESERVE)
    check_reclassify(tissue, rng.integers(0, 3, S), 0, 5, 0)


# every R at which another path is taken: the votes rows that fit a block's table (L / T), the erased entries that do (L)
@pytest.mark.parametrize("T,R", [(T, R) for T in (1, 5, 256) for R in (3, 130, L // 5 - 1, L // 5, L // 5 + 1, 65535)] +
                         [(1, L - 2), (1, L - 1), (1, L), (256, L // 256 - 1), (256, L // 256), (5, L - 1), (5, L)])
def test_reclassify_tissue_and_region_counts(T, R):
    rng = np.random.default_rng(T * 65536 + R)
    S = 130 * 40 * 7
    tissue = runs(rng, S, 0, T + 1, 30) if T < 256 else runs(rng, S, 0, 255, 30)
    atlas = np.where(rng.random(S) < 0.5, runs(rng, S, 0, min(R + 2, 65535), 12), runs(rng, S, max(0, R - 40), min(R + 2, 65535), 12))
    for tb, flags in ((1, A.CLAMP | A.PRESERVE), (2, 0)):
        exp = check_reclassify(tissue, atlas, R, T, flags, tb, impls=(A.IMPL_LDS, A.IMPL_GLOBAL) if tb == 2 else IMPLS)
    assert exp[1][R].sum() > 0 or T == 1                           # the last row is in use


@pytest.mark.parametrize("tb", [1, 2])
def test_reclassify_at_odd_addresses_with_guard_words(tb):
    rng = np.random.default_rng(77 + tb)
    for S in (1, 5, 9, 2049 + 13):
        tissue, atlas = pat_solid(rng, S, 130, 5)
        for a_off in (1, 7):                                       # elements: 2 and 14 bytes off a 16-byte boundary
            for t_off in (1, 3):                                   # elements: 1 and 3 bytes (uint8), 2 and 6 bytes (uint16)

                def place(t_src, a_src):
                    abuf = torch.full((S + 32,), GUARD, dtype=torch.int32, device=DEV).to(torch.uint16)
                    tbuf = torch.zeros(S + 32, dtype=torch.int32, device=DEV).to(t_src.dtype)
                    assert abuf.data_ptr() % 16 == 0 and tbuf.data_ptr() % 16 == 0
                    a_dev, t_dev = abuf[a_off:a_off + S], tbuf[t_off:t_off + S]
                    a_dev.copy_(a_src)
                    t_dev.copy_(t_src)
                    assert a_dev.data_ptr() % 16 == 2 * a_off and t_dev.data_ptr() % 16 == t_off * t_src.element_size()

                    def after():
                        g = host(abuf)
                        assert (g[:a_off] == GUARD).all() and (g[a_off + S:] == GUARD).all()
                    return t_dev, a_dev, after

                check_reclassify(tissue, atlas, 130, 5, A.CLAMP | A.PRESERVE, tb, place=place)


# ---- grow ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 1, 33), (33, 9, 9), (65, 3, 2), (40, 37, 29)]       # (W, H, D)


def check_grow(tissue, atlas, T, grow, flags=0, max_rounds=None, smooth_rounds=1, tb=1, expect=None):
    """tissue, atlas: (D, H, W) numpy arrays.  The device twice against the restatement: the atlas and the three reports exactly."""
    exp = expect if expect is not None else grow_ref(tissue, atlas, T, grow, flags, max_rounds, smooth_rounds)
    t_dev, a_src = dev_int(tissue, torch.uint8 if tb == 1 else torch.uint16), dev_int(atlas, torch.uint16)
    spec = dict(filled=(T, torch.uint32), relabelled=(T, torch.uint32), info=(2, torch.uint32))
    for rep in range(2):
        a_dev, out = a_src.clone(), garbage(spec, rep)
        assert A.grow(t_dev, a_dev, T, grow, flags=flags, max_rounds=max_rounds, smooth_rounds=smooth_rounds, out=out) is out
        assert same(host(a_dev), exp[0]), (rep, int((host(a_dev) != exp[0]).sum()))
        for name, want in zip(("filled", "relabelled", "info"), exp[1:]):
            assert same(host(out[name]), want), (name, rep, host(out[name]).tolist(), want.tolist())
    return exp


def snake(shape):
    """a one-voxel-wide path through all of its voxels: in every other z-plane rows along x at every other y joined at alternating
    ends; the planes joined alternately where the comb ends and where it starts.  Returns (mask, head): head is the path's first voxel"""
    D, H, W = shape
    m = np.zeros(shape, bool)
    y_last = (H - 1) // 2 * 2
    x_end = W - 1 if (y_last // 2) % 2 == 0 else 0                  # where the comb's last row ends
    for zi, z in enumerate(range(0, D, 2)):
        for y in range(0, H, 2):
            m[z, y, :] = True
            if y + 2 < H:
                m[z, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = True
        if z + 2 < D:
            m[(z + 1,) + ((y_last, x_end) if zi % 2 == 0 else (0, 0))] = True
    return m, (0, 0, 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_grow_a_seed_at_the_centre_of_a_solid_tissue_and_two_seeds_with_ties(shape):
    W, H, D = shape
    tissue = np.ones((D, H, W), np.int64)
    atlas = np.zeros((D, H, W), np.int64)
    atlas[D // 2, H // 2, W // 2] = 9
    for smooth in (0, 1):
        exp = check_grow(tissue, atlas, 2, [1], smooth_rounds=smooth)
        assert (exp[0] == 9).all() and exp[3][1] == 1 and exp[1][1] == W * H * D - 1
    atlas[0, 0, 0], atlas[D - 1, H - 1, W - 1] = 7, 4              # both ends: the voxels at equal distance take the smaller label
    exp = check_grow(tissue, atlas, 2, [1], smooth_rounds=0, tb=2)
    assert exp[3][1] == 1 and (exp[0] != 0).all()
    for max_rounds in (1, 3):                                      # the restatement's truncated state
        exp = check_grow(tissue, atlas, 2, [1], max_rounds=max_rounds, smooth_rounds=1)
        if W + H + D > 12:
            assert exp[3].tolist() == [max_rounds, 0] and not exp[0].all()


# not the largest shape: its snake takes 11 000 rounds, minutes in the restatement
@pytest.mark.parametrize("shape", SHAPES[:-1])
def test_grow_a_snake_takes_one_round_per_voxel(shape):
    W, H, D = shape
    m, head = snake((D, H, W))
    tissue = np.where(m, 1, 2)
    atlas = np.zeros((D, H, W), np.int64)
    atlas[head] = 3
    rounds = int(m.sum()) - 1                                      # 848 at (33, 9, 9): the chain of early exits
    exp = check_grow(tissue, atlas, 3, [1], max_rounds=rounds + 50, smooth_rounds=0)
    assert exp[3].tolist() == [rounds, 1] and (exp[0][m] == 3).all() and not exp[0][~m].any()
    if shape == (33, 9, 9):
        assert rounds > 300
    if rounds > 0:                                                 # exactly enough rounds: complete, but no round filled nothing
        assert check_grow(tissue, atlas, 3, [1], max_rounds=rounds, smooth_rounds=0)[3].tolist() == [rounds, 0]
    if rounds > 3:                                                 # W + H + D rounds are not enough for a long snake: converged = 0
        exp = check_grow(tissue, atlas, 3, [1], max_rounds=3, smooth_rounds=0)
        assert exp[3].tolist() == [3, 0] and int((exp[0] == 3).sum()) == 4


@pytest.mark.parametrize("shape", SHAPES)
def test_grow_random_tissue_maps_with_subsets_flagged(shape):
    W, H, D = shape
    rng = np.random.default_rng(W * 10000 + H * 100 + D)
    for n_t, flagged, flags, tb in ((2, [1], 0, 1), (3, [1, 2], A.PRESERVE, 2), (4, [0, 2, 3], A.CLAMP, 1), (4, [1, 2, 3], A.CLAMP | A.PRESERVE, 1)):
        tissue = rng.integers(0, n_t + 1, (D, H, W))               # the value n_t is >= T
        atlas = np.where(rng.random((D, H, W)) < 0.15, rng.integers(1, 6, (D, H, W)), 0)
        for smooth in (0, 1, 2):
            check_grow(tissue, atlas, n_t, flagged, flags, smooth_rounds=smooth, tb=tb)
    # all tissues in one call against one call per tissue (evaluate.cpp:166-174)
    exp = grow_ref(tissue, atlas, 4, [1, 2, 3], A.CLAMP, None, 2)
    t_dev, a_dev = dev_int(tissue, torch.uint8), dev_int(atlas, torch.uint16)
    filled = np.zeros(4, np.uint32)
    for t in (1, 2, 3):
        filled += host(A.grow(t_dev, a_dev, 4, [t], flags=A.CLAMP, smooth_rounds=2)["filled"])
    assert host(a_dev).tobytes() == exp[0].tobytes() and filled.tobytes() == exp[1].tobytes()


def test_grow_an_unreachable_pocket_stays_0_and_the_fill_converges():
    D, H, W = 9, 9, 33
    tissue = np.ones((D, H, W), np.int64)
    tissue[3:6, 3:6, 10:13] = 2                                    # a shell of tissue 2 ...
    tissue[4, 4, 11] = 1                                           # ... around one voxel of tissue 1 no label reaches
    atlas = np.zeros((D, H, W), np.int64)
    atlas[0, 0, 0] = 5
    exp = check_grow(tissue, atlas, 3, [1, 2], smooth_rounds=1)
    assert exp[0][4, 4, 11] == 0 and exp[3][1] == 1 and not exp[0][tissue == 2].any() and exp[1].tolist() == [0, D * H * W - 27 - 1, 0]


# ---- prepare_atlas ---------------------------------------------------------------------------------------------------------------
def synthetic_template(shape):
    """nested shells of tissues 1..4 around the centre, 0 outside, and some voxels of 5 and 6 that must read 0"""
    D, H, W = shape
    z, y, x = np.indices(shape)
    r = np.sqrt(((x - W / 2) / (W / 2)) ** 2 + ((y - H / 2) / (H / 2)) ** 2 + ((z - D / 2) / (D / 2)) ** 2)
    t = (4 - np.floor(r / 0.22)).clip(0, 4).astype(np.int64)
    rng = np.random.default_rng(3)
    high = rng.random(shape) < 0.03
    t[high] = rng.integers(5, 7, int(high.sum()))
    return t


def synthetic_atlas(shape):
    """up to 12 regions (the innermost shell may miss a third): the template's four shells, shifted by a voxel or so, each cut in
    three along x; 3 % holes, many more in a thin slab through the centre, and a margin of zeros"""
    D, H, W = shape
    z, y, x = np.indices(shape)
    r = np.sqrt(((x - W / 2 - 0.7) / (W / 2)) ** 2 + ((y - H / 2 + 0.6) / (H / 2)) ** 2 + ((z - D / 2) / (D / 2)) ** 2)
    shell = (4 - np.floor(r / 0.22)).clip(0, 4).astype(np.int64)
    a = np.where(shell > 0, (shell - 1) * 3 + 1 + x * 3 // W, 0)
    rng = np.random.default_rng(4)
    a[rng.random(shape) < 0.03] = 0
    a[(rng.random(shape) < 0.6) & (np.abs(z - D / 2) < D / 10)] = 0
    a[:, :, :2] = 0
    return a


def prepare_ref(template, on_grid, T=5):
    """evaluate.cpp:130-175 with the two restatements: preserve, totals and coverage, reclassify, then one tissue at a time"""
    D, H, W = template.shape
    R = int(on_grid.max())
    flags = A.CLAMP | A.PRESERVE
    out, votes, total, covered, majority, erased = reclassify_ref(template, on_grid, R, T, flags)
    grown, filled = [], np.zeros(T, np.uint32)
    rounds, converged = 0, 1
    for t in range(1, T):
        if total[t] == 0 or np.float32(covered[t]) / np.float32(total[t]) <= np.float32(0.75):
            continue
        grown.append(t)
        out, f, _, info = grow_ref(template, out, T, [t], flags, W + H + D, 1)
        filled += f
        rounds, converged = max(rounds, int(info[0])), converged & int(info[1])
    return out, dict(n_regions=R, majority=majority, erased=erased, grown=grown, filled=filled, rounds=rounds, converged=bool(converged),
                     total=total, covered=covered)


@pytest.mark.parametrize("with_map", [False, True])
def test_prepare_atlas_against_the_restatements_chained_in_the_reference_order(with_map):
    shape = (29, 37, 40)
    template = synthetic_template(shape)
    t_dev = dev_int(template, torch.uint8)
    if with_map:
        small = (15, 19, 20)
        a_dev = dev_int(synthetic_atlas(small), torch.uint16)
        m = (np.diag([0.5, 0.5, 0.5]).reshape(9), np.zeros(3))     # template voxel -> atlas position
        on_grid = SP.resample(a_dev.to(torch.int32).to(torch.float32), shape, m, mode="majority").cpu().numpy().astype(np.int64)
    else:
        a_dev, m = dev_int(synthetic_atlas(shape), torch.uint16), None
        on_grid = synthetic_atlas(shape)
    before = host(a_dev).copy()
    exp, rep = prepare_ref(template, on_grid)
    R = rep["n_regions"]
    assert R in (11, 12) and 1 <= len(rep["grown"]) < 4 and rep["filled"].sum() > 0 and rep["erased"].sum() > 0
    for _ in range(2):
        got, report = A.prepare_atlas(t_dev, a_dev, n_tissues=5, map=m)
        assert got.dtype == torch.uint16 and tuple(got.shape) == shape and host(got).tobytes() == exp.tobytes()
        assert host(a_dev).tobytes() == before.tobytes()            # the input is not changed
        assert report["n_regions"] == R and report["grown"] == rep["grown"] and report["converged"] == rep["converged"]
        assert report["majority"].tobytes() == rep["majority"].tobytes() and report["erased"].tobytes() == rep["erased"].tobytes()
        assert report["filled"].tobytes() == rep["filled"].tobytes() and report["rounds"] == rep["rounds"]
        assert report["tissue_total"].tobytes() == rep["total"].tobytes() and report["covered"].tobytes() == rep["covered"].tobytes()
        assert report["erased_reported"] == [int(rep["erased"][a]) for a in range(1, R + 1) if rep["majority"][a] > 0]
        cov = report["coverage"]
        assert cov.dtype == np.float32 and cov[0] == 0 and all((cov[t] > np.float32(0.75)) == (t in rep["grown"]) for t in range(1, 5))


# ---- two host threads, two streams, their own scratch --------------------------------------------------------------------------------
def test_two_threads_on_two_streams_with_their_own_scratch():
    shape = (29, 37, 40)
    S = int(np.prod(shape))
    cases, errors = [], []
    for k in range(2):
        rng = np.random.default_rng(50 + k)
        tissue, atlas = pat_solid(rng, S, 130, 5)
        exp_r = reclassify_ref(tissue, atlas, 130, 5, A.CLAMP | A.PRESERVE)
        exp_g = grow_ref(tissue.reshape(shape), exp_r[0].reshape(shape), 5, [1, 2, 3, 4], A.CLAMP | A.PRESERVE, None, 1)
        cases.append((dev_int(tissue.reshape(shape), torch.uint8), dev_int(atlas.reshape(shape), torch.uint16), exp_r, exp_g))
    torch.cuda.synchronize()

    def work(k):
        try:
            t_dev, a_src, exp_r, exp_g = cases[k]
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(A.atlas_scratch_bytes(S, 130, 5, sum(shape)), dtype=torch.uint8, device=DEV)
                for _ in range(3):
                    a_dev = a_src.clone()
                    r = A.reclassify(t_dev, a_dev, 130, 5, flags=A.CLAMP | A.PRESERVE, scratch=scratch, stream=stream.cuda_stream)
                    g = A.grow(t_dev, a_dev, 5, [1, 2, 3, 4], flags=A.CLAMP | A.PRESERVE, scratch=scratch, stream=stream.cuda_stream)
                    stream.synchronize()
                    assert host(a_dev).tobytes() == exp_g[0].tobytes()
                    assert host(r["votes"]).tobytes() == exp_r[1].tobytes() and host(r["erased"]).tobytes() == exp_r[5].tobytes()
                    assert host(g["filled"]).tobytes() == exp_g[1].tobytes() and host(g["info"]).tobytes() == exp_g[3].tobytes()
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
