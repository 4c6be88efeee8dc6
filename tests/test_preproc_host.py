"""CPU: the host half of a model's pre-processing chain and orientation (include/unet_preproc.h, unet-studio_amd/preproc.py) -- the
ABI the library exports, parsing, the geometry and orientation maps' known answers, the exact identities the no-op path rests on,
and argument errors found before any device call.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import preproc as PRE
from unet_studio_amd import space as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3, dtype=np.float32).reshape(9).tobytes()
ZERO = np.zeros(3, np.float32).tobytes()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_unet_preproc_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_preproc.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(PRE.EXPORTS) == {"unet_preproc_filter", "unet_preproc_downsample", "unet_preproc_upsample",
                                            "unet_preproc_permute", "unet_preproc_scratch_bytes", "unet_preproc_normalize"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_PREPROC_([A-Z_]+) = (\d+)", hdr)}
    assert (enums["GAUSSIAN"], enums["MEAN"]) == (PRE.FILTER_GAUSSIAN, PRE.FILTER_MEAN)
    assert (enums["IMPL_DEFAULT"], enums["IMPL_LDS"], enums["IMPL_VOXEL"]) == (PRE.IMPL_DEFAULT, PRE.IMPL_LDS, PRE.IMPL_VOXEL)
    for name, op in PRE.PERMUTES.items():
        assert enums[name.upper()] == op


def test_the_other_headers_do_not_mention_the_new_prefix():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_preproc.h":
            assert "unet_preproc_" not in open(os.path.join(ROOT, "include", h)).read(), h


# ---- parsing ---------------------------------------------------------------------------------------------------------------------
def test_parse_known_answers():
    assert PRE.parse_chain("") == [] and PRE.parse_chain(None) == [] and PRE.parse_chain(" + +") == []
    assert PRE.parse_chain("gaussian_filter") == ["gaussian_filter"]
    assert PRE.parse_chain(" gaussian_filter + downsampling+ +normalize ") == ["gaussian_filter", "downsampling", "normalize"]
    assert PRE.parse_chain("+".join(PRE.COMMANDS)) == list(PRE.COMMANDS)
    assert set(PRE.COMMANDS) == {"none", "gaussian_filter", "smoothing_filter", "normalize", "upsampling", "downsampling", "flip_x",
                                 "flip_y", "flip_z", "swap_xy", "swap_yz", "swap_xz"} and len(PRE.COMMANDS) == 12
    assert PRE.active(PRE.parse_chain("none+flip_x+none")) == ["flip_x"]
    assert PRE.parse_orientation("swap_xy + flip_x") == ["swap_xy", "flip_x"]
    assert PRE.parse_orientation("") == [] and PRE.parse_orientation(None) == []


def test_unknown_commands_have_the_reference_message():
    with pytest.raises(U.UNetError) as e:
        PRE.parse_chain("gaussian_filter+sharpen")
    assert str(e.value) == "unknown command sharpen"
    with pytest.raises(U.UNetError) as e:
        PRE.parse_chain("softmax")                          # a postproc command is not a preproc command
    assert str(e.value) == "unknown command softmax"
    for bad in ("gaussian_filter", "normalize", "none", "downsampling", "flip_w"):
        with pytest.raises(U.UNetError) as e:
            PRE.parse_orientation("flip_x+" + bad)          # only the six flips / swaps orient
        assert str(e.value) == "unknown command " + bad
    with pytest.raises(U.UNetError, match="unknown command rot90"):
        PRE.geometry(["flip_x", "rot90"], (4, 4, 4), (1, 1, 1))


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def apply(map, p):
    m, t = map
    assert m.dtype == np.float32 and m.shape == (9,) and t.dtype == np.float32 and t.shape == (3,)
    return np.asarray(m, np.float64).reshape(3, 3) @ np.asarray(p, np.float64) + np.asarray(t, np.float64)


def test_geometry_known_answers():
    dims, vs, G = PRE.geometry("downsampling", (61, 70, 41), (1, 1, 1.2))
    assert dims == (31, 35, 21) and vs == (2.0, 2.0, 2.4)
    assert np.array_equal(G[0], (2 * np.eye(3)).reshape(9).astype(np.float32)) and np.array_equal(G[1], np.float32([0.5, 0.5, 0.5]))
    assert np.array_equal(apply(G, (3, 4, 5)), [6.5, 8.5, 10.5])
    dims, vs, G = PRE.geometry("upsampling", (31, 35, 21), (2, 2, 2.4))
    assert dims == (62, 70, 42) and vs == (1.0, 1.0, 1.2)
    assert np.array_equal(G[0], (0.5 * np.eye(3)).reshape(9).astype(np.float32)) and np.array_equal(G[1], np.float32([-0.25] * 3))
    # hand-written: flip_x on (10, 20, 30), then swap_yz -> grid (10, 30, 20); result (x, y, z) <- flipped (x, z, y) <- original (9 - x, z, y)
    dims, vs, G = PRE.geometry("flip_x+swap_yz", (10, 20, 30), (1, 2, 3))
    assert dims == (10, 30, 20) and vs == (1.0, 3.0, 2.0)
    assert np.array_equal(G[0], np.float32([-1, 0, 0, 0, 0, 1, 0, 1, 0])) and np.array_equal(G[1], np.float32([9, 0, 0]))
    # swap_yz first, then flip_y of the swapped grid (10, 30, 20): result (x, y, z) <- (x, 29 - y, z) <- original (x, z, 29 - y)
    dims, vs, G = PRE.geometry("swap_yz+flip_y", (10, 20, 30), (1, 2, 3))
    assert dims == (10, 30, 20)
    assert np.array_equal(G[0], np.float32([1, 0, 0, 0, 0, 1, 0, -1, 0])) and np.array_equal(G[1], np.float32([0, 0, 29]))
    # filters, normalize and none move nothing; down then up: x -> 2 * (x/2 - 0.25) + 0.5 = x
    dims, vs, G = PRE.geometry("gaussian_filter+none+normalize+smoothing_filter", (5, 6, 7), (1, 1, 1))
    assert dims == (5, 6, 7) and G[0].tobytes() == EYE and G[1].tobytes() == ZERO
    dims, vs, G = PRE.geometry("downsampling+upsampling", (61, 70, 41), (1, 1, 1.2))
    assert dims == (62, 70, 42) and vs == (1.0, 1.0, 1.2) and G[0].tobytes() == EYE and G[1].tobytes() == ZERO
    with pytest.raises(U.UNetError, match="2\\^31"):
        PRE.geometry("upsampling", (1024, 1024, 256), (1, 1, 1))
    with pytest.raises(U.UNetError):
        PRE.geometry("flip_x", (4, 0, 4), (1, 1, 1))
    with pytest.raises(U.UNetError):
        PRE.geometry("flip_x", (4, 4, 4), (1, 0, 1))


def test_orientation_map_known_answers():
    D0, vs0, M = PRE.orientation_map("swap_xy+flip_x", (48, 56, 40), (1.0, 1.5, 2.0))
    assert D0 == (56, 48, 40) and vs0 == (1.5, 1.0, 2.0)
    # swap_xy of the D0 grid gives (48, 56, 40) with (x, y, z) <- (y, x, z); flip_x of that gives (x, y, z) <- (47 - x, y, z)
    assert np.array_equal(M[0], np.float32([0, 1, 0, -1, 0, 0, 0, 0, 1])) and np.array_equal(M[1], np.float32([0, 47, 0]))
    for p in [(0, 0, 0), (47, 55, 39), (5, 7, 11)]:
        assert np.array_equal(apply(M, p), [p[1], 47 - p[0], p[2]])
    # the orientation applied to D0 yields the model's grid exactly
    assert PRE.geometry("swap_xy+flip_x", D0, vs0)[:2] == ((48, 56, 40), (1.0, 1.5, 2.0))
    D0, vs0, M = PRE.orientation_map("swap_xy+swap_yz", (3, 4, 5), (1, 2, 3))
    assert PRE.geometry("swap_xy+swap_yz", D0, vs0)[:2] == ((3, 4, 5), (1.0, 2.0, 3.0)) and D0 == (5, 3, 4)
    D0, vs0, M = PRE.orientation_map("flip_z", (3, 4, 5), (1, 2, 3))
    assert D0 == (3, 4, 5) and np.array_equal(apply(M, (1, 2, 0)), [1, 2, 4])


def test_empty_chains_give_exact_identities_and_composition_keeps_the_bits():
    for text in ("", None, "none", "none+none"):
        dims, vs, G = PRE.geometry(text, (61, 70, 41), (1, 1, 1.2))
        assert dims == (61, 70, 41) and vs == (1.0, 1.0, 1.2) and G[0].tobytes() == EYE and G[1].tobytes() == ZERO
    for text in ("", None):
        D0, vs0, M = PRE.orientation_map(text, (48, 56, 40), (1, 1, 1))
        assert D0 == (48, 56, 40) and vs0 == (1.0, 1.0, 1.0) and M[0].tobytes() == EYE and M[1].tobytes() == ZERO
    # what the no-op path rests on: composing with the exact identity on either side leaves F's bits alone, so its inverse too
    F = SP.model_to_image_map((48, 56, 40), (1, 1, 1), (40, 44, 64), (1.2, 1.1, 0.8))
    ident = PRE.geometry("", (40, 44, 64), (1.2, 1.1, 0.8))[2]
    for c in (SP.compose_map(F, ident), SP.compose_map(ident, F), SP.compose_map(ident, SP.compose_map(F, ident))):
        assert c[0].tobytes() == F[0].tobytes() and c[1].tobytes() == F[1].tobytes()
        i, j = SP.invert_map(c), SP.invert_map(F)
        assert i[0].tobytes() == j[0].tobytes() and i[1].tobytes() == j[1].tobytes()


# ---- argument errors, before any device call ---------------------------------------------------------------------------------------
def test_scratch_bytes_and_its_errors():
    n = PRE.preproc_scratch_bytes(2 * 256 * 256 * 180)
    assert 256 < n < 1 << 16 and PRE.preproc_scratch_bytes(1) > 256
    with pytest.raises(U.UNetError, match="values must be positive"):
        PRE.preproc_scratch_bytes(0)
    rc = U.engine.lib.unet_preproc_scratch_bytes(10, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


def test_argument_errors_need_no_device():
    a, b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)      # never dereferenced
    lib = U.engine.lib

    def err(rc):
        assert rc != 0
        return lib.unet_last_error().decode()

    calls = {
        "filter": lambda src=a, dst=b, s=(4, 4, 4), ch=1: lib.unet_preproc_filter(src, dst, s[0], s[1], s[2], ch, 0, 0, None),
        "down": lambda src=a, dst=b, s=(4, 4, 4), ch=1: lib.unet_preproc_downsample(src, dst, s[0], s[1], s[2], ch, None),
        "up": lambda src=a, dst=b, s=(4, 4, 4), ch=1: lib.unet_preproc_upsample(src, dst, s[0], s[1], s[2], ch, None),
        "permute": lambda src=a, dst=b, s=(4, 4, 4), ch=1: lib.unet_preproc_permute(src, dst, s[0], s[1], s[2], ch, 3, None),
    }
    for name, call in calls.items():
        assert "null device pointer" in err(call(src=None)), name
        assert "null device pointer" in err(call(dst=None)), name
        assert "src and dst must differ" in err(call(dst=a)), name
        assert "dimensions must be positive" in err(call(s=(0, 4, 4))), name
        assert "dimensions must be positive" in err(call(s=(4, 4, -1))), name
        assert "2^31" in err(call(s=(2048, 1024, 1024))), name
        assert "channels" in err(call(ch=0)), name
        assert "channels" in err(call(ch=65536)), name
    assert "2^31" in err(calls["up"](s=(1024, 1024, 256)))             # the RESULT would have 2^31 voxels
    assert "unknown kind 2" in err(lib.unet_preproc_filter(a, b, 4, 4, 4, 1, 2, 0, None))
    assert "unknown kind -1" in err(lib.unet_preproc_filter(a, b, 4, 4, 4, 1, -1, 0, None))
    assert "unknown impl 3" in err(lib.unet_preproc_filter(a, b, 4, 4, 4, 1, 0, 3, None))
    assert "unknown op 6" in err(lib.unet_preproc_permute(a, b, 4, 4, 4, 1, 6, None))
    assert "unknown op -1" in err(lib.unet_preproc_permute(a, b, 4, 4, 4, 1, -1, None))
    assert "null device pointer" in err(lib.unet_preproc_normalize(None, 64, a, 1 << 20, None))
    assert "values must be positive" in err(lib.unet_preproc_normalize(a, 0, b, 1 << 20, None))
    assert "null scratch" in err(lib.unet_preproc_normalize(a, 64, None, 0, None))
    assert "scratch too small" in err(lib.unet_preproc_normalize(a, 64, b, 16, None))


def test_wrapper_errors_need_no_device():
    host = np.zeros((1, 4, 4, 4), np.float32)
    with pytest.raises(U.UNetError, match="device tensor"):
        PRE.run_preproc(host, "gaussian_filter")                 # a host array is not a device tensor
    with pytest.raises(U.UNetError, match="device tensor"):
        PRE.apply("flip_x", host)
    with pytest.raises(U.UNetError, match="device tensor"):
        PRE.normalize_(host)
    with pytest.raises(U.UNetError) as e:
        PRE.run_preproc(host, "gaussian_filter+blur")
    assert str(e.value) == "unknown command blur"
    assert PRE.result_shape("downsampling", (2, 41, 70, 61)) == (2, 21, 35, 31)
    assert PRE.result_shape("swap_xz", (2, 41, 70, 61)) == (2, 61, 70, 41)
    assert PRE.result_shape("gaussian_filter", (2, 41, 70, 61)) == (2, 41, 70, 61)
