"""CPU: the host half of the tiled evaluation (include/unet_tiles.h, unet-studio_amd/tiles.py) -- the plan's known answers and its
properties over a sweep, the canvas, the weights, the ABI the library exports, the argument errors of both entry points found
before any device call, and the refusals of EvaluateUNet that need no device.  No device calls."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import tiles as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,ov,origins", [(129, 128, .25, [0, 1]), (228, 128, .25, [0, 50, 100]), (320, 128, .25, [0, 96, 192]),
                                            (13, 8, .25, [0, 5]), (15, 8, .25, [0, 4, 7]), (17, 8, 0, [0, 5, 9]),
                                            (8, 8, .25, [0]), (37, 16, .25, [0, 11, 21]), (18, 16, .25, [0, 2]), (30, 16, .25, [0, 7, 14])])
def test_plan_known_answers(C, T, ov, origins):
    assert TL.plan_axis(C, T, ov) == origins


def test_plan_properties_over_the_sweep():
    for ov in (0, .1, .25, .4, .49):
        for T in range(2, 40):
            S = T - int(math.ceil(ov * T))
            for C in range(T, 6 * T):
                o = TL.plan_axis(C, T, ov)
                n = len(o)
                assert all(isinstance(v, int) for v in o)
                assert o[0] == 0 and o[-1] == C - T, (C, T, ov)
                assert all(0 < b - a <= S for a, b in zip(o, o[1:])), (C, T, ov, o)
                # n is minimal: n - 1 steps of at most S cannot reach C - T with one tile less
                assert n == 1 or (n - 2) * S < C - T, (C, T, ov, o)
                assert (n == 1) == (C == T)
                cover = np.zeros(C, int)
                for a in o:
                    cover[a:a + T] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (C, T, ov, o)


def test_plan_tiles_and_its_refusals():
    plan = TL.plan_tiles((37, 18, 30), (16, 16, 16), 0.25)
    assert plan == ([0, 11, 21], [0, 2], [0, 7, 14])
    org = TL.tile_origins(plan)
    assert len(org) == 18 and org[0] == (0, 0, 0) and org[1] == (11, 0, 0) and org[3] == (0, 2, 0) and org[-1] == (21, 2, 14)
    assert org[(2 * 2 + 1) * 3 + 1] == (11, 2, 14)                  # (iz*ny + iy)*nx + ix
    assert TL.plan_tiles((16, 16, 16), (16, 16, 16)) == ([0], [0], [0])
    assert len(TL.plan_axis(8 + 15 * 6, 8, 0.25)) == 16
    with pytest.raises(U.UNetError, match="at most 16"):
        TL.plan_axis(8 + 15 * 6 + 1, 8, 0.25)
    with pytest.raises(U.UNetError, match="does not hold"):
        TL.plan_axis(7, 8, 0.25)
    for bad in (0.5, -0.1, 1, float("nan"), "x", None):
        with pytest.raises(U.UNetError, match="tile_overlap"):
            TL.plan_axis(20, 8, bad)
    with pytest.raises(U.UNetError, match="above 512"):
        TL.plan_tiles((600, 600, 600), (513, 16, 16))
    with pytest.raises(U.UNetError, match="whole numbers"):
        TL.plan_tiles((37.5, 18, 30), (16, 16, 16))


# ---- the canvas ------------------------------------------------------------------------------------------------------------------
def test_canvas_dims():
    assert TL.canvas_dims((16, 16, 16), (1, 1, 1), (37, 18, 30), (1, 1, 1)) == (37, 18, 30)
    assert TL.canvas_dims((16, 16, 16), (1, 1, 1), (14, 15, 16), (1, 1, 1)) == (16, 16, 16)        # it fits: the model's grid
    assert TL.canvas_dims((16, 16, 16), (1, 1, 1), (37, 18, 30), (0.9, 1.1, 1.0)) == (34, 20, 30)  # 33.3 -> 34, 19.8 -> 20
    assert TL.canvas_dims((16, 16, 16), (2, 2, 2), (37, 18, 30), (1, 1, 1)) == (19, 16, 16)        # 18.5 -> 19, 9 and 15 -> 16
    # a ratio within 1e-6 of an integer is that integer: 18 * 1.3 / 0.6 is 39.00000000000001 in float64
    assert 18 * 1.3 / 0.6 > 39 and TL.canvas_dims((16, 16, 16), (0.6, 1, 1), (18, 16, 16), (1.3, 1, 1)) == (39, 16, 16)
    assert TL.canvas_dims((16, 16, 16), (1, 1, 1), (20, 16, 16), (1 + 4e-8, 1, 1)) == (20, 16, 16)
    assert TL.canvas_dims((16, 16, 16), (1, 1, 1), (20, 16, 16), (1 + 1e-6, 1, 1)) == (21, 16, 16)  # 2e-5 over: rounded up
    # an orientation with a swap: the extents are taken in the frame the model -> image map is computed in (D0, vs0) ...
    D0, vs0, _ = U.preproc.orientation_map("swap_xy+flip_z", (16, 24, 8), (1, 2, 3))
    assert D0 == (24, 16, 8) and vs0 == (2, 1, 3)
    # ... image 100 x 20 x 30 at 1 mm there: 50, 20, 10 against D0 -> (50, 20, 10), swapped back to the model's frame
    assert TL.canvas_dims((16, 24, 8), (1, 2, 3), (100, 20, 30), (1, 1, 1), orientation="swap_xy+flip_z") == (20, 50, 10)
    assert TL.canvas_dims((16, 24, 8), (1, 2, 3), (100, 20, 30), (1, 1, 1), orientation=["flip_x"]) == (100, 24, 10)
    cD0 = U.preproc.orientation_map("swap_xy+flip_z", (20, 50, 10), (1, 2, 3))[0]
    assert cD0 == (50, 20, 10)                                       # the canvas's own D0 is the extent frame again
    with pytest.raises(U.UNetError, match="unknown command"):
        TL.canvas_dims((16, 16, 16), (1, 1, 1), (20, 16, 16), (1, 1, 1), orientation="swap_xw")
    with pytest.raises(U.UNetError, match="image_vs"):
        TL.canvas_dims((16, 16, 16), (1, 1, 1), (20, 16, 16), (1, 0, 1))


def test_weights():
    assert TL.weights(8).tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and TL.weights(5).tolist() == [1, 2, 3, 2, 1]
    assert TL.weights(1).tolist() == [1] and TL.weights(8).dtype == np.float32
    w = TL.weights(512).astype(np.float64)
    assert w.max() == 256 and np.float32(w.max() ** 3) == w.max() ** 3 == 2 ** 24      # the product stays exact in fp32


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_unet_tiles_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_tiles.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(TL.EXPORTS) == {"unet_tiles_blend", "unet_tiles_postproc"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    assert int(re.search(r"#define UNET_TILES_MAX_AXIS (\d+)", hdr).group(1)) == TL.TILES_MAX_AXIS == 16
    assert int(re.search(r"#define UNET_TILES_MAX_DIM (\d+)", hdr).group(1)) == TL.TILES_MAX_DIM == 512
    assert ctypes.sizeof(TL.UnetTilePlan) == 4 * (3 + 3 * 16)
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.tiles is TL and U.plan_tiles is TL.plan_tiles and U.canvas_dims is TL.canvas_dims
    for h in ("unet_hip.h", "unet_postproc.h", "unet_space.h", "unet_preproc.h"):
        assert "unet_tiles_" not in open(os.path.join(ROOT, "include", h)).read()


def test_argument_errors_need_no_device():
    fake = ctypes.c_void_p(0x1000)      # never dereferenced
    lib = U.engine.lib
    f = ctypes.c_float(0.5)

    def plan(x=(0, 5), y=(0,), z=(0, 4, 7), n=None):
        s = TL.UnetTilePlan()
        for a, o in enumerate((x, y, z)):
            s.n[a] = len(o) if n is None else n[a]
            for i, v in enumerate(o):
                s.origin[a][i] = v
        return ctypes.byref(s)

    def err(rc):
        assert rc != 0
        return lib.unet_last_error().decode()

    # tile 8 x 6 x 5, canvas 13 x 6 x 12: x [0, 5], y [0], z [0, 4, 7]
    def blend(tiles=fake, c=3, t=(8, 6, 5), p=None, cv=(13, 6, 12), canvas=fake):
        return lib.unet_tiles_blend(tiles, c, t[0], t[1], t[2], p if p is not None else plan(), cv[0], cv[1], cv[2], canvas, None)

    def post(tiles=fake, c=3, t=(8, 6, 5), p=None, cv=(13, 6, 12), lp=None, fg=None, lab=fake):
        return lib.unet_tiles_postproc(tiles, c, t[0], t[1], t[2], p if p is not None else plan(), cv[0], cv[1], cv[2], f, lp, fg, lab, None)

    for call, who in ((blend, "unet_tiles_blend"), (post, "unet_tiles_postproc")):
        assert who + ": null tiles" in err(call(tiles=None))
        assert "null plan" in err(call(p=ctypes.POINTER(TL.UnetTilePlan)()))
        assert "at least 2" in err(call(c=1))
        assert "65535" in err(call(c=65537))
        assert "tile dimensions must be positive" in err(call(t=(8, 0, 5)))
        assert "canvas dimensions must be positive" in err(call(cv=(13, 6, -1)))
        assert "above 512" in err(call(t=(513, 6, 5), cv=(513, 6, 12), p=plan(x=(0,))))
        assert "2^31" in err(call(t=(512, 512, 512), cv=(2048, 1024, 1024), p=plan(x=(0,), y=(0,), z=(0,))))
        assert "axis x: n must be in [1, 16], got 0" in err(call(p=plan(n=(0, 1, 3))))
        assert "axis z: n must be in [1, 16], got 17" in err(call(p=plan(n=(2, 1, 17))))
        assert "axis x: the first origin must be 0" in err(call(p=plan(x=(1, 5))))
        assert "axis x: the last origin must be canvas - tile = 5" in err(call(p=plan(x=(0, 4))))
        assert "axis y: the last origin must be canvas - tile = 1" in err(call(cv=(13, 7, 12)))
        assert "axis z: the origins must ascend" in err(call(p=plan(z=(0, 4, 4, 7))))
        assert "axis z: the origins must ascend" in err(call(p=plan(z=(0, 5, 4, 7))))
        assert "axis z: a gap between tiles 0 and 1" in err(call(p=plan(z=(0, 6, 7))))
        assert "axis x: a gap between tiles 0 and 1" in err(call(p=plan(x=(0, 9)), cv=(17, 6, 12)))
    assert "null canvas" in err(blend(canvas=None))
    assert "no output wanted" in err(post(lab=None))


def test_wrapper_errors_need_no_device():
    host = np.zeros((2, 3, 5, 6, 8), np.float32)
    plan = ([0, 5], [0], [0])
    with pytest.raises(U.UNetError, match="device tensor"):
        TL.blend(host, plan, (5, 6, 13))
    with pytest.raises(U.UNetError, match="three lists"):
        TL.blend(host, ([0, 5], [0]), (5, 6, 13))
    with pytest.raises(U.UNetError, match=r"axis x: n must be in \[1, 16\], got 17"):
        TL.blend(host, (list(range(17)), [0], [0]), (5, 6, 13))
    with pytest.raises(U.UNetError, match="canvas_shape"):
        TL.blend(host, plan, (5, 6))
    with pytest.raises(U.UNetError, match="unknown output mask"):
        TL.postproc_tiles(host, plan, (5, 6, 13), outputs=("mask",))
    with pytest.raises(U.UNetError, match="no output wanted"):
        TL.postproc_tiles(host, plan, (5, 6, 13), outputs=())
    with pytest.raises(U.UNetError, match="device tensor"):
        TL.postproc_tiles(host, plan, (5, 6, 13))
    with pytest.raises(U.UNetError, match="in place of logits"):
        U.run_postproc(host, "softmax", outputs=("label_prob",), tiles=(host, plan, (5, 6, 13)))
    with pytest.raises(U.UNetError, match="device tensor"):
        U.run_postproc(None, "softmax", outputs=("label_prob",), tiles=(host, plan, (5, 6, 13)))


# ---- EvaluateUNet's refusals that need no device -----------------------------------------------------------------------------------
class FakeModel:
    """what EvaluateUNet reads of a model before the first upload"""
    in_count, out_count = 1, 3
    dim, voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    postproc, preproc, orientation, fov_strategy = "softmax+create_mask+argmax", "", "", "align_top"
    single_component_label = []
    prepared = 0

    def device(self):
        return "cpu"

    def prepare_for_inference(self, device):
        self.prepared += 1

    def forward(self, x, packs_current=False):
        raise AssertionError("the forward was reached")


def test_evaluate_refusals_need_no_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: None)     # start() makes its copy stream first
    m = FakeModel()
    marker = np.zeros((16, 16, 16), np.float32)

    def start(ios, **kw):
        ev = U.EvaluateUNet(m, device="cpu", **kw)
        return ev, ev.start(ios)

    ev, out = start([[marker]], fov_strategy="spiral")
    assert ev.aborted and ev.error_msg == "unknown fov_strategy spiral" and not ev.running and out[0][0] is marker
    m.fov_strategy = "pyramid"
    ev, out = start([[marker]], fov_strategy="model")
    assert ev.aborted and ev.error_msg == "unknown fov_strategy pyramid" and out[0][0] is marker
    m.fov_strategy = "align_top"
    for bad in (0.5, -0.01, float("nan"), "a lot"):
        ev, out = start([[marker]], fov_strategy="tiles", tile_overlap=bad)
        assert ev.aborted and "tile_overlap must be in [0, 0.5)" in ev.error_msg and out[0][0] is marker
    # without "tiles" in force the overlap is not looked at, as the model's fov_strategy is not without "model"
    m.fov_strategy = "pyramid"
    nv = U.NativeVolume(np.zeros((30, 18, 37), np.float32), (1, 1, 1), map=(np.eye(3).reshape(9), np.zeros(3)))
    small = np.zeros((16, 15, 16), np.float32)
    ev, out = start([[nv], [marker]], fov_strategy="tiles")
    assert ev.aborted and "a caller's map and tiles do not combine" in ev.error_msg and ev.cur_prog == 0 and out[1][0] is marker
    ev, out = start([[small], [marker]], fov_strategy="tiles")
    assert ev.aborted and "smaller than the model's" in ev.error_msg and ev.cur_prog == 0 and out[1][0] is marker
    m.fov_strategy = "tiles"
    ev, out = start([[small], [marker]], fov_strategy="model")
    assert ev.aborted and "smaller than the model's" in ev.error_msg and out[1][0] is marker
