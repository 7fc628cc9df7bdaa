"""CPU: the crop planner (recognizer.cpp: plan_sizes, plan_horizontal, plan_free, crop_refit_fw; boxpost.cpp: perspective_inverse) through
bbocr_host_crop_plan against oracle/recog.py, as hypothesis properties with a derandomised seed.  Everything is compared exactly; the
perspective matrices bit for bit (their products are rounded to 1/32 pixel by the warp, so one differing bit can move a sample).

The oracle's pixel work is stubbed out (cv2.resize, warpPerspective and the Pillow resize return, or report, only their sizes): the planner is
about geometry, and a 1 x 3000 box resizes to 64 x 192000."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crop_cases as cc  # noqa: E402

SETTINGS = dict(deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


class _ResizedTo(Exception):
    pass


@pytest.fixture()
def sizes_only(monkeypatch):
    """the oracle with its three resamplers reduced to their sizes; warps: the (M, (w, h)) of every warpPerspective call"""
    from oracle import imgproc, recog

    warps = []
    blank = lambda h, w: np.broadcast_to(np.uint8(0), (int(h), int(w)))

    def warp(src, M, dsize_wh):
        warps.append((M, (int(dsize_wh[0]), int(dsize_wh[1]))))
        return blank(dsize_wh[1], dsize_wh[0])

    def pil_resize(img, dsize_wh):
        raise _ResizedTo(int(dsize_wh[0]))

    monkeypatch.setattr(imgproc, "resize_linear_u8", lambda src, dsize_wh: blank(dsize_wh[1], dsize_wh[0]))
    monkeypatch.setattr(imgproc, "pil_resize_bicubic_u8", pil_resize)
    monkeypatch.setattr(recog, "warp_perspective_u8", warp)
    return warps


def _resized_w(crop, imgW):
    """AlignCollate's resized_w"""
    from oracle import recog

    try:
        recog.align_collate_one(crop, 64, imgW)
    except _ResizedTo as e:
        return e.args[0]
    raise AssertionError("AlignCollate did not reach its resize")


def _plan(lib, H, W, hori, free):
    n = len(hori) + len(free)
    harr = (C.c_int * max(1, 4 * len(hori)))(*[int(v) for b in hori for v in b])
    farr = (C.c_double * max(1, 8 * len(free)))(*[float(v) for q in free for p in q for v in p])
    taken, geom, minv = (C.c_int * n)(), (C.c_int * (9 * n))(), (C.c_double * (9 * n))()
    assert lib.bbocr_host_crop_plan(H, W, harr, len(hori), farr, len(free), taken, geom, minv) == 0
    keys = ("sx0", "sy0", "sw", "sh", "rw", "rh", "fw", "imgW", "warp")
    return [(bool(taken[k]), dict(zip(keys, geom[9 * k:9 * k + 9])), np.array(minv[9 * k:9 * k + 9], dtype=np.float64)) for k in range(n)]


_PAGE = np.zeros((3000, 3000), dtype=np.uint8)


@st.composite
def _hori_case(draw):
    H, W = draw(st.integers(1, 3000)), draw(st.integers(1, 3000))
    kind = draw(st.sampled_from(["inside", "left", "right", "top", "bottom", "thin_w", "thin_h", "multiple", "large", "any"]))
    w, h = draw(st.integers(1, 400)), draw(st.integers(1, 400))
    if kind == "thin_w":
        w = 1
    elif kind == "thin_h":
        h = 1
    elif kind == "multiple":
        h = draw(st.integers(1, 100))
        w = h * draw(st.integers(1, 30))
        if draw(st.booleans()):
            w, h = h, w
    elif kind == "large":
        w, h = draw(st.integers(1, 3000)), draw(st.integers(1, 3000))
    x, y = draw(st.integers(0, max(0, W - w))), draw(st.integers(0, max(0, H - h)))
    if kind == "left":
        x = -draw(st.integers(1, w + 2))
    elif kind == "right":
        x = W - draw(st.integers(-2, w))
    elif kind == "top":
        y = -draw(st.integers(1, h + 2))
    elif kind == "bottom":
        y = H - draw(st.integers(-2, h))
    elif kind == "any":
        x, y = draw(st.integers(-500, 3400)), draw(st.integers(-500, 3400))
    return H, W, [x, x + w, y, y + h]


@settings(max_examples=1200, **SETTINGS)
@given(case=_hori_case())
def test_horizontal_boxes(lib, sizes_only, case):
    """the clamped rectangle, the resize target, the own padded width and AlignCollate's content width of a horizontal box; a box that is
    empty after clamping (the oracle raises there) is reported as not taken"""
    from oracle import recog

    H, W, box = case
    (taken, g, _), = _plan(lib, H, W, [box], [])
    try:
        il, max_width = recog.get_image_list([box], [], _PAGE[:H, :W])
    except ValueError:
        assert not taken and min(cc.clamped(box, H, W)[2:]) <= 0, case
        return
    assert taken == (len(il) == 1), (case, g)
    if not taken:
        return
    quad, crop = il[0]
    assert (g["sx0"], g["sy0"], g["sw"], g["sh"]) == (quad[0][0], quad[0][1], quad[2][0] - quad[0][0], quad[2][1] - quad[0][1]) == cc.clamped(box, H, W), case
    assert (g["rh"], g["rw"]) == crop.shape and g["imgW"] == max_width and g["warp"] == 0, (case, g, crop.shape, max_width)
    assert g["fw"] == _resized_w(crop, max_width), (case, g)
    assert (g["rw"], g["rh"], g["imgW"], g["fw"]) == cc.plan_sizes(g["sw"], g["sh"]), (case, g)       # the test suite's own classifier agrees


@st.composite
def _free_case(draw):
    kind = draw(st.sampled_from(["plain", "plain", "quarter", "leaving", "sliver"]))
    f = lambda lo, hi: draw(st.floats(lo, hi, allow_nan=False, allow_infinity=False, width=64))
    w, h = f(4.0, 400.0), f(4.0, 200.0)
    if draw(st.booleans()):
        w, h = h, w
    if kind == "sliver":
        if draw(st.booleans()):
            w = f(0.05, 1.5)
        else:
            h = f(0.05, 1.5)
    cx, cy = (f(-60.0, 480.0), f(-60.0, 360.0)) if kind == "leaving" else (f(0.0, 420.0), f(0.0, 300.0))
    jitter = tuple((f(-1.5, 1.5), f(-1.5, 1.5)) for _ in range(4)) if kind != "sliver" else ()
    quad = cc._rot_quad(cx, cy, w, h, f(-90.0, 90.0), jitter=jitter, shear=f(-0.3, 0.3))
    if kind == "quarter":
        quad = [[round(v * 4) / 4 for v in p] for p in quad]
    return quad


@settings(max_examples=1000, **SETTINGS)
@given(quad=_free_case())
def test_free_quads(lib, sizes_only, quad):
    """a free box is skipped exactly when the oracle drops it; else its warp size, the inverted perspective matrix (bit for bit) and the
    sizes derived from the warp are the oracle's"""
    from oracle import recog

    (taken, g, minv), = _plan(lib, cc.H, cc.W, [], [quad])
    del sizes_only[:]
    il, max_width = recog.get_image_list([], [quad], _PAGE[:cc.H, :cc.W])
    (M, (mw, mh)), = sizes_only
    assert (mw, mh) == cc.free_size(quad)
    assert taken == (len(il) == 1), (quad, g, (mw, mh))
    if not taken:
        assert mw <= 0 or mh <= 0
        return
    crop = il[0][1]
    assert (g["sx0"], g["sy0"], g["sw"], g["sh"], g["warp"]) == (0, 0, mw, mh, 1), (quad, g)
    want = recog.invert3x3(M).reshape(9)
    assert np.array_equal(minv.view(np.int64), want.view(np.int64)), (quad, minv.tolist(), want.tolist())
    assert (g["rh"], g["rw"]) == crop.shape and g["imgW"] == max_width, (quad, g, crop.shape, max_width)
    assert g["fw"] == _resized_w(crop, max_width), (quad, g)


def test_degenerate_boxes_are_not_taken(lib, sizes_only):
    """boxes on which the oracle raises (empty after clamping) or that it drops come back as not taken, with zeroed outputs, between boxes
    that are taken; bad arguments are refused"""
    from oracle import recog

    H, W = 50, 80
    hori = [[10, 30, 5, 25], [80, 120, 5, 25], [-30, 0, 5, 25], [10, 30, 50, 70], [10, 30, -9, 0], [30, 10, 5, 25], [10, 10, 5, 25], [0, 80, 0, 50]]
    free = [[[5.0, 5.0], [5.5, 5.0], [5.5, 30.0], [5.0, 30.0]], [[5.0, 5.0], [40.0, 5.0], [40.0, 5.9], [5.0, 5.9]], [[5.0, 5.0], [40.0, 6.0], [39.0, 20.0], [4.0, 19.0]]]
    got = _plan(lib, H, W, hori, free)
    assert [t for t, _, _ in got] == [True, False, False, False, False, False, False, True, False, False, True]
    for b, (t, g, minv) in zip(hori, got):
        if t:
            continue
        with pytest.raises(ValueError):
            recog.get_image_list([b], [], _PAGE[:H, :W])
        assert not any(g.values()) and not minv.any()
    for q, (t, g, minv) in zip(free, got[len(hori):]):
        assert t == (len(recog.get_image_list([], [q], _PAGE[:H, :W])[0]) == 1)
    one, tk = (C.c_int * 9)(), (C.c_int * 1)()
    d9 = (C.c_double * 9)()
    box = (C.c_int * 4)(1, 2, 1, 2)
    assert lib.bbocr_host_crop_plan(0, 10, box, 1, None, 0, tk, one, d9) != 0
    assert lib.bbocr_host_crop_plan(10, 10, None, 1, None, 0, tk, one, d9) != 0
    assert lib.bbocr_host_crop_plan(10, 10, box, 1, None, 0, None, one, d9) != 0
    assert lib.bbocr_host_crop_plan(10, 10, box, -1, None, 0, tk, one, d9) != 0
    assert lib.bbocr_host_crop_plan(10, 10, box, 1, None, 0, tk, one, d9) == 0 and tk[0] == 1 and one[4] == 64
