"""CPU: which kernel every launcher of the pre-processing chain takes, from the host functions the launchers themselves switch on
(bbocr_host_pp_*_route), and the reference of the fused UnsharpMask kernels' edge cases against Pillow itself.

* over H, W in [1, 40] + {64, 127, 128, 129, 511, 512, 4095, 4096} and all 16 pairs of pointer bits every function returns members of its
  own part of the enum only, and never a dword route for a misaligned pointer or a W % 4 != 0 plane;
* the thresholds the launchers document sit where the rows of tests/preproc_cases.py assume them;
* every row of the GPU test's table takes the routes it names, and the table reaches every member of the enum;
* oracle.preprocess.pil_unsharp_L equals PIL.ImageFilter.UnsharpMask on both planes of every unsharp row.
"""
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import preproc_cases as pc  # noqa: E402

SIZES = list(range(1, 41)) + [64, 127, 128, 129, 511, 512, 4095, 4096]
BITS = list(itertools.product(range(4), range(4)))
# dword kernels that index the plane by rows: W % 4 == 0 and aligned pointers.  UNSHARP_PASSES_VEC is not among them on purpose: its
# combine runs flat over the H * W bytes (dwords + a byte tail), so it asks for aligned pointers only
ROW_VECTOR = {"GAUSS_X4", "HIST_X4", "APPLY_CELL_2", "APPLY_CELL_8", "APPLY_CELL_32", "APPLY_VEC", "BOX0_X4", "UNSHARP_FUSED"}
FLAT_VECTOR = {"UNSHARP_PASSES_VEC"}


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def ids():
    from bb_ocr_amd import _lib

    return _lib.PP_ROUTE_IDS


def test_header_and_binding_agree(ids):
    from bb_ocr_amd import _lib

    header = open(os.path.join(ROOT, "include", "bbocr.h")).read()
    enum = header[header.index("BBOCR_PP_GAUSS_X4 = 0"):header.index("BBOCR_PP_ROUTE_COUNT")]
    names = re.findall(r"BBOCR_PP_([A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert tuple(names) == ids
    parts = [n for names in _lib.PP_ROUTES_OF.values() for n in names]
    assert sorted(parts) == sorted(ids), "PP_ROUTES_OF splits the enum: every member in exactly one part"


def _sweep(lib, ids, key, fn, with_dst=True):
    """fn(H, W, src_bits, dst_bits) -> id or BBOCR_ERR_ARG; -> {(H, W, sb, db): name} of the accepted arguments"""
    from bb_ocr_amd import _lib

    allowed, got = set(_lib.PP_ROUTES_OF[key]), {}
    for H in SIZES:
        for W in SIZES:
            for sb, db in BITS if with_dst else [(s, 0) for s in range(4)]:
                r = fn(H, W, sb, db)
                if r == -1:
                    continue
                assert 0 <= r < len(ids) and ids[r] in allowed, (key, H, W, sb, db, r)
                name = ids[r]
                if name in ROW_VECTOR:
                    assert W % 4 == 0 and sb == 0 and db == 0, (key, H, W, sb, db, name)
                if name in FLAT_VECTOR:
                    assert sb == 0 and db == 0, (key, H, W, sb, db, name)
                got[(H, W, sb, db)] = name
    assert set(got.values()) == allowed, f"{key}: the sweep never reaches {allowed - set(got.values())}"
    return got


def test_gauss_routes(lib, ids):
    got = _sweep(lib, ids, "gauss", lib.bbocr_host_pp_gauss_route)
    assert len(got) == len(SIZES) ** 2 * 16
    for (H, W, sb, db), name in got.items():
        assert (name == "GAUSS_X4") == (W % 4 == 0 and W >= 8 and sb == 0 and db == 0)


def test_clahe_routes(lib, ids):
    def tiles(H, W):                                            # clahe.cpp pads both axes as soon as one does not divide the 8 x 8 grid
        pad = H % 8 or W % 8
        EH, EW = (H + 8 - H % 8, W + 8 - W % 8) if pad else (H, W)
        return None if EH - H >= H or EW - W >= W else (EH // 8, EW // 8)

    hist = _sweep(lib, ids, "clahe_hist", lambda H, W, sb, db: lib.bbocr_host_pp_clahe_hist_route(H, W, sb), with_dst=False)
    apply_ = _sweep(lib, ids, "clahe_apply", lib.bbocr_host_pp_clahe_apply_route)
    for H in SIZES:
        for W in SIZES:
            t = tiles(H, W)
            assert ((H, W, 0, 0) in hist) == ((H, W, 0, 0) in apply_) == (t is not None), (H, W)
            if t is None:
                continue
            assert (hist[(H, W, 0, 0)] == "HIST_X4") == (W % 4 == 0)
            if W % 4:
                want = "APPLY_BYTE"
            elif H * W < 1 << 14:
                want = "APPLY_VEC"
            else:
                want = "APPLY_CELL_32" if t[0] >= 512 else ("APPLY_CELL_8" if t[0] >= 64 else "APPLY_CELL_2")
            assert apply_[(H, W, 0, 0)] == want, (H, W, t)
            assert all(apply_[(H, W, sb, db)] == "APPLY_BYTE" for sb, db in BITS if sb or db)
    for H, W in pc.CLAHE_REFUSED:
        assert lib.bbocr_host_pp_clahe_hist_route(H, W, 0) == -1 and lib.bbocr_host_pp_clahe_apply_route(H, W, 0, 0) == -1


def test_box_and_unsharp_routes(lib, ids):
    assert lib.bbocr_host_pp_unsharp_box_radius(1.0) == 0 and lib.bbocr_host_pp_unsharp_box_radius(2.0) == 1
    for r in (0, 1):
        got = _sweep(lib, ids, "box", lambda H, W, sb, db: lib.bbocr_host_pp_box_route(H, W, r, sb, db)) if r == 0 else {
            k: ids[lib.bbocr_host_pp_box_route(k[0], k[1], r, k[2], k[3])] for k in itertools.product((1, 8, 64), (4, 8, 9), range(4), range(4))}
        for (H, W, sb, db), name in got.items():
            assert (name == "BOX0_X4") == (r == 0 and W % 4 == 0 and sb == 0 and db == 0)
    got = _sweep(lib, ids, "unsharp", lambda H, W, sb, db: lib.bbocr_host_pp_unsharp_route(H, W, 1.0, sb, db))
    for (H, W, sb, db), name in got.items():
        want = "UNSHARP_PASSES_BYTE" if sb or db else ("UNSHARP_FUSED" if W % 4 == 0 else "UNSHARP_PASSES_VEC")
        assert name == want, (H, W, sb, db)
    for H, W, sb, db in itertools.product((1, 17), (4, 8, 9), range(4), range(4)):      # box radius 1: never fused
        assert ids[lib.bbocr_host_pp_unsharp_route(H, W, 2.0, sb, db)] == ("UNSHARP_PASSES_BYTE" if sb or db else "UNSHARP_PASSES_VEC")


def test_resize_routes(lib, ids):
    from bb_ocr_amd import _lib

    allowed, seen = set(_lib.PP_ROUTES_OF["resize"]), set()
    scales = (0.25, 0.3, 0.5, 0.52, 0.55, 0.6, 0.7, 0.8, 1.0, 1.02, 1.04, 1.05, 1.1, 1.5, 2.0, 3.0)
    for H in SIZES:
        for W in SIZES:
            for sy in scales:
                for sx in (sy, 1.0, 1.5):
                    dh, dw = max(1, int(H * sy)), max(1, int(W * sx))
                    r = lib.bbocr_host_pp_resize_route(H, W, dh, dw)
                    assert 0 <= r < len(ids) and ids[r] in allowed, (H, W, dh, dw, r)
                    # a tile's source window must fit the kernel's LDS window: 128 columns, 36 rows
                    if ids[r] != "RESIZE_PIXEL":
                        th = 32 if ids[r] == "RESIZE_TILED32" else 16
                        assert -(-64 * W // dw) + 4 <= 128 and -(-th * H // dh) + 4 <= 36, (H, W, dh, dw, ids[r])
                    seen.add(ids[r])
    assert seen == allowed
    for n, want in pc.RESIZE_BOUNDARIES:
        assert ids[lib.bbocr_host_pp_resize_route(40, 40, n, n)] == want, n
    assert lib.bbocr_host_pp_resize_route(0, 4, 4, 4) == -1
    for dw in SIZES:
        for db in range(4):
            assert lib.bbocr_host_pp_resize_dword_rows(dw, db) == int(dw % 4 == 0 and db == 0)
    assert lib.bbocr_host_pp_resize_dword_rows(0, 0) == -1 and lib.bbocr_host_pp_resize_dword_rows(8, 4) == -1


def test_bad_arguments(lib):
    assert lib.bbocr_host_pp_gauss_route(0, 8, 0, 0) == -1 and lib.bbocr_host_pp_gauss_route(8, 8, 4, 0) == -1
    assert lib.bbocr_host_pp_gauss_route(8, 8, 0, -1) == -1 and lib.bbocr_host_pp_box_route(8, 8, -1, 0, 0) == -1
    assert lib.bbocr_host_pp_unsharp_route(8, 8, 0.0, 0, 0) == -1 and lib.bbocr_host_pp_clahe_hist_route(8, 8, 4) == -1


# ---------------------------------------------------------------------------------------------------- the GPU test's table
@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_rows_take_the_routes_they_name(lib, ids, group):
    for c in pc.GROUPS[group]:
        assert 0 <= c.so <= 3 and 0 <= c.do <= 3 and c.H * c.W <= 4097 * 12
        assert pc.routes_reported(lib, ids, c) == c.routes, c


def test_coverage_of_the_route_enum(ids):
    reached = {r for c in pc.ALL_CASES for r in c.routes.values() if isinstance(r, str)}
    # the tiled resize's stores: whole dwords, refused for a misaligned destination, refused for dw % 4 != 0
    assert {(c.dw % 4 == 0, c.do, c.routes["resize_dword_rows"]) for c in pc.GROUPS["resize"] if "resize_dword_rows" in c.routes} >= {
        (True, 0, 1), (True, 1, 0), (False, 0, 0)}
    assert reached == set(ids), f"route ids no row reaches: {sorted(set(ids) - reached)}; unknown: {sorted(reached - set(ids))}"
    # and the edges the fused UnsharpMask kernels fix up
    fused = {(c.H, c.W) for c in pc.UNSHARP_CASES if c.routes["unsharp"] == "UNSHARP_FUSED"}
    assert {(H, W) for H in pc.UNSHARP_H for W in (4, 8, 12)} | {(1, 1028), (17, 1028)} <= fused
    tails = {(c.H * c.W) & 3 for c in pc.UNSHARP_CASES if c.routes["unsharp"] == "UNSHARP_PASSES_VEC"}
    assert tails == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------- the reference of the unsharp rows
def test_unsharp_reference_equals_pillow():
    from PIL import Image, ImageFilter

    from oracle import preprocess as pp

    done, wrong = set(), 0
    for c in pc.UNSHARP_CASES:
        radius, percent = pc.unsharp_args(c)
        key = (c.H, c.W, radius, percent)
        if key in done:
            continue
        done.add(key)
        for name, a in pc.planes(c).items():
            want = np.asarray(Image.fromarray(a).filter(ImageFilter.UnsharpMask(radius=radius, percent=percent, threshold=3)))
            wrong += int((pp.pil_unsharp_L(a, radius, percent, 3) != want).sum())
    # 33 fused shapes (W = 8 serves the misaligned rows too) + 2 wide + 9 + 2 with a tail, each at three settings, + 3 shapes at radius 2
    assert len(done) == 46 * 3 + 3 and wrong == 0, (len(done), wrong)
