"""CPU: bbocr_host_pages_plan, the planning function bbocr_readtext_pages runs (no device is touched: the page pointers are only compared
with NULL, so any non-zero value stands in for a device address)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def _pages(shapes, rgb=0x1000, pitch=None):
    from bb_ocr_amd import _lib

    arr = (_lib.bbocr_page * max(1, len(shapes)))()
    for k, (H, W) in enumerate(shapes):
        arr[k].dev_rgb, arr[k].H, arr[k].W = rgb, H, W
        if pitch is not None:
            arr[k].rgb_pitch = pitch
    return arr


def _plan(lib, shapes, params=None, arr=None):
    n = len(shapes)
    arr = _pages(shapes) if arr is None else arr
    grp, slot = (C.c_int * max(1, n))(), (C.c_int * max(1, n))()
    ro, go = (C.c_longlong * max(1, n))(), (C.c_longlong * max(1, n))()
    ng, sb = C.c_int(), (C.c_longlong * 2)()
    rc = lib.bbocr_host_pages_plan(arr, n, params, grp, slot, ro, go, C.byref(ng), sb)
    return rc, list(grp)[:n], list(slot)[:n], list(ro)[:n], list(go)[:n], ng.value, list(sb)


def _check_plan(shapes, grp, slot, ro, go, ng, sb):
    n = len(shapes)
    # every page in exactly one group, groups numbered by first appearance, pages of a group share (H, W) -- and equal shapes one group
    assert all(0 <= g < ng for g in grp) and sorted(set(grp)) == list(range(ng))
    first_seen = []
    for g in grp:
        if g not in first_seen:
            first_seen.append(g)
    assert first_seen == list(range(ng))
    shape_of = {}
    for i in range(n):
        assert shape_of.setdefault(grp[i], shapes[i]) == shapes[i]
    assert len(set(shape_of.values())) == ng == len(set(shapes))
    # slot_in_group: a permutation of 0 .. nb - 1 inside each group that keeps the caller's order
    for g in range(ng):
        assert [slot[i] for i in range(n) if grp[i] == g] == list(range(grp.count(g)))
    # staging ranges: disjoint, inside staging_bytes; each group's block contiguous, [nb][H][W][c] in slot order
    for off, c, total in ((ro, 3, sb[0]), (go, 1, sb[1])):
        spans = sorted((off[i], off[i] + shapes[i][0] * shapes[i][1] * c) for i in range(n))
        assert spans[0][0] >= 0 and spans[-1][1] <= total
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for g in range(ng):
            members = [i for i in range(n) if grp[i] == g]
            base = off[members[0]]
            H, W = shapes[members[0]]
            assert base % 256 == 0
            assert [off[i] for i in members] == [base + k * H * W * c for k in range(len(members))]


def test_plan_of_seeded_random_page_lists(lib):
    rng = np.random.default_rng(20)
    A, B, Cc = (192, 320), (250, 500), (288, 416)
    cases = [[A], [A] * 5, [(200 + 8 * k, 300 + 8 * k) for k in range(7)], [A, B, A], [A, B, Cc, B, A, A, Cc]]
    for _ in range(20):
        pool = [(int(rng.integers(1, 700)), int(rng.integers(1, 700))) for _ in range(int(rng.integers(1, 6)))]
        cases.append([pool[int(rng.integers(len(pool)))] for _ in range(int(rng.integers(1, 40)))])
    for shapes in cases:
        rc, grp, slot, ro, go, ng, sb = _plan(lib, shapes)
        assert rc == 0, shapes
        _check_plan(shapes, grp, slot, ro, go, ng, sb)
    rc, grp, slot, *_ = _plan(lib, [A, B, A])
    assert (grp, slot) == ([0, 1, 0], [0, 0, 1])
    # every output pointer is optional
    assert lib.bbocr_host_pages_plan(_pages([A, B]), 2, None, None, None, None, None, None, None) == 0


def test_plan_refuses_bad_arguments(lib):
    from bb_ocr_amd import _lib

    ok = [(192, 320), (64, 64)]
    assert _plan(lib, ok)[0] == 0
    assert _plan(lib, [])[0] == -1                                            # n <= 0
    assert lib.bbocr_host_pages_plan(_pages(ok), -3, None, None, None, None, None, None, None) == -1
    assert lib.bbocr_host_pages_plan(None, 2, None, None, None, None, None, None, None) == -1
    arr = _pages(ok)
    arr[1].dev_rgb = None
    assert _plan(lib, ok, arr=arr)[0] == -1                                   # a null dev_rgb
    for bad in ((0, 64), (64, 0), (-5, 64), (64, -1)):
        assert _plan(lib, [ok[0], bad])[0] == -1                              # H or W <= 0
    assert _plan(lib, ok, arr=_pages(ok, pitch=3 * 320 - 1))[0] == -1         # a pitch smaller than the row (page 0: 320 pixels)
    assert _plan(lib, ok, arr=_pages(ok, pitch=3 * 320))[0] == 0
    arr = _pages(ok)
    arr[0].dev_gray, arr[0].gray_pitch = 0x2000, 319
    assert _plan(lib, ok, arr=arr)[0] == -1                                   # ... also of a given gray plane
    arr[0].gray_pitch = 320
    assert _plan(lib, ok, arr=arr)[0] == 0
    # a page that collapses to zero size under canvas_size / mag_ratio: 2 x 2000 on a 256 canvas has int(2 * 0.128) = 0 rows
    p = _lib.bbocr_params()
    lib.bbocr_default_params(C.byref(p))
    assert _plan(lib, [(2, 2000)], C.byref(p))[0] == 0
    p.canvas_size = 256
    assert _plan(lib, [ok[0], (2, 2000)], C.byref(p))[0] == -1
    p.canvas_size, p.mag_ratio = 2560, 0.001
    assert _plan(lib, ok, C.byref(p))[0] == -1
