"""-m gpu: the crop stage (crnn_misc.hip: crop_warp / crop_resize / crop_hist / crop_pil_h / crop_final; recognizer.cpp's planner) through
bbocr_op_crops and bbocr_op_crops_pages on the shared cases of tests/crop_cases.py, bit exact against oracle/recog.py, in every element type
crop_final_kernel writes (bf16, fp16, the exact mode's codes).  tests/test_crop_cases_cpu.py shows that these cases reach every regime and
would see each of a list of planted defects.  A failure names the box, its regime and the first differing (row, column)."""
import ctypes as C

import numpy as np
import pytest
import torch

import crop_cases as cc

pytestmark = pytest.mark.gpu

READERS = {"bf16": "reader", "fp16": "reader_fp16", "exact": "reader_exact"}
FORCED_W = 256         # modes 1..4: below the rw of "height 1 (40x1)" (2560): the horizontal Pillow pass runs on a 64-row image


@pytest.fixture(params=sorted(READERS))
def rd(request):
    return request.param, request.getfixturevalue(READERS[request.param])


def _arrays(hori, free):
    harr = (C.c_int * max(1, 4 * len(hori)))(*[int(v) for b in hori for v in b])
    farr = (C.c_double * max(1, 8 * len(free)))(*[float(v) for q in free for p in q for v in p])
    return harr, farr


def _sentinel(n, imgW):
    """[n + 1][64][imgW] of the sentinel pattern: row n is a guard the call must leave alone"""
    return torch.full((n + 1, 64, imgW), cc.SENTINEL, dtype=torch.int16, device="cuda")


def _compare(got, wants, el, what):
    """got int16 [n + 1][64][imgW] (host) against wants = [(description, float32 [64][imgW])]"""
    g = got.numpy()
    assert (g[len(wants)] == cc.SENTINEL).all(), f"{what}: the row behind the {len(wants)} reported crops was written"
    for i, (desc, t) in enumerate(wants):
        cc.assert_same(g[i], cc.to_el(t, el), f"{what}, crop {i} = {desc}")
        assert not (g[i] == cc.SENTINEL).any(), f"{what}, crop {i} = {desc}: sentinel left"


@pytest.mark.parametrize("contrast", [0.0, 0.5])
def test_bucket_layout_every_own_width(rd, contrast):
    """mode 0: per own padded width the boxes of that bucket, in box order; skipped boxes are not counted"""
    el, reader = rd
    page = cc.make_page()
    items = cc.stage_a_cases()
    d = torch.from_numpy(page.copy()).cuda()
    harr, farr = _arrays(cc.HORI, cc.FREE)
    widths = sorted({it[1] for it in items if it})
    assert len(widths) >= 8 and sum(it is None for it in items) == len(cc.SKIPPED)
    seen = 0
    for mw in widths:
        ks = [k for k, it in enumerate(items) if it and it[1] == mw]
        out = _sentinel(len(ks), mw)
        torch.cuda.synchronize()           # the fill runs on torch's stream, the library on its own non-blocking one
        n_out = C.c_int()
        reader._check(reader._lib.bbocr_op_crops(reader._h, C.c_void_p(d.data_ptr()), cc.H, cc.W, harr, len(cc.HORI), farr, len(cc.FREE), mw, float(contrast),
                                                 C.c_void_p(out.data_ptr()), C.byref(n_out), 0))
        assert n_out.value == len(ks), f"{el}, bucket {mw}: {n_out.value} crops, the oracle keeps {len(ks)}"
        _compare(out.cpu(), [(cc.describe(k), cc.reference(k, None, contrast)) for k in ks], el, f"{el}, contrast {contrast}, bucket {mw}")
        seen += len(ks)
    assert seen == len(items) - len(cc.SKIPPED)


@pytest.mark.parametrize("contrast", [0.0, 0.5])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
@pytest.mark.parametrize("el", ["bf16", "exact"])
def test_forced_width_and_rot90(request, el, rot, contrast):
    """modes 1..4 (the batched branch rotation_info takes): every box at one forced width, as np.rot90(crop, mode - 1)"""
    reader = request.getfixturevalue(READERS[el])
    items = cc.stage_a_cases()
    ks = [k for k, it in enumerate(items) if it]
    assert any(items[k][0].shape[0] == 64 and items[k][0].shape[1] > FORCED_W for k in ks)       # a non-tall crop narrower than its rw
    d = torch.from_numpy(cc.make_page().copy()).cuda()
    harr, farr = _arrays(cc.HORI, cc.FREE)
    out = _sentinel(len(ks), FORCED_W)
    torch.cuda.synchronize()
    n_out = C.c_int()
    reader._check(reader._lib.bbocr_op_crops(reader._h, C.c_void_p(d.data_ptr()), cc.H, cc.W, harr, len(cc.HORI), farr, len(cc.FREE), FORCED_W, float(contrast),
                                             C.c_void_p(out.data_ptr()), C.byref(n_out), 1 + rot))
    assert n_out.value == len(ks)
    _compare(out.cpu(), [(cc.describe(k), cc.reference(k, FORCED_W, contrast, rot)) for k in ks], el, f"{el}, rot90 x{rot}, contrast {contrast}, width {FORCED_W}")


GUARD = 0x5A


def _pages():
    """three pages of different shapes cut from the shared page, with boxes of their own (edges crossed, a box skipped on each kind)"""
    page = cc.make_page()
    a = page                                                                # the whole page with the whole list
    b = np.ascontiguousarray(page[20:200, 30:330])                          # 180 x 300: goes to the device as a strided view between guard bytes
    c = np.ascontiguousarray(page[150:240, 250:380])                        # 90 x 130: noise | low and narrow bands
    hb = [[-4, 120, 10, 74], [200, 340, 100, 200], [10, 138, -6, 250], [40, 240, 20, 148], [300, 330, 5, 40], [5, 6, 60, 124]]
    fb = [cc._rot_quad(280.0, 170.0, 100.0, 30.0, 14.0), cc._rot_quad(8.0, 6.0, 90.0, 28.0, -25.0), [[10.0, 10.0], [10.4, 10.0], [10.4, 50.0], [10.0, 50.0]]]
    hc = [[0, 130, 0, 90], [100, 140, 60, 95], [-3, 60, 80, 95], [20, 84, 10, 74]]
    fc = [cc._rot_quad(120.0, 80.0, 60.0, 20.0, 30.0)]
    return [(a, cc.HORI, cc.FREE), (b, hb, fb), (c, hc, fc)]


@pytest.mark.parametrize("case", [(0, 0.0), (0, 0.5), (3, 0.5)], ids=["own widths", "own widths contrast", "forced rot90 x2 contrast"])
def test_pages_against_the_reference(rd, case):
    """bbocr_op_crops_pages: the page-table variants of the kernels (each page its own bounds and row pitch), against the oracle page by page"""
    from bb_ocr_amd import _lib

    el, reader = rd
    mode, contrast = case
    pages = _pages()
    dev = [torch.from_numpy(p.copy()).cuda() for p, _, _ in pages]
    big = torch.full((180 + 9, 300 + 23), GUARD, dtype=torch.uint8, device="cuda")
    big[4:184, 11:311] = dev[1]
    dev[1] = big[4:184, 11:311]
    assert dev[1].stride(0) > dev[1].shape[1]
    arr = (_lib.bbocr_page * 3)()
    for k, g in enumerate(dev):
        arr[k].dev_gray, arr[k].H, arr[k].W, arr[k].gray_pitch = g.data_ptr(), g.shape[0], g.shape[1], g.stride(0)
    harr, farr = _arrays([b for _, h, _ in pages for b in h], [q for _, _, f in pages for q in f])
    hoff = (C.c_int * 4)(*np.concatenate([[0], np.cumsum([len(h) for _, h, _ in pages])]).tolist())
    foff = (C.c_int * 4)(*np.concatenate([[0], np.cumsum([len(f) for _, _, f in pages])]).tolist())
    per_page = [cc.stage_a(p, h, f) for p, h, f in pages]
    assert all(any(it is None for it in items) for items in per_page[:2])
    rot = mode - 1 if mode else 0
    widths = sorted({it[1] for items in per_page for it in items if it}) if mode == 0 else [FORCED_W]
    for mw in widths:
        wants = []
        for pi, items in enumerate(per_page):
            for k, it in enumerate(items):
                if it is None or (mode == 0 and it[1] != mw):
                    continue
                w, h = cc.source_size(k, pages[pi][1], pages[pi][2], pages[pi][0].shape)
                wants.append((f"page {pi} box {k} ({cc.regime_name(cc.classify(w, h))})", cc.collate(it[0], mw, contrast, rot)))
        out = _sentinel(len(wants), mw)
        torch.cuda.synchronize()
        n_out = C.c_int()
        reader._check(reader._lib.bbocr_op_crops_pages(reader._h, arr, 3, harr, hoff, farr, foff, mw, float(contrast), C.c_void_p(out.data_ptr()),
                                                       C.byref(n_out), mode))
        assert n_out.value == len(wants), f"{el}, pages, width {mw}: {n_out.value} crops, the oracle keeps {len(wants)}"
        _compare(out.cpu(), wants, el, f"{el}, pages, mode {mode}, contrast {contrast}, width {mw}")
    assert (big[:4] == GUARD).all() and (big[184:] == GUARD).all() and (big[:, :11] == GUARD).all() and (big[:, 311:] == GUARD).all()
