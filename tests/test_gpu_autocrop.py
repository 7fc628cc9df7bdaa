"""-m gpu: the text-region auto-crop on the device (csrc/autocrop.hip, bbocr_auto_crop / bbocr_op_autocrop_stage) against the CPU
restatement of tests/autocrop_ref.py, stage by stage and box by box, and through the extractor's OCR input path; its rect morphology
and component kernels on the designed masks of tests/autocrop_cases.py (bbocr_op_autocrop_mask_stage)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

import autocrop_cases as cases
import autocrop_ref as ref

pytestmark = pytest.mark.gpu

PHOTO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photos", "IMG_9684.JPG")
STAGES = ("clahe", "composite", "merged", "external")


def _stage(reader, page_dev, stage):
    from bb_ocr_amd.preprocess import _page_layout

    H, W, pitch, ch = _page_layout(reader, page_dev)
    out = torch.full((H, W), 7, dtype=torch.uint8, device=page_dev.device)
    reader._check(reader._lib.bbocr_op_autocrop_stage(reader._h, stage, C.c_void_p(page_dev.data_ptr()), H, W, pitch, ch, C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def _want(st, name):
    v = st[name]
    return v if v.dtype == np.uint8 and name == "clahe" else np.where(v, 255, 0).astype(np.uint8)


def _check_page(reader, host, dev=None, margin=128):
    from bb_ocr_amd.preprocess import auto_crop_box_device

    dev = reader._to_dev(host) if dev is None else dev
    st = ref.stages(host)
    for k, name in enumerate(STAGES):
        got = _stage(reader, dev, k)
        want = _want(st, name)
        bad = int((got != want).sum())
        assert bad == 0, f"stage {name}: {bad} of {want.size} pixels differ"
    box, comps = auto_crop_box_device(reader, dev, margin, with_components=True)
    wbox, wcomps = ref.crop_box(st["boxes"], host.shape[0], host.shape[1], margin)
    assert box == wbox and comps == wcomps
    return box


def _text_page(seed, H=600, W=800, frame=False):
    """white page, dark text-like bars; frame=True draws a thick rectangle larger than 10 % of the page around them"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 235, np.uint8)
    for _ in range(12):
        y, x = int(rng.integers(H // 4, 3 * H // 4)), int(rng.integers(W // 4, W // 2))
        img[y:y + 8, x:x + int(rng.integers(30, 150))] = 20
    if frame:
        img[40:H - 40, 40:48] = img[40:H - 40, W - 48:W - 40] = 10
        img[40:48, 40:W - 40] = img[H - 48:H - 40, 40:W - 40] = 10
    return img


@pytest.mark.parametrize("shape", [(64, 64), (97, 131), (240, 320), (333, 250)])
def test_stages_random_pages(reader, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    _check_page(reader, rng.integers(0, 256, shape, dtype=np.uint8))
    bgr = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    _check_page(reader, bgr)


@pytest.mark.parametrize("seed", [0, 3])
def test_stages_synth_pages(reader, seed):
    from bb_ocr_amd import synth

    img, _ = synth.page(seed, width=640, height=480, lines=8)
    bgr = np.ascontiguousarray(img[:, :, ::-1])
    _check_page(reader, bgr)
    _check_page(reader, ref.to_gray(bgr), margin=0)


def test_framed_text_and_strided_view(reader):
    # a frame larger than 10 % of the page encloses the text: only the frame is external, and it is dropped by area -> None
    page = _text_page(5, frame=True)
    assert _check_page(reader, page) is None
    st = ref.stages(page)
    from scipy import ndimage

    assert len(st["boxes"]) == 1 and ndimage.label(st["merged"], structure=np.ones((3, 3), bool))[1] > 1
    # the same text without the frame is found; a view of a larger plane is read through its pitch, in place
    plain = _text_page(5)
    big = torch.zeros((700, 1000), dtype=torch.uint8, device=reader.device)
    big[37:637, 101:901] = torch.from_numpy(plain).to(reader.device)
    view = big[37:637, 101:901]
    assert not view.is_contiguous()
    assert _check_page(reader, plain, dev=view) is not None
    bgr = torch.zeros((700, 1000, 3), dtype=torch.uint8, device=reader.device)
    bgr[37:637, 101:901] = torch.from_numpy(np.repeat(plain[:, :, None], 3, axis=2)).to(reader.device)
    _check_page(reader, np.repeat(plain[:, :, None], 3, axis=2), dev=bgr[37:637, 101:901])


def test_empty_and_constant_pages(reader):
    from bb_ocr_amd.preprocess import auto_crop_box_device

    for v in (0, 128, 255):
        page = np.full((120, 160), v, np.uint8)
        assert auto_crop_box_device(reader, reader._to_dev(page)) == ref.auto_crop(page)[0]
        _check_page(reader, page)


@pytest.fixture(scope="module")
def photo_f2(reader):
    from bb_ocr_amd.preprocess import _imread_bgr, central_edge_crop_box, preprocess_bgr_device

    f2 = preprocess_bgr_device(reader, reader._to_dev(_imread_bgr(PHOTO)))
    b = central_edge_crop_box(f2.shape[0], f2.shape[1], 15)
    view = f2[b[1]:b[3], b[0]:b[2]]
    return f2, view, view.contiguous().cpu().numpy()


def test_full_photo_page(reader, photo_f2):
    # the f2 output of a phone photograph of a book page, edge-cropped 15 % as a view of the device plane
    _, view, host = photo_f2
    assert _check_page(reader, host, dev=view) is not None


def test_concurrent_calls(reader, photo_f2):
    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import auto_crop_box_device

    _, view, _ = photo_f2
    pages = [reader._to_dev(_text_page(s)) for s in range(3)] + [view]
    serial = [auto_crop_box_device(reader, p, 128, with_components=True) for p in pages]
    img, _ = synth.page(1, width=640, height=480, lines=8)
    rgb = torch.from_numpy(img[None]).to(reader.device)
    want_text = [t for _, t, _ in reader.readtext_device(rgb)[0]]
    got, errs = {}, []

    def crop(k):
        try:
            for _ in range(3):
                for i, p in enumerate(pages):
                    assert auto_crop_box_device(reader, p, 128, with_components=True) == serial[i]
            got[k] = True
        except Exception as e:        # reported below
            errs.append(e)

    def ocr():
        try:
            for _ in range(3):
                assert [t for _, t, _ in reader.readtext_device(rgb)[0]] == want_text
            got["ocr"] = True
        except Exception as e:
            errs.append(e)

    ts = [threading.Thread(target=crop, args=(0,)), threading.Thread(target=crop, args=(1,)), threading.Thread(target=ocr)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert len(got) == 3


def test_error_paths(reader):
    from bb_ocr_amd.preprocess import auto_crop_box_device

    page = reader._to_dev(_text_page(1, 64, 64))
    box, found, n = (C.c_int * 4)(), C.c_int(), C.c_int()
    comps = (C.c_int * 16)()
    f = reader._lib.bbocr_auto_crop
    ptr = C.c_void_p(page.data_ptr())
    cases = [
        (ptr, 64, 64, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (None, 64, 64, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 0, 64, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 64, 0, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 64, 64, 63, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 64, 64, 64, 2, 128, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 22, 22, 64, 3, 128, box, C.byref(found), comps, 4, C.byref(n)),      # pitch < 3 W
        (ptr, 64, 64, 64, 1, -1, box, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 64, 64, 64, 1, 128, None, C.byref(found), comps, 4, C.byref(n)),
        (ptr, 64, 64, 64, 1, 128, box, None, comps, 4, C.byref(n)),
        (ptr, 64, 64, 64, 1, 128, box, C.byref(found), None, 4, C.byref(n)),
        (ptr, 64, 64, 64, 1, 128, box, C.byref(found), comps, 4, None),
        (ptr, 4, 4, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)),           # smaller than the CLAHE grid
    ]
    for k, args in enumerate(cases):
        rc = f(reader._h, *args)
        assert rc == (0 if k == 0 else -1), (k, rc)                          # BBOCR_OK / BBOCR_ERR_ARG
    assert f(None, ptr, 64, 64, 64, 1, 128, box, C.byref(found), comps, 4, C.byref(n)) == -1
    out = torch.empty((64, 64), dtype=torch.uint8, device=reader.device)
    st = reader._lib.bbocr_op_autocrop_stage
    assert st(reader._h, 4, ptr, 64, 64, 64, 1, C.c_void_p(out.data_ptr())) == -1
    assert st(reader._h, 0, ptr, 64, 64, 64, 1, None) == -1
    with pytest.raises(ValueError):
        auto_crop_box_device(reader, page, -1)
    with pytest.raises(ValueError):
        auto_crop_box_device(reader, page.float())
    with pytest.raises(ValueError):
        auto_crop_box_device(reader, page.t())                               # columns not packed
    # the context still works afterwards
    assert auto_crop_box_device(reader, page) == ref.auto_crop(_text_page(1, 64, 64))[0]


def test_extract_texts_with_crops(reader, photo_f2):
    from PIL import Image

    from bb_ocr_amd import extractor_batch
    from bb_ocr_amd.reader import decode_file

    got = extractor_batch.extract_texts(reader, [PHOTO, PHOTO], ocr_image_indices=[0, 1], use_preprocessing=True, edge_crop_percent=15,
                                        crop_for_ocr=True)
    # the reference on the host: the restatement's crop of the same f2 page, the PNG it writes, the thumbnail rule, readtext
    _, _, host = photo_f2
    b = ref.auto_crop(host)[0]
    crop = host[b[1]:b[3], b[0]:b[2]]
    for i in (0, 1):
        max_dim = 1600 if i == 0 else 2400
        img = Image.fromarray(crop).convert("RGB")
        if max(img.size) > max_dim:
            import io

            img.thumbnail((max_dim, max_dim))
            buf = io.BytesIO()
            img.save(buf, format="JPEG", quality=90 if i == 0 else 95)
            rgb, gray = decode_file(buf.getvalue())
        else:
            rgb, gray = np.asarray(img), crop
        want = " ".join(t for _, t, _ in reader.readtext_arrays(rgb[None], gray[None])[0])
        assert got[i] == want, (i, got[i], want)
    # defaults: the keywords off leave the pages as they were
    assert extractor_batch.extract_texts(reader, [PHOTO]) == extractor_batch.extract_texts(reader, [PHOTO], use_preprocessing=False,
                                                                                            edge_crop_percent=0.0, crop_for_ocr=False)


# ---- designed masks (tests/autocrop_cases.py) through bbocr_op_autocrop_mask_stage: the rect morphology and the component kernels on
# structure the pages above never give them.  Every comparison is exact.

MODES = {"merged": 0, "external": 1, "components": 2}
GUARD = 96


def _mask_stage(reader, mask, mode, max_boxes=None):
    """-> (u8 [H,W] output, sorted (x, y, w, h) boxes, reported count).  The mask is a view inside a larger plane of nonzero bytes, its
    set pixels any nonzero value; the output lies between guard bytes, which must come back as they were."""
    H, W = mask.shape
    host = np.full((H + 3, W + 7), 1, np.uint8)
    host[2:H + 2, 3:W + 3] = np.where(mask, 1 + (np.arange(mask.size).reshape(H, W) % 255), 0)
    view = torch.from_numpy(host).to(reader.device)[2:H + 2, 3:W + 3]
    assert view.stride() == (W + 7, 1)
    flat = torch.full((GUARD + H * W + GUARD,), 7, dtype=torch.uint8, device=reader.device)
    cap = ((H + 1) // 2) * ((W + 1) // 2) if max_boxes is None else max_boxes
    boxes, n = (C.c_int * (4 * cap + 4))(*([-5] * (4 * cap + 4))), C.c_int(-1)
    reader._check(reader._lib.bbocr_op_autocrop_mask_stage(reader._h, MODES[mode], C.c_void_p(view.data_ptr()), H, W, W + 7,
                                                           C.c_void_p(flat.data_ptr() + GUARD), boxes, cap, C.byref(n)))
    got = flat.cpu().numpy()
    assert (got[:GUARD] == 7).all() and (got[GUARD + H * W:] == 7).all(), "guard bytes around the destination were written"
    k = min(n.value, cap)
    assert list(boxes[4 * k:]) == [-5] * (4 * (cap - k) + 4), "box slots beyond the copied ones were written"
    return got[GUARD:GUARD + H * W].reshape(H, W), sorted(tuple(boxes[4 * i:4 * i + 4]) for i in range(k)), n.value


def _u8(m):
    return np.where(m, 255, 0).astype(np.uint8)


def _check_mask_case(reader, name, e):
    got, boxes, n = _mask_stage(reader, e.mask, "merged")
    bad = int((got != _u8(e.merged)).sum())
    assert bad == 0 and n == 0 and boxes == [], f"{name} merged: {bad} of {got.size} pixels differ"
    for mode, (wmask, wboxes) in (("external", e.external), ("components", e.components)):
        got, boxes, n = _mask_stage(reader, e.mask, mode)
        bad = int((got != _u8(wmask)).sum())
        assert bad == 0, f"{name} {mode}: {bad} of {got.size} pixels differ"
        assert n == len(wboxes) and boxes == sorted(wboxes), f"{name} {mode}: boxes {boxes[:8]} want {sorted(wboxes)[:8]}"


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_mask_stage_designed_cases(reader, family):
    exp = {n: e for n, e in cases.expected().items() if n in cases.FAMILIES[family]()}
    assert exp
    for name, e in exp.items():
        _check_mask_case(reader, name, e)


def test_mask_stage_consecutive_calls_agree(reader):
    exp = cases.expected()
    names = [n for n in exp if n.startswith(("random/", "chain/", "lattice/", "checkerboard/", "diamond/", "area/"))]
    assert len(names) >= 12
    for mode in MODES:
        for name in names:
            a, b = _mask_stage(reader, exp[name].mask, mode), _mask_stage(reader, exp[name].mask, mode)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (mode, name)
    # a large mask, then a small one in the same work buffer, then the page path: nothing of the earlier call shows
    big, small = exp["random/8x8230/p0.01"], exp["diamond/closed"]
    _check_mask_case(reader, "big", big)
    _check_mask_case(reader, "small", small)
    _check_page(reader, _text_page(1, 64, 64))
    _check_mask_case(reader, "small", small)


def test_mask_stage_box_limit_and_errors(reader):
    e = cases.expected()["lattice/11x33"]
    want = sorted(e.components[1])
    full = _mask_stage(reader, e.mask, "components")
    assert full[1] == want and full[2] == len(want) == 102
    # fewer slots than boxes: the count is still the whole count, and only that many boxes are copied (each a real one)
    _, some, n = _mask_stage(reader, e.mask, "components", max_boxes=5)
    assert n == 102 and len(some) == 5 and set(some) <= set(want)
    _, none, n = _mask_stage(reader, e.mask, "components", max_boxes=0)
    assert n == 102 and none == []
    f = reader._lib.bbocr_op_autocrop_mask_stage
    src = torch.ones((16, 40), dtype=torch.uint8, device=reader.device)
    dst = torch.full((16, 40), 7, dtype=torch.uint8, device=reader.device)
    sp, dp = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    boxes, cnt = (C.c_int * 16)(), C.c_int()
    assert f(reader._h, 2, sp, 16, 40, 40, dp, None, 0, C.byref(cnt)) == 0 and cnt.value == 1          # no box buffer needed for 0 slots
    bad = [
        (2, None, 16, 40, 40, dp, boxes, 4, C.byref(cnt)),
        (2, sp, 16, 40, 40, None, boxes, 4, C.byref(cnt)),
        (2, sp, 16, 40, 40, dp, None, 4, C.byref(cnt)),
        (2, sp, 16, 40, 40, dp, boxes, 4, None),
        (2, sp, 16, 40, 39, dp, boxes, 4, C.byref(cnt)),          # pitch < W
        (2, sp, 0, 40, 40, dp, boxes, 4, C.byref(cnt)),
        (2, sp, 16, 0, 40, dp, boxes, 4, C.byref(cnt)),
        (3, sp, 16, 40, 40, dp, boxes, 4, C.byref(cnt)),          # unknown modes
        (-1, sp, 16, 40, 40, dp, boxes, 4, C.byref(cnt)),
        (2, sp, 16, 40, 40, dp, boxes, -1, C.byref(cnt)),
    ]
    dst.fill_(7)
    for k, args in enumerate(bad):
        assert f(reader._h, *args) == -1, k                       # BBOCR_ERR_ARG
    assert f(None, 2, sp, 16, 40, 40, dp, boxes, 4, C.byref(cnt)) == -1
    assert bool((dst == 7).all())                                 # refused before anything was queued
    # the context still works afterwards
    assert _mask_stage(reader, e.mask, "components")[1] == want


@pytest.mark.parametrize("shape", cases.BAR_PAGES)
def test_stages_sparse_bar_pages(reader, shape):
    # widths that are no multiple of 32, a merged mask with structure: gray, BGR, and both as views of larger planes
    from scipy import ndimage

    H, W = shape
    page = cases.bar_page(shape)
    st = ref.stages(page)
    assert W % 32 and len(st["boxes"]) >= 3 and 0.02 < st["merged"].mean() < 0.6
    assert ndimage.label(st["merged"], structure=np.ones((3, 3), bool))[1] == len(st["boxes"])
    assert _check_page(reader, page, margin=8) is not None
    bgr = np.repeat(page[:, :, None], 3, axis=2)
    bgr[:, :, 0] = np.minimum(bgr[:, :, 0], 200)                 # not a gray image in three channels
    _check_page(reader, bgr, margin=8)
    big = torch.full((H + 9, W + 21), 255, dtype=torch.uint8, device=reader.device)
    big[4:H + 4, 11:W + 11] = torch.from_numpy(page).to(reader.device)
    _check_page(reader, page, dev=big[4:H + 4, 11:W + 11], margin=8)
    big3 = torch.full((H + 9, W + 21, 3), 255, dtype=torch.uint8, device=reader.device)
    big3[4:H + 4, 11:W + 11] = torch.from_numpy(bgr).to(reader.device)
    _check_page(reader, bgr, dev=big3[4:H + 4, 11:W + 11], margin=8)
