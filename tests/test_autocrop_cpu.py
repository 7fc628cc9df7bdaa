"""CPU: the restatement of the extractor's text-region auto-crop (tests/autocrop_ref.py) on synthetic pages -- the semantics the device
kernels must reproduce -- and the host arithmetic of the crop boxes (bb_ocr_amd.preprocess)."""
import numpy as np
import pytest
from scipy import ndimage

import autocrop_ref as ref


def test_gaussian_taps():
    from oracle import preprocess as opp

    k = ref.gaussian_taps_fixed(31)
    assert sum(k) == 256 and k == k[::-1] and max(k) == k[15]
    for sigma in (0.8, 1.0, 3.0, 5.0):
        assert ref.gaussian_taps_fixed(3, sigma) == opp.gaussian_kernel3_fixed(sigma)


def test_otsu_special_cases():
    for v in (0, 9, 255):
        assert ref.otsu_threshold(np.full((7, 9), v, np.uint8)) == 0          # single-valued: every bin skipped
    two = np.array([[10] * 5 + [200] * 5], np.uint8)
    assert ref.otsu_threshold(two) == 10                                     # first maximum kept
    assert ref.otsu_threshold(np.arange(256, dtype=np.uint8).reshape(16, 16)) == 127


def _text_page(seed, H=400, W=500, frame=False):
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 235, np.uint8)
    for _ in range(10):
        y, x = int(rng.integers(H // 4, 3 * H // 4)), int(rng.integers(W // 4, W // 2))
        img[y:y + 6, x:x + int(rng.integers(20, 100))] = 20
    if frame:
        img[30:H - 30, 30:36] = img[30:H - 30, W - 36:W - 30] = 10
        img[30:36, 30:W - 30] = img[H - 36:H - 30, 30:W - 30] = 10
    return img


def test_frame_hides_the_text_inside():
    framed = ref.stages(_text_page(2, frame=True))
    # RETR_EXTERNAL: only the frame is a contour; the text blocks inside its hole are not, even though the frame is dropped by area
    assert len(framed["boxes"]) == 1
    assert ndimage.label(framed["merged"], structure=np.ones((3, 3), bool))[1] > 1
    assert ref.crop_box(framed["boxes"], 400, 500)[0] is None
    box, kept = ref.auto_crop(_text_page(2))
    assert box is not None and kept


def test_empty_page_gives_none():
    assert ref.auto_crop(np.full((100, 120), 255, np.uint8)) == (None, [])
    assert ref.crop_box([], 100, 100) == (None, [])


def test_small_union_inflated_and_margin_clamped():
    # union 50 x 50 of a 1000 x 1000 page < 12 %: inflated by int(0.03 * 1000) = 30, then the margin
    assert ref.crop_box([(100, 100, 50, 50)], 1000, 1000, margin=0)[0] == (70, 70, 180, 180)
    assert ref.crop_box([(100, 100, 50, 50)], 1000, 1000, margin=128)[0] == (0, 0, 308, 308)
    # area filter: specks below 0.01 % and blobs above 10 % are dropped
    assert ref.crop_box([(0, 0, 9, 9), (0, 0, 400, 400)], 1000, 1000)[0] is None
    # a large union is not inflated; the margin is clamped at every edge
    assert ref.crop_box([(0, 0, 300, 300), (600, 600, 300, 300)], 1000, 1000, margin=128)[0] == (0, 0, 1000, 1000)


def test_folded_morphology_equals_literal():
    # the device folds CLOSE / OPEN / dilate of both variants into five rect passes; with the border never taking part that is exact
    rng = np.random.default_rng(0)
    for shape, p in (((61, 87), 0.2), ((120, 45), 0.05), ((7, 300), 0.5)):
        m = rng.random(shape) < p
        a = ref.erode(ref.dilate(m, 17, 5), 19, 7)
        b = ref.erode(ref.dilate(m, 29, 9), 31, 11)
        assert np.array_equal(ref.dilate(a | b, 13, 5), ref.merged_mask(m))


def test_external_components_rules():
    fg = np.zeros((20, 20), bool)
    fg[2:18, 2] = fg[2:18, 17] = fg[2, 2:18] = fg[17, 2:18] = True          # ring
    fg[8:11, 8:11] = True                                                   # blob in its hole
    fg[0, 19] = True                                                        # touches the edge
    mask, boxes = ref.external_components(fg)
    assert sorted(boxes) == [(2, 2, 16, 16), (19, 0, 1, 1)]
    assert not mask[9, 9] and mask[2, 5]
    # 8-connected foreground: a diagonal step joins two pieces
    fg2 = np.zeros((10, 10), bool)
    fg2[3, 3] = fg2[4, 4] = True
    assert ref.external_components(fg2)[1] == [(3, 3, 2, 2)]


def test_central_edge_crop_box():
    from bb_ocr_amd.preprocess import central_edge_crop_box

    assert central_edge_crop_box(8568, 6426, 15) == (964, 1285, 5462, 7283)
    assert central_edge_crop_box(100, 100, 0) is None
    assert central_edge_crop_box(100, 100, 41) is None                      # 18 px left < max(16, 20 % of 100)
    assert central_edge_crop_box(100, 100, 40) == (40, 40, 60, 60)
    assert central_edge_crop_box(30, 30, 10) == (3, 3, 27, 27)
    assert central_edge_crop_box(18, 300, 10) is None                       # 14 rows left < 16


def test_extract_texts_keywords_default_off():
    import inspect

    from bb_ocr_amd import extractor_batch

    sig = inspect.signature(extractor_batch.extract_texts)
    assert sig.parameters["use_preprocessing"].default is False
    assert sig.parameters["edge_crop_percent"].default == 0.0
    assert sig.parameters["crop_for_ocr"].default is False
    assert sig.parameters["crop_margin"].default == 128
