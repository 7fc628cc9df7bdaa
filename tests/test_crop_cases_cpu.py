"""CPU: the shared crop cases (tests/crop_cases.py) can fail.  They reach every regime of the crop stage (coverage by the classifier), both
branches and both inner edges of adjust_contrast_grey; the reference they are compared with agrees with the installed Pillow where it
restates Pillow; and each plausible defect of the stage, planted into the reference as a mutant, changes at least one output element on
this very case set -- so the bit-exact GPU comparison over these cases would see the same defect in a kernel."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import crop_cases as cc  # noqa: E402
from oracle import imgproc, recog  # noqa: E402

# (stage-A regime, tall, padded) cells that must be hit, with the box that was designed for each
CELLS = {
    "area2 200x128": ("area2", False, True),
    "bilinear neighbour 201x128": ("down", False, True),
    "same 100x64": ("same", False, True),
    "same 192x64 unpadded": ("same", False, False),
    "down 200x190": ("down", False, True),
    "down 370x100": ("down", False, True),
    "down whole page": ("down", False, True),
    "same tall 64x128": ("same", True, True),
    "area2 tall 128x256": ("area2", True, True),
    "up tall 20x300": ("up", True, True),
    "up tall 3x40": ("up", True, True),
    "width 1 (1x64)": ("up", True, True),
    "height 1 (40x1)": ("up", False, False),
    "up negative x_min": ("up", False, False),
    "up over the top edge": ("up", False, True),
    "free half-pixel 256x128 (area2)": ("area2", False, False),
    "free steep tall": ("up", True, True),
}


def test_every_named_regime_is_reached():
    items = cc.stage_a_cases()
    cells = {}
    for k, name in enumerate(cc.NAMES):
        w, h = cc.source_size(k)
        if name in cc.SKIPPED:
            assert (w <= 0 or h <= 0) and items[k] is None, name
            continue
        assert w > 0 and h > 0 and items[k] is not None, name
        cells[name] = cc.classify(w, h)
        rw, rh, imgW, fw = cc.plan_sizes(w, h)
        assert items[k][0].shape == (rh, rw) and items[k][1] == imgW, name            # the classifier's sizes are the oracle's
    for name, cell in CELLS.items():
        assert cells[name] == cell, (name, cells[name])
    assert cc.SKIPPED <= set(cc.NAMES)
    size = lambda name: cc.source_size(cc.NAMES.index(name))
    assert size("area2 200x128") == (200, 128) and size("bilinear neighbour 201x128") == (201, 128) and size("down whole page") == (cc.W, cc.H)
    assert cc.plan_sizes(*size("width 1 (1x64)"))[1] == 4096 and cc.plan_sizes(*size("height 1 (40x1)"))[0] == 2560
    # boxes that leave the page on each side are clamped, not dropped
    for name, side in (("up negative x_min", 0), ("up over the top edge", 2), ("past the right edge", 1), ("past the bottom edge", 3)):
        b = cc.HORI[cc.HORI_NAMES.index(name)]
        assert (b[side] < 0) if side in (0, 2) else (b[side] > (cc.W if side == 1 else cc.H)), name
    # the free boxes: one inside, two leaving the page over opposite corners
    quad = lambda name: np.array(cc.FREE[cc.FREE_NAMES.index(name)])
    q = quad("free inside")
    assert q.min() > 0 and q[:, 0].max() < cc.W - 1 and q[:, 1].max() < cc.H - 1
    assert quad("free over the top-left corner").min(axis=0).max() < 0
    q = quad("free over the bottom-right corner")
    assert q[:, 0].max() > cc.W and q[:, 1].max() > cc.H
    assert len({imgW for _, imgW in filter(None, items)}) >= 8                       # own-width buckets of the bucket layout


def test_contrast_branches_and_inner_edges():
    lut, untouched, narrow, dark = [], [], [], []
    for name, item in zip(cc.NAMES, cc.stage_a_cases()):
        if item is None:
            continue
        contrast, high, low = recog.contrast_grey(item[0])
        assert abs(contrast - 0.5) > 1e-6, name                 # no crop sits on the threshold, where a last-bit difference would decide
        (lut if contrast < 0.5 else untouched).append(name)
        if contrast < 0.5 and high - low < 10:
            narrow.append(name)                                  # ratio = 200 / max(10, high - low) takes its floor
        if high + low < 10:
            dark.append(name)                                    # contrast = (high - low) / max(10, high + low) takes its floor
    assert len(lut) >= 4 and len(untouched) >= 4, (lut, untouched)
    assert any(n.startswith("narrow band") for n in narrow) and any(n.startswith("black band") for n in dark), (narrow, dark)
    assert set(dark) & set(lut) and set(dark) & set(untouched)
    # the low band: contrast about 0.13, below the target; its `same` crop puts the 10th percentile between two grey levels
    k = cc.NAMES.index("low band same 100x64")
    contrast, high, low = recog.contrast_grey(cc.stage_a_cases()[k][0])
    assert 0.05 < contrast < 0.2 and low == pytest.approx(107.6) and np.percentile(cc.stage_a_cases()[k][0], 10, method="nearest") == 108
    # tall crops are among those that get a LUT (the LUT is then applied inside the horizontal Pillow pass)
    assert any(cc.classify(*cc.source_size(cc.NAMES.index(n)))[1] for n in lut)


def test_reference_pillow_resize_is_pillows():
    """pil_resize_bicubic_u8 == Image.resize(BICUBIC) on the stage-A image of every case AlignCollate really resamples (tall, or rotated)"""
    from PIL import Image

    n = 0
    for k, item in enumerate(cc.stage_a_cases()):
        if item is None:
            continue
        crop = item[0]
        w, h = cc.source_size(k)
        variants = [crop] if cc.classify(w, h)[1] else []
        if k % 5 == 0:
            variants.append(np.ascontiguousarray(np.rot90(crop)))                 # a rotation_info variant: hundreds of rows down to 64
        for img in variants:
            fw = min(item[1], math.ceil(64 * (img.shape[1] / img.shape[0])))
            want = np.asarray(Image.fromarray(img).resize((fw, 64), Image.BICUBIC))
            cc.assert_same(imgproc.pil_resize_bicubic_u8(img, (fw, 64)), want, f"Pillow cross-check, {cc.describe(k)}, {img.shape} -> 64 x {fw}")
            n += 1
    assert n >= 12


def test_exact_mode_codes_recover_every_grey_level():
    img = np.arange(64 * 64, dtype=np.int64).reshape(64, 64) % 256
    t = recog.align_collate_one(img.astype(np.uint8), 64, 128)[0]
    codes = cc.codes_from_tensor(t)
    assert set(np.unique(img)) == set(range(256))
    assert np.array_equal(codes[:, :64], img) and np.array_equal(codes[:, 64:], np.repeat(img[:, 63:64], 64, axis=1))
    assert np.array_equal(cc.to_el(t, "exact"), (codes + 1).astype(np.int16))
    for el in ("bf16", "fp16", "exact"):
        assert cc.SENTINEL not in set(np.unique(cc.to_el(t, el).view(np.uint16)).tolist()), el


# ------------------------------------------------------------------------------------------------ sensitivity: mutants of the reference
FORCED_W = 256        # the forced width of the rotation_info checks (tests/test_gpu_crops.py)


def _outputs():
    """every output the GPU tests compare, from the un-cached reference builders: own-width crops at contrast 0 and 0.5, and the rot90
    variants at the forced width"""
    items = cc.stage_a(cc.make_page(), cc.HORI, cc.FREE)
    out = {}
    for k, item in enumerate(items):
        if item is None:
            out[k] = None
            continue
        for contrast in (0.0, 0.5):
            out[k, contrast] = cc.collate(item[0], item[1], contrast)
        for rot in (1, 2, 3):
            out[k, "rot", rot] = cc.collate(item[0], FORCED_W, 0.0, rot)
    return out


@pytest.fixture(scope="module")
def baseline():
    return _outputs()


def _changed(baseline, got):
    """keys of the outputs present on both sides whose elements differ (a mutant may also change WHICH boxes are taken: not counted)"""
    return [key for key in baseline if baseline[key] is not None and got.get(key) is not None and not np.array_equal(baseline[key], got[key])]


def _warp_variant(border_zero=True, rounder=np.rint):
    """recog.warp_perspective_u8 restated with its border rule and its coordinate rounding open to change"""
    def warp(src, M, dsize_wh):
        dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
        Mi = recog.invert3x3(M)
        sh, sw = src.shape
        xs, ys = np.arange(dw, dtype=np.float64)[None, :], np.arange(dh, dtype=np.float64)[:, None]
        X0 = Mi[0, 0] * xs + (Mi[0, 1] * ys + Mi[0, 2])
        Y0 = Mi[1, 0] * xs + (Mi[1, 1] * ys + Mi[1, 2])
        W0 = Mi[2, 0] * xs + (Mi[2, 1] * ys + Mi[2, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            Wi = np.where(W0 != 0, 32.0 / W0, 0.0)
        X = rounder(np.clip(X0 * Wi, -2147483648.0, 2147483647.0)).astype(np.int64)
        Y = rounder(np.clip(Y0 * Wi, -2147483648.0, 2147483647.0)).astype(np.int64)
        sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
        ax, ay = X & 31, Y & 31
        s = src.astype(np.int64)

        def tap(yy, xx):
            v = s[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
            return np.where((yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw), v, 0) if border_zero else v

        acc = (tap(sy, sx) * ((32 - ax) * (32 - ay) * 32) + tap(sy, sx + 1) * (ax * (32 - ay) * 32) + tap(sy + 1, sx) * ((32 - ax) * ay * 32)
               + tap(sy + 1, sx + 1) * (ax * ay * 32))
        return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    return warp


def _coeffs_from_double(ssize, dsize):
    """imgproc.linear_coeffs with fx kept in double"""
    scale = 1.0 / (float(dsize) / float(ssize))
    fx = (np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5
    sx = np.floor(fx).astype(np.int32)
    fx = fx - sx
    lo, hi = sx < 0, sx >= ssize - 1
    fx[lo | hi] = 0.0
    sx[lo] = 0
    sx[hi] = ssize - 1
    return sx, np.minimum(sx + 1, ssize - 1), np.rint((1.0 - fx) * 2048).astype(np.int32), np.rint(fx * 2048).astype(np.int32)


def _resize_without_last_clamp(orig_resize):
    """cv2.resize whose taps are not clamped at the last column / row.  Removing only the clamp of the second tap's index changes no value:
    wherever sx + 1 reaches ssize, sx was clamped to ssize - 1 and fx set to 0, so that tap's weight is 0.  The defect that can show is the
    whole last-column clamp missing -- the second tap reads one pixel past the crop with a weight above 0.  Here that pixel is the mirror
    image (255 - v) of the last one."""
    def resize(src, dsize_wh):
        dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
        sh, sw = src.shape
        if (sw, sh) == (dw, dh) or (sw, sh) == (2 * dw, 2 * dh):
            return orig_resize(src, dsize_wh)
        ext = np.pad(src, ((0, 1), (0, 1)), mode="edge")
        ext[-1, :], ext[:, -1] = 255 - ext[-1, :], 255 - ext[:, -1]
        x0, x1, a0, a1 = _last_open(sw, dw)
        y0, y1, b0, b1 = _last_open(sh, dh)
        a = ext.astype(np.int32)
        rows = a[:, x0] * a0[None, :] + a[:, x1] * a1[None, :]
        v = (((b0[:, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
        return np.clip(v, 0, 255).astype(np.uint8)
    return resize


def _last_open(ssize, dsize):
    """linear_coeffs of the ssize -> dsize resize without the clamp at the last source pixel: the second tap may be index ssize"""
    scale = 1.0 / (float(dsize) / float(ssize))
    fx = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int32)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    fx[lo] = 0.0
    sx[lo] = 0
    assert sx.max() <= ssize - 1
    return sx, sx + 1, imgproc._cv_round_f32((np.float32(1.0) - fx) * np.float32(2048)), imgproc._cv_round_f32(fx * np.float32(2048))


def _unclamped_image_list(orig):
    """get_image_list that does not clamp a horizontal box to the page: what lies outside reads as 0"""
    P = 64

    def get_image_list(horizontal_list, free_list, img, **kw):
        if not horizontal_list:
            return orig(horizontal_list, free_list, img, **kw)
        assert not free_list
        big = np.pad(img, P)
        moved = [[max(b[0], -P) + P, min(b[1], img.shape[1] + P) + P, max(b[2], -P) + P, min(b[3], img.shape[0] + P) + P] for b in horizontal_list]
        return orig(moved, [], big, **kw)
    return get_image_list


def _collate_variant(orig, pad_zero=False, floor_fw=False):
    def align_collate_one(crop, imgH, imgW, adjust_contrast=0.0):
        if floor_fw:
            recog.math = SimpleNamespace(ceil=lambda v: max(1, math.floor(v)))
        try:
            out = orig(crop, imgH, imgW, adjust_contrast=adjust_contrast)
        finally:
            recog.math = math
        if pad_zero:
            fw = min(imgW, math.ceil(imgH * (crop.shape[1] / float(crop.shape[0]))))
            out[0, :, fw:] = 0.0
        return out
    return align_collate_one


def _contrast_variant(orig, force=None, method="linear"):
    def contrast_grey(img):
        high, low = np.float64(np.percentile(img, 90, method=method)), np.float64(np.percentile(img, 10, method=method))
        contrast = (high - low) / np.maximum(10, high + low)
        return (contrast if force is None else force), high, low
    return contrast_grey


MUTANTS = {
    "warp border replicates instead of reading 0": lambda: [(recog, "warp_perspective_u8", _warp_variant(border_zero=False))],
    "warp coordinates floored instead of rint": lambda: [(recog, "warp_perspective_u8", _warp_variant(rounder=np.floor))],
    "bilinear coefficients from a double fx": lambda: [(imgproc, "linear_coeffs", _coeffs_from_double)],
    "bilinear clamp at the last column removed": lambda: [(imgproc, "resize_linear_u8", _resize_without_last_clamp(imgproc.resize_linear_u8))],
    "horizontal box not clamped to the page": lambda: [(recog, "get_image_list", _unclamped_image_list(recog.get_image_list))],
    "padding filled with 0": lambda: [(recog, "align_collate_one", _collate_variant(recog.align_collate_one, pad_zero=True))],
    "fw floored instead of ceiled": lambda: [(recog, "align_collate_one", _collate_variant(recog.align_collate_one, floor_fw=True))],
    "np.rot90 turned the other way": lambda: [(cc, "_rot90", lambda m, k: np.rot90(m, -k))],
    "contrast LUT always applied": lambda: [(recog, "contrast_grey", _contrast_variant(recog.contrast_grey, force=-1.0))],
    "contrast LUT never applied": lambda: [(recog, "contrast_grey", _contrast_variant(recog.contrast_grey, force=2.0))],
    "percentile by nearest rank": lambda: [(recog, "contrast_grey", _contrast_variant(recog.contrast_grey, method="nearest"))],
}


def test_restated_pieces_equal_the_oracle(monkeypatch, baseline):
    """the un-mutated forms of the restatements used by the mutants change nothing"""
    monkeypatch.setattr(recog, "warp_perspective_u8", _warp_variant())
    monkeypatch.setattr(recog, "contrast_grey", _contrast_variant(recog.contrast_grey))
    monkeypatch.setattr(recog, "align_collate_one", _collate_variant(recog.align_collate_one))
    assert _changed(baseline, _outputs()) == []


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_case_set_sees_mutant(monkeypatch, baseline, mutant):
    for target, name, value in MUTANTS[mutant]():
        monkeypatch.setattr(target, name, value)
    changed = _changed(baseline, _outputs())
    assert changed, f"mutant '{mutant}' changes no output of the case set: extend the cases"
