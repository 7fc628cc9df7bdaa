"""The crop stage's shared cases (tests/test_crop_cases_cpu.py, tests/test_gpu_crops.py, tests/test_gpu_stages.py): one gray page, boxes that
reach every regime of the stage between the detector's boxes and the recogniser's input (crnn_misc.hip's crop kernels, recognizer.cpp's
planner), a pure-Python classifier of a box into its regime, and the reference builders on oracle/recog.py.  Everything here is bit exact.

Regime of a w x h source (a clamped horizontal box, or a free box's warped crop), as plan_sizes / crop_resize_kernel / crop_final_kernel see it:
  stage A   same   cv2.resize target == source: a copy
            area2  source == 2 x target on both axes: cv::resize's INTER_AREA shortcut
            up     bilinear, the short side is below 64
            down   bilinear, the short side is above 64 (scale > 1 coefficients)
  tall      the resize target is not 64 rows high (the box is taller than wide): both Pillow passes of AlignCollate run
  padded    AlignCollate's content width fw is below the padded width imgW: NormalizePAD replicates the last content column
"""
import functools
import math

import numpy as np

from oracle import recog

H, W = 300, 420
NOISE_W = 260                  # columns [0, 260): full-range noise; columns [260, 420): four bands of BAND_H rows
BAND_H = 75
BANDS = ("gradient", "low", "narrow", "black")
SENTINEL = 0x7FC1              # 16-bit pattern no mode writes: a NaN as bf16 and as fp16, far above the exact mode's codes 1..256


def band_origin(name):
    return NOISE_W, BANDS.index(name) * BAND_H


# the `same` box of a band (100 x 64 at this offset from the band's origin): in the low band its 6400 pixels are set by count, see make_page
SAME_IN_BAND = (10, 110, 5, 69)


@functools.lru_cache(maxsize=None)
def make_page():
    """uint8 [300][420]: noise | gradient, low contrast (100..140), narrow (10th and 90th percentile fewer than 10 apart), near black (0..6)"""
    rng = np.random.default_rng(20240)
    page = rng.integers(0, 256, (H, W), dtype=np.uint8)
    bw = W - NOISE_W
    x0, y0 = band_origin("gradient")
    yy, xx = np.mgrid[0:BAND_H, 0:bw]
    page[y0:y0 + BAND_H, x0:] = (20 + xx * 1.3 + yy * 0.4).astype(np.uint8)
    x0, y0 = band_origin("low")
    page[y0:y0 + BAND_H, x0:] = rng.integers(100, 141, (BAND_H, bw), dtype=np.uint8)
    # the low band's `same` crop: exactly 640 of its 6400 pixels are <= 104, the others >= 108, so np.percentile(.., 10) (virtual index
    # 639.9) interpolates between 104 and 108: 107.6 where a nearest-rank percentile says 108
    n = (SAME_IN_BAND[1] - SAME_IN_BAND[0]) * (SAME_IN_BAND[3] - SAME_IN_BAND[2])
    vals = np.concatenate([rng.integers(100, 104, 639), [104, 108], rng.integers(108, 141, n - 641)]).astype(np.uint8)
    rng.shuffle(vals)
    page[y0 + SAME_IN_BAND[2]:y0 + SAME_IN_BAND[3], x0 + SAME_IN_BAND[0]:x0 + SAME_IN_BAND[1]] = vals.reshape(64, 100)
    x0, y0 = band_origin("narrow")
    page[y0:y0 + BAND_H, x0:] = rng.integers(120, 127, (BAND_H, bw), dtype=np.uint8)
    x0, y0 = band_origin("black")
    page[y0:y0 + BAND_H, x0:] = rng.integers(0, 7, (BAND_H, bw), dtype=np.uint8)
    page.setflags(write=False)
    return page


def _rot_quad(cx, cy, w, h, deg, jitter=(), shear=0.0):
    """corners tl, tr, br, bl of a w x h rectangle turned by deg about (cx, cy), sheared along its own x axis, each corner moved by jitter"""
    a = math.radians(deg)
    ca, sa = math.cos(a), math.sin(a)
    pts = []
    for i, (u, v) in enumerate(((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))):
        u += shear * v
        jx, jy = jitter[i] if jitter else (0.0, 0.0)
        pts.append([cx + u * ca - v * sa + jx, cy + u * sa + v * ca + jy])
    return pts


# horizontal boxes: (name, [x_min, x_max, y_min, y_max])
_HORI = [
    ("area2 200x128", [10, 210, 5, 133]),
    ("bilinear neighbour 201x128", [10, 211, 5, 133]),
    ("same 100x64", [30, 130, 150, 214]),
    ("same 192x64 unpadded", [20, 212, 200, 264]),
    ("down 200x190", [40, 240, 100, 290]),
    ("down 370x100", [20, 390, 50, 150]),
    ("down whole page", [0, W, 0, H]),
    ("same tall 64x128", [100, 164, 20, 148]),
    ("area2 tall 128x256", [60, 188, 10, 266]),
    ("up tall 20x300", [200, 220, 0, 300]),
    ("up tall 3x40", [250, 253, 100, 140]),
    ("width 1 (1x64)", [255, 256, 150, 214]),
    ("height 1 (40x1)", [100, 140, 280, 281]),
    ("up negative x_min", [-7, 90, 240, 270]),
    ("up over the top edge", [50, 120, -10, 25]),
    ("past the right edge", [380, 450, 30, 70]),
    ("past the bottom edge", [150, 230, 280, 330]),
    ("clamped width 0", [W, W + 40, 10, 40]),
]
for _b in BANDS:
    _x, _y = band_origin(_b)
    _HORI += [
        (f"{_b} band same 100x64", [_x + SAME_IN_BAND[0], _x + SAME_IN_BAND[1], _y + SAME_IN_BAND[2], _y + SAME_IN_BAND[3]]),
        (f"{_b} band up 120x30", [_x + 5, _x + 125, _y + 20, _y + 50]),
        (f"{_b} band down 150x70", [_x + 2, _x + 152, _y + 2, _y + 72]),
        (f"{_b} band tall 20x70", [_x + 130, _x + 150, _y + 2, _y + 72]),
    ]

# free boxes: (name, [[x, y] x 4] tl, tr, br, bl)
_FREE = [
    ("free inside", _rot_quad(130.0, 150.0, 150.0, 40.0, 12.0, jitter=((0.3, -0.2), (-0.4, 0.6), (0.2, 0.1), (-0.1, -0.5)), shear=0.1)),
    ("free over the top-left corner", _rot_quad(20.0, 15.0, 120.0, 36.0, -20.0)),
    ("free over the bottom-right corner", _rot_quad(400.0, 290.0, 110.0, 30.0, 15.0)),
    ("free half-pixel 256x128 (area2)", [[40.5, 30.5], [296.5, 30.5], [296.5, 158.5], [40.5, 158.5]]),
    ("free steep tall", _rot_quad(320.0, 120.0, 30.0, 150.0, 10.0, shear=0.05)),
    ("free narrower than a pixel", [[50.0, 50.0], [50.6, 50.2], [50.6, 90.2], [50.0, 90.0]]),
]

HORI_NAMES = [n for n, _ in _HORI]
HORI = [b for _, b in _HORI]
FREE_NAMES = [n for n, _ in _FREE]
FREE = [q for _, q in _FREE]
NAMES = HORI_NAMES + FREE_NAMES            # box k of every device entry point: the horizontal boxes, then the free ones
SKIPPED = {"clamped width 0", "free narrower than a pixel"}


# ------------------------------------------------------------------------------------------------ the classifier (no oracle, no library)
def plan_sizes(w, h):
    """(rw, rh, imgW, fw) of a w x h source: get_image_list's resize target and own padded width, AlignCollate's content width"""
    ratio = w / h
    if ratio < 1.0:
        ratio = 1.0 / ratio
        rw, rh = 64, int(64 * ratio)
    else:
        rw, rh = int(64 * ratio), 64
    imgW = math.ceil(max(ratio, 1.0)) * 64
    fw = min(imgW, math.ceil(64 * (rw / rh)))
    return rw, rh, imgW, fw


def classify(w, h):
    """(stage-A regime, tall, padded) of a w x h source"""
    rw, rh, imgW, fw = plan_sizes(w, h)
    if (rw, rh) == (w, h):
        regime = "same"
    elif (w, h) == (2 * rw, 2 * rh):
        regime = "area2"
    elif rw <= w and rh <= h:
        regime = "down"
    elif rw >= w and rh >= h:
        regime = "up"
    else:
        raise AssertionError(f"{w} x {h} -> {rw} x {rh}: one axis grows, the other shrinks")
    return regime, rh != 64, fw != imgW


def regime_name(cell):
    return f"{cell[0]}{' tall' if cell[1] else ''}{' padded' if cell[2] else ' fw == imgW'}"


def clamped(box, h=H, w=W):
    """get_image_list's clamp of a horizontal box: (x_min, y_min, width, height)"""
    x_min, x_max, y_min, y_max = max(0, box[0]), min(box[1], w), max(0, box[2]), min(box[3], h)
    return x_min, y_min, x_max - x_min, y_max - y_min


def free_size(quad):
    """four_point_transform's (maxWidth, maxHeight), float32 as numpy computes them"""
    r = np.asarray(quad, dtype=np.float32)
    tl, tr, br, bl = r
    d = lambda p, q: int(np.sqrt(((p[0] - q[0]) ** 2) + ((p[1] - q[1]) ** 2)))
    return max(d(br, bl), d(tr, tl)), max(d(tr, br), d(tl, bl))


def source_size(k, hori=None, free=None, shape=(H, W)):
    """(w, h) of box k's source; a side <= 0: the box is skipped"""
    hori = HORI if hori is None else hori
    free = FREE if free is None else free
    if k < len(hori):
        return clamped(hori[k], *shape)[2:]
    return free_size(free[k - len(hori)])


def box_regime(k):
    w, h = source_size(k)
    return regime_name(classify(w, h)) if w > 0 and h > 0 else "skipped"


# ------------------------------------------------------------------------------------------------ references (oracle/recog.py)
def stage_a(page, hori, free):
    """per box (horizontal, then free): None for a box get_image_list drops (or raises on: empty after clamping), else (crop uint8, own imgW)"""
    out = []
    for b in hori:
        try:
            il, mw = recog.get_image_list([b], [], page)
        except ValueError:
            il = []
        out.append((il[0][1], int(mw)) if il else None)
    for q in free:
        il, mw = recog.get_image_list([], [q], page)
        out.append((il[0][1], int(mw)) if il else None)
    return out


@functools.lru_cache(maxsize=None)
def stage_a_cases():
    return stage_a(make_page(), HORI, FREE)


_rot90 = np.rot90              # (the sensitivity test turns it the other way)


def collate(crop, imgW, contrast, rot=0):
    """AlignCollate of np.rot90(crop, rot) at the padded width imgW: float32 [64][imgW]"""
    c = np.ascontiguousarray(_rot90(crop, rot)) if rot else crop
    return recog.align_collate_one(c, 64, imgW, adjust_contrast=contrast)[0]


def codes_from_tensor(t):
    """the uint8 image behind AlignCollate's float32 tensor (ToTensor, sub_(0.5).div_(0.5) undone)"""
    return np.rint((t.astype(np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)).astype(np.int32)


def to_el(t, el):
    """what crop_final_kernel stores for the float32 tensor t, as int16 bit patterns: bf16 / fp16 values, or the exact mode's codes
    1 + grey level (the pad columns carry the last content column's code, as t carries its value)"""
    import torch

    if el == "exact":
        return (codes_from_tensor(t) + 1).astype(np.int16)
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[el]
    return torch.from_numpy(np.array(t, dtype=np.float32)).to(dt).view(torch.int16).numpy()


@functools.lru_cache(maxsize=None)
def reference(k, imgW, contrast, rot=0):
    """float32 [64][imgW] of box k of the shared list, or None when it is skipped; imgW None: its own padded width"""
    item = stage_a_cases()[k]
    if item is None:
        return None
    t = collate(item[0], item[1] if imgW is None else imgW, contrast, rot)
    t.setflags(write=False)
    return t


def first_diff(got, want):
    """(row, column) of the first differing element of two [64][w] arrays, None when they are equal"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return tuple(int(v) for v in bad[0]) if len(bad) else None


def describe(k, names=None, regime=None):
    return f"box {k} ({(names or NAMES)[k]}; {regime or box_regime(k)})"


def assert_same(got, want, what):
    """bit-exact comparison of one crop; the message carries `what` and the first differing (row, column) with both values"""
    d = first_diff(got, want)
    if d is not None:
        n = int((np.asarray(got) != np.asarray(want)).sum())
        raise AssertionError(f"{what}: {n} elements differ, first at (row {d[0]}, column {d[1]}): got {int(np.asarray(got)[d])}, want {int(np.asarray(want)[d])}")
