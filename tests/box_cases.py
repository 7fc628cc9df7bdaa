"""Designed heat maps and threshold settings for the box stage (threshold, CCL, statistics, acceptance, row extremes), shared by
tests/test_box_cases_cpu.py (oracle only) and tests/test_gpu_box_knobs.py (device against oracle).

Every map is a float32 ``(text, link)`` pair ``[h, w]``; every value is written as an exact float32.  What each shape is for:

``edges()``        component maxima on either side of ``text_threshold`` by one ulp (upstream compares the float32 maximum with the
                   Python float in double: ``f32(0.7)`` and ``f32(0.9)`` lie BELOW 0.7 and 0.9, ``f32(0.5)`` is 0.5), areas of 9 / 10 / 11
                   pixels around ``size < 10``, pixels exactly at and one ulp above ``low_text`` / ``link_threshold`` (``>``, not
                   ``>=``) alone and as the rim of an accepted block, and runs longer than a wave whose only accepted pixel is at the
                   run's end (the segmented maximum of ``ccl_stats_kernel``).
``bridges()``      link strips and faint text tails between the two thresholds: what is one component depends on ``low_text`` and
                   ``link_threshold`` separately; link-only pixels count towards the area, never towards the row extremes.
``narrow()``       maps 16 and 48 pixels wide: four rows per 64-pixel wave, and rows cut by the wave segments at a different offset on
                   every row.
``page_seams()``   three 16 x 32 pages whose foreground meets across the page borders of the flattened batch.
``wrap_batch()``   two 1536 x 1408 pages: 4,325,376 pixels, more than the 16384 * 256 = 4,194,304 that one grid round of the CCL kernels
                   covers -- blobs at the pixel where the second round starts and in the batch's last wave.
"""
import numpy as np

f32 = np.float32


def up(v, n=1):
    """The float32 ``n`` ulps above ``v``."""
    v = f32(v)
    for _ in range(n):
        v = np.nextafter(v, f32(2))
    return v


def down(v, n=1):
    v = f32(v)
    for _ in range(n):
        v = np.nextafter(v, f32(-1))
    return v


# (text_threshold, low_text, link_threshold)
SETTINGS = [
    (0.7, 0.4, 0.4),
    (0.7, 0.4, 0.2),
    (0.7, 0.2, 0.4),
    (0.7, 0.2, 0.2),
    (0.5, 0.4, 0.4),
    (0.9, 0.25, 0.6),
]


def setting_kw(s):
    return {"text_threshold": s[0], "low_text": s[1], "link_threshold": s[2]}


def _maps(h, w):
    return np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)


def _rect(m, y, x, h, w, v):
    m[y:y + h, x:x + w] = f32(v)


# ------------------------------------------------------------------------------------------------ edges
# name -> (y, x) of one pixel of the block; 3 rows x 4 columns of one value unless said otherwise
EDGE_BLOCKS = {
    "max_0.7": (1, 2), "max_0.7_up": (1, 10), "max_0.7_down": (1, 18), "max_0.5": (1, 26), "max_0.5_down": (1, 34),
    "max_0.9": (1, 42), "max_0.9_up": (1, 50),
    "area_9": (1, 60), "area_10": (1, 68), "area_11": (1, 76),
    "all_0.4": (8, 2), "all_0.4_up": (8, 10), "all_0.2": (8, 18), "all_0.2_up": (8, 26),
    "rim_0.4": (8, 37), "rim_0.4_up": (8, 47), "rim_0.2": (8, 57), "rim_0.2_up": (8, 67),
    "link_0.4": (8, 80), "link_0.4_up": (8, 100), "link_0.2": (8, 120), "link_0.2_up": (8, 140),
    "under_0.4": (14, 2), "under_0.4_up": (14, 22), "under_0.2": (14, 42), "under_0.2_up": (14, 62),
    "run_max_last": (20, 30), "run_max_segment_start": (24, 30), "run_low": (28, 30), "run_high_neighbour": (28, 62),
}
EDGE_VALUES = {
    "max_0.7": f32(0.7), "max_0.7_up": up(0.7), "max_0.7_down": down(0.7), "max_0.5": f32(0.5), "max_0.5_down": down(0.5),
    "max_0.9": f32(0.9), "max_0.9_up": up(0.9),
    "all_0.4": f32(0.4), "all_0.4_up": up(0.4), "all_0.2": f32(0.2), "all_0.2_up": up(0.2),
}
RUN_X0, RUN_X1 = 30, 140       # the long runs cover x in [30, 140]: 111 pixels, three wave segments (rows 20, 24, 28 start on a segment)


def edges():
    """48 x 160.  Row band y 1..3: one 3 x 4 block per maximum (EDGE_VALUES), then blocks of 9, 10 and 11 pixels at 0.9.
    Row band y 7..11: blocks wholly at / one ulp above 0.4 and 0.2; 3 x 4 blocks at 0.95 inside a one-pixel rim at those four values;
    3 x 4 blocks at 0.95 with a six-pixel link strip at those four values to their right.
    Row band y 14..16: 3 x 4 blocks at 0.95 with a six-pixel link strip at 0.9 to their right, the TEXT under the strip at those four values:
    pixels of the component either way, text pixels (row extremes) only above ``low_text``.
    Rows 20 and 24: runs x 30..140 at 0.45 whose only pixel above (0.95) is the last one (x 140) / the first of the run's last wave
    segment (x 128).  Row 28: a run x 30..60 at 0.45 (rejected at 0.5 and above), one background pixel, a run x 62..75 at 0.95."""
    text, link = _maps(48, 160)
    for name, v in EDGE_VALUES.items():
        y, x = EDGE_BLOCKS[name]
        _rect(text, y, x, 3, 4, v)
    y, x = EDGE_BLOCKS["area_9"]
    _rect(text, y, x, 3, 3, 0.9)
    y, x = EDGE_BLOCKS["area_10"]
    _rect(text, y, x, 3, 3, 0.9)
    text[y, x + 3] = f32(0.9)
    y, x = EDGE_BLOCKS["area_11"]
    _rect(text, y, x, 3, 4, 0.9)
    text[y + 2, x + 3] = 0
    for name, v in (("rim_0.4", f32(0.4)), ("rim_0.4_up", up(0.4)), ("rim_0.2", f32(0.2)), ("rim_0.2_up", up(0.2))):
        y, x = EDGE_BLOCKS[name]
        _rect(text, y - 1, x - 1, 5, 6, v)
        _rect(text, y, x, 3, 4, 0.95)
    for name, v in (("link_0.4", f32(0.4)), ("link_0.4_up", up(0.4)), ("link_0.2", f32(0.2)), ("link_0.2_up", up(0.2))):
        y, x = EDGE_BLOCKS[name]
        _rect(text, y, x, 3, 4, 0.95)
        _rect(link, y + 1, x + 4, 1, 6, v)
    for name, v in (("under_0.4", f32(0.4)), ("under_0.4_up", up(0.4)), ("under_0.2", f32(0.2)), ("under_0.2_up", up(0.2))):
        y, x = EDGE_BLOCKS[name]
        _rect(text, y, x, 3, 4, 0.95)
        _rect(link, y + 1, x + 4, 1, 6, 0.9)
        _rect(text, y + 1, x + 4, 1, 6, v)
    _rect(text, 20, RUN_X0, 1, RUN_X1 - RUN_X0 + 1, 0.45)
    text[20, RUN_X1] = f32(0.95)
    _rect(text, 24, RUN_X0, 1, RUN_X1 - RUN_X0 + 1, 0.45)
    text[24, 128] = f32(0.95)
    _rect(text, 28, 30, 1, 31, 0.45)
    _rect(text, 28, 62, 1, 14, 0.95)
    return text, link


# ------------------------------------------------------------------------------------------------ bridges
def bridges():
    """48 x 160.
    (a) y 2..5: two 4 x 8 text blocks at 0.9 (x 4..11, x 24..31) joined by a link strip at 0.3 (y 3..4, x 12..23).
    (b) y 10..13: a 4 x 8 text block at 0.9 (x 4..11) with a text tail at 0.3 (y 11..12, x 12..25).
    (c) y 2..6, x 50..60: link 0.9 over text 0 -- area without text, rejected at every setting.
    (d) y 10..13, x 50..57: a text block at 0.9; link strip at 0.5 over text 0 (y 11, x 58..75) touching it.
    (e) y 20..23: two text blocks at 1.0 (x 4..11, x 24..31) joined by a link strip at 0.5 (y 21..22, x 12..23).
    (f) y 30..33: a text block at 1.0 (x 4..11) with a text tail at 0.22 (y 31..32, x 12..25).
    (g) y 20..23, x 60..67: a text block at 1.0; link 0.5 over text 0 on y 18..25, x 56..59: rows of the component without a text pixel.
    (h) y 30..33, x 60..67: a text block at 1.0 whose left half lies under link 0.9 as well (both maps foreground)."""
    text, link = _maps(48, 160)
    _rect(text, 2, 4, 4, 8, 0.9)
    _rect(text, 2, 24, 4, 8, 0.9)
    _rect(link, 3, 12, 2, 12, 0.3)
    _rect(text, 10, 4, 4, 8, 0.9)
    _rect(text, 11, 12, 2, 14, 0.3)
    _rect(link, 2, 50, 5, 11, 0.9)
    _rect(text, 10, 50, 4, 8, 0.9)
    _rect(link, 11, 58, 1, 18, 0.5)
    _rect(text, 20, 4, 4, 8, 1.0)
    _rect(text, 20, 24, 4, 8, 1.0)
    _rect(link, 21, 12, 2, 12, 0.5)
    _rect(text, 30, 4, 4, 8, 1.0)
    _rect(text, 31, 12, 2, 14, 0.22)
    _rect(text, 20, 60, 4, 8, 1.0)
    _rect(link, 18, 56, 8, 4, 0.5)
    _rect(text, 30, 60, 4, 8, 1.0)
    _rect(link, 30, 60, 4, 4, 0.9)
    return text, link


# ------------------------------------------------------------------------------------------------ narrow
def _narrow_16x16():
    text, link = _maps(16, 16)
    _rect(text, 0, 0, 8, 1, 0.9)            # vertical stroke on x = 0 ...
    _rect(text, 0, 1, 1, 4, 0.9)            # ... with a hook along the first row: 12 pixels
    _rect(text, 2, 12, 4, 4, 1.0)           # blob touching x = w - 1
    _rect(text, 9, 0, 1, 16, 0.9)           # a full-width row
    _rect(text, 11, 10, 2, 6, 1.0)          # ends on (12, 15) ...
    _rect(text, 13, 0, 2, 6, 0.9)           # ... and this one starts on (13, 0), the next pixel of the flattened map: not connected
    return text, link


def _narrow_64x16():
    text, link = _maps(64, 16)
    _rect(text, 1, 2, 40, 1, 0.9)           # long one-pixel stroke: ten waves
    _rect(text, 0, 13, 41, 2, 1.0)          # long two-pixel stroke from the first row
    _rect(text, 5, 6, 12, 3, 0.9)
    _rect(link, 10, 9, 2, 4, 0.9)           # link bridge from the middle block to the right stroke
    _rect(text, 44, 0, 1, 16, 0.9)          # one full-width row
    _rect(text, 47, 0, 2, 16, 1.0)          # two full-width rows
    _rect(text, 51, 11, 3, 5, 0.9)          # ends on (53, 15)
    _rect(text, 54, 0, 3, 5, 1.0)           # starts on (54, 0)
    _rect(text, 59, 0, 5, 4, 0.9)           # bottom-left corner
    _rect(text, 60, 9, 4, 7, 1.0)           # bottom-right corner, last pixel of the map
    return text, link


# the component of the 48-wide maps that the wave segments cut: rows NARROW_CUT_ROWS, x in [NARROW_CUT_X0, NARROW_CUT_X1]
NARROW_CUT_ROWS = range(1, 8)
NARROW_CUT_X0, NARROW_CUT_X1 = 10, 40


def _narrow_16x48():
    text, link = _maps(16, 48)
    for y in NARROW_CUT_ROWS:               # segment boundaries at x = 16 (rows 1, 5), x = 32 (rows 2, 6), none on row 3, x = 0 on row 4
        _rect(text, y, NARROW_CUT_X0, 1, NARROW_CUT_X1 - NARROW_CUT_X0 + 1, 0.9 if y & 1 else 1.0)
    _rect(text, 0, 44, 3, 4, 0.9)           # ends on (2, 47)
    _rect(text, 3, 0, 4, 3, 1.0)            # starts on (3, 0)
    _rect(text, 10, 0, 1, 48, 0.9)          # a full-width row
    _rect(text, 12, 20, 4, 3, 1.0)          # strokes down to the last row
    _rect(text, 12, 45, 4, 3, 0.9)
    _rect(text, 12, 0, 4, 1, 0.9)
    _rect(text, 12, 1, 1, 9, 0.9)
    return text, link


def _narrow_40x48():
    text, link = _maps(40, 48)
    for y in NARROW_CUT_ROWS:
        _rect(text, y, NARROW_CUT_X0, 1, NARROW_CUT_X1 - NARROW_CUT_X0 + 1, 1.0 if y & 1 else 0.9)
    for k in range(12):                     # a staircase: a slanted component, two pixels per step, through several segment boundaries
        _rect(text, 10 + k, 4 + 3 * k, 2, 4, 0.9)
    _rect(text, 10, 30, 1, 18, 1.0)         # ends on (10, 47)
    _rect(text, 11, 0, 1, 3, 0.9)           # starts on (11, 0), the next pixel of the flattened map: another component
    _rect(text, 12, 0, 4, 2, 1.0)
    _rect(text, 26, 0, 2, 48, 0.9)          # two full-width rows
    _rect(text, 28, 5, 9, 1, 0.9)           # ... with strokes hanging from them
    _rect(text, 28, 46, 12, 1, 1.0)
    _rect(link, 30, 6, 2, 30, 0.9)          # and a link-only bar joined to the first stroke
    _rect(text, 36, 10, 4, 30, 1.0)         # bottom block down to the last row
    text[37:39, 12:38] = 0                  # hollow: one component with two long runs per row
    return text, link


def narrow():
    """{name: (text, link)} for 16 x 16, 64 x 16, 16 x 48 and 40 x 48 maps (h x w), each with its left-right mirror image (another
    offset of every run inside its wave, and a second page of the same shape for the batched run)."""
    out = {}
    for name, fn in (("16x16", _narrow_16x16), ("64x16", _narrow_64x16), ("16x48", _narrow_16x48), ("40x48", _narrow_40x48)):
        text, link = fn()
        out[name] = (text, link)
        out[name + "_mirror"] = (np.ascontiguousarray(text[:, ::-1]), np.ascontiguousarray(link[:, ::-1]))
    return out


def designed_maps():
    """{name: (text, link)}: every single-page map."""
    out = {"edges": edges(), "bridges": bridges()}
    out.update({"narrow_" + k: v for k, v in narrow().items()})
    return out


# ------------------------------------------------------------------------------------------------ page seams
def page_seams():
    """float32 [3, 16, 32, 2].  Page 0: rows 14..15, x 6..15 and a block y 12..15, x 28..31 that ends on the page's last pixel.  Page 1:
    rows 0..1, x 6..15 (the same columns), a block y 0..3, x 0..3 from the page's first pixel, and a fully foreground last row.  Page 2: a
    fully foreground first row and a block in the middle.  Five components reach a page border from either side; none crosses it."""
    heat = np.zeros((3, 16, 32, 2), np.float32)
    _rect(heat[0, ..., 0], 14, 6, 2, 10, 0.9)
    _rect(heat[0, ..., 0], 12, 28, 4, 4, 1.0)
    _rect(heat[1, ..., 0], 0, 6, 2, 10, 0.9)
    _rect(heat[1, ..., 0], 0, 0, 4, 4, 1.0)
    _rect(heat[1, ..., 0], 15, 0, 1, 32, 0.9)
    _rect(heat[2, ..., 0], 0, 0, 1, 32, 1.0)
    _rect(heat[2, ..., 0], 6, 10, 4, 9, 0.9)
    return heat


# ------------------------------------------------------------------------------------------------ grid-stride wrap
WRAP_H, WRAP_W = 1536, 1408
WRAP_ROUND = 16384 * 256                     # pixels per grid round of the CCL kernels: the second round starts at this flattened index
# 4,194,304 = page 1, row 1442, x 1280.  The batch has 4,325,376 = 67,584 * 64 pixels: it ends on a whole wave, inside the second round.
# (page, y, x, rows, columns, value), text map only
WRAP_BLOBS = [
    (0, 3, 5, 6, 40, 0.9),                   # ordinary blobs of the first round
    (0, 700, 0, 5, 30, 1.0),                 # touching x = 0
    (0, 900, 1378, 5, 30, 0.9),              # touching x = w - 1
    (0, 1532, 100, 4, 50, 1.0),              # page 0's last rows ...
    (1, 0, 100, 4, 50, 0.9),                 # ... page 1's first rows, same columns: two components
    (1, 1442, 1250, 2, 81, 0.9),             # horizontal run THROUGH flattened pixel 4,194,304 (x 1280 of its first row)
    (1, 1420, 600, 51, 2, 1.0),              # vertical stroke crossing row 1442: its upper part in the first round, the rest in the second
    (1, 1400, 1290, 41, 2, 0.9),             # vertical stroke ending one row above the run (row 1441 stays background)
    (1, 1500, 640, 6, 24, 1.0),              # an ordinary blob of the second round
    (1, 1532, 1344, 4, 64, 0.9),             # the batch's last wave: row 1535, x 1344..1407, and three rows above it
]


def wrap_rows(page, y0, y1):
    """Rows [y0, y1) of ``page`` of the wrap batch -> float32 [y1 - y0, WRAP_W, 2]."""
    band = np.zeros((y1 - y0, WRAP_W, 2), np.float32)
    for p, y, x, h, w, v in WRAP_BLOBS:
        a, b = max(y, y0), min(y + h, y1)
        if p == page and a < b:
            band[a - y0:b - y0, x:x + w, 0] = f32(v)
    return band


def wrap_batch():
    """float32 [2, 1536, 1408, 2]: both pages empty apart from WRAP_BLOBS."""
    return np.stack([wrap_rows(0, 0, WRAP_H), wrap_rows(1, 0, WRAP_H)])
