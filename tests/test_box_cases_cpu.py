"""CPU: the designed box-stage maps of tests/box_cases.py against the rules of getDetBoxes_core, oracle only.  The expectations for
``edges`` are written out from upstream's rules (``size < 10``, ``max(textmap) < text_threshold`` in double, ``threshold`` with ``>``),
not recorded from a run: they pin the oracle that tests/test_gpu_box_knobs.py then compares the device with."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_cases as bc  # noqa: E402
from oracle import boxes as obox  # noqa: E402

NONE, REJECTED, ACCEPTED = "no component", "rejected", "accepted"

# (text_threshold, low_text, link_threshold) = (0.7, 0.4, 0.4)
EDGES_AT_07 = {
    "max_0.7": REJECTED,            # float(f32(0.7)) = 0.699999988... < 0.7
    "max_0.7_up": ACCEPTED,         # 0.70000005 >= 0.7
    "max_0.7_down": REJECTED,
    "max_0.5": REJECTED, "max_0.5_down": REJECTED,
    "max_0.9": ACCEPTED, "max_0.9_up": ACCEPTED,
    "area_9": REJECTED, "area_10": ACCEPTED, "area_11": ACCEPTED,
    "all_0.4": NONE,                # text > f32(0.4) is false on every pixel
    "all_0.4_up": REJECTED,         # a 12-pixel component whose maximum is below 0.7
    "all_0.2": NONE, "all_0.2_up": NONE,
    "rim_0.4": ACCEPTED, "rim_0.4_up": ACCEPTED, "rim_0.2": ACCEPTED, "rim_0.2_up": ACCEPTED,
    "link_0.4": ACCEPTED, "link_0.4_up": ACCEPTED, "link_0.2": ACCEPTED, "link_0.2_up": ACCEPTED,
    "under_0.4": ACCEPTED, "under_0.4_up": ACCEPTED, "under_0.2": ACCEPTED, "under_0.2_up": ACCEPTED,
    "run_max_last": ACCEPTED, "run_max_segment_start": ACCEPTED,
    "run_low": REJECTED, "run_high_neighbour": ACCEPTED,
}
# (0.5, 0.4, 0.4): the three blocks between 0.5 and 0.7 join; f32(0.5) is exactly 0.5, one ulp below is not
EDGES_AT_05 = dict(EDGES_AT_07, **{"max_0.7": ACCEPTED, "max_0.7_down": ACCEPTED, "max_0.5": ACCEPTED, "max_0.5_down": REJECTED})
# component areas: the 3 x 4 core alone is 12, core + one-pixel rim 5 x 6 = 30, core + six link pixels 18
AREAS_LOW_04 = {"rim_0.4": 12, "rim_0.4_up": 30, "rim_0.2": 12, "rim_0.2_up": 12,
                "link_0.4": 12, "link_0.4_up": 18, "link_0.2": 12, "link_0.2_up": 12, "area_9": 9, "area_10": 10, "area_11": 11,
                "under_0.4": 18, "under_0.4_up": 18, "under_0.2": 18, "under_0.2_up": 18}      # the link strip (0.9) holds them at any text value
AREAS_LOW_02 = {"rim_0.4": 30, "rim_0.4_up": 30, "rim_0.2": 12, "rim_0.2_up": 30,
                "link_0.4": 18, "link_0.4_up": 18, "link_0.2": 12, "link_0.2_up": 18}


def _status(setting):
    text, link = bc.edges()
    det, labels, mapper = obox.get_det_boxes_core(text, link, setting[0], setting[2], setting[1])
    out, area = {}, {}
    for name, (y, x) in bc.EDGE_BLOCKS.items():
        k = int(labels[y, x])
        out[name] = NONE if k == 0 else (ACCEPTED if k in mapper else REJECTED)
        area[name] = int((labels == k).sum()) if k else 0
    return out, area, det


def test_edges_follow_the_rules_at_0_7_and_0_5():
    got, area, det = _status((0.7, 0.4, 0.4))
    assert got == EDGES_AT_07
    assert len(det) == sum(v == ACCEPTED for v in EDGES_AT_07.values()) == 20
    assert {k: area[k] for k in AREAS_LOW_04} == AREAS_LOW_04
    got, area, det = _status((0.5, 0.4, 0.4))
    assert got == EDGES_AT_05
    assert len(det) == 23
    got, area, _ = _status((0.7, 0.2, 0.2))
    assert {k: area[k] for k in AREAS_LOW_02} == AREAS_LOW_02
    assert got["all_0.2"] == NONE and got["all_0.2_up"] == REJECTED and got["all_0.4"] == REJECTED
    # (0.9, ...): float(f32(0.9)) = 0.89999998 < 0.9 -- every block AT f32(0.9) goes, one ulp above stays
    got, _, _ = _status((0.9, 0.25, 0.6))
    assert got["max_0.9"] == REJECTED and got["max_0.9_up"] == ACCEPTED and got["area_11"] == REJECTED and got["rim_0.4"] == ACCEPTED


def test_edges_one_polygon_by_hand():
    """The block one ulp above 0.7: 3 x 4 pixels at x 10..13, y 1..3.  size 12, niter = int(sqrt(12 * 3 / 12) * 2) = 3: a 4 x 4 rect kernel
    with its anchor at (2, 2) (cv2.dilate's centre anchor is ksize // 2): dst(x) reads src(x - 2 .. x + 1), so a pixel spreads one to the left
    / up and two to the right / down: x 9..15, y 0..5.  An axis-aligned rectangle is its own minimum-area box; the corners are doubled
    (the heat map has half the page's resolution) and divided by ``ratio``, then truncated."""
    text, link = bc.edges()
    _, _, polys = obox.detect_from_heatmap(text, link, 1.0)
    assert [18, 0, 30, 0, 30, 10, 18, 10] in [list(map(int, p)) for p in polys]
    _, _, polys = obox.detect_from_heatmap(text, link, 1.5)
    assert [12, 0, 20, 0, 20, 6, 12, 6] in [list(map(int, p)) for p in polys]          # 18 / 1.5, 30 / 1.5, 10 / 1.5 = 6.67


def test_the_segmented_maximum_case_is_what_it_claims():
    """Rows 20 and 24 of ``edges``: runs of more than 64 pixels that start mid-wave (flattened index & 63 != 0) and whose only pixel at or
    above 0.5 is the run's last one / the first of its last wave segment."""
    text, _ = bc.edges()
    w = text.shape[1]
    for y, hot in ((20, bc.RUN_X1), (24, 128)):
        run = text[y, bc.RUN_X0:bc.RUN_X1 + 1]
        assert len(run) > 64 and (y * w + bc.RUN_X0) & 63 != 0
        assert text[y, bc.RUN_X0 - 1] == 0 and text[y, bc.RUN_X1 + 1] == 0 and not text[y - 1].any() and not text[y + 1].any()
        assert [bc.RUN_X0 + int(i) for i in np.nonzero(run >= 0.5)[0]] == [hot]
        assert (y * w + bc.RUN_X0) // 64 + 2 == (y * w + bc.RUN_X1) // 64      # three wave segments
    assert (24 * w + 128) & 63 == 0


def _oracle(text, link, ratio, setting):
    h, f, p = obox.detect_from_heatmap(text, link, ratio, **bc.setting_kw(setting))
    return [list(map(int, q)) for q in p], [list(map(int, b)) for b in h], [np.asarray(b, dtype=np.float64).tolist() for b in f]


def test_every_knob_bites():
    """Any two settings of the grid give different (polys, horizontal, free) on at least one designed map: no threshold can be mixed up
    with another, or left at its default, without a comparison in tests/test_gpu_box_knobs.py changing."""
    for need in [(0.7, 0.4, 0.4), (0.7, 0.4, 0.2), (0.7, 0.2, 0.4), (0.7, 0.2, 0.2), (0.5, 0.4, 0.4), (0.9, 0.25, 0.6)]:
        assert need in bc.SETTINGS
    maps = bc.designed_maps()
    res = {s: {n: _oracle(t, l, 1.0, s) for n, (t, l) in maps.items()} for s in bc.SETTINGS}
    for a, b in itertools.combinations(bc.SETTINGS, 2):
        assert any(res[a][n] != res[b][n] for n in maps), (a, b)
    # the two bridge shapes alone tell the four (low_text, link_threshold) combinations apart
    text, link = bc.bridges()
    four = [_oracle(text[:16, :40], link[:16, :40], 1.0, (0.7, lt, lk)) for lt in (0.4, 0.2) for lk in (0.4, 0.2)]
    assert all(x != y for x, y in itertools.combinations(four, 2))
    assert [len(x[0]) for x in four] == [3, 2, 3, 2]        # the link strip at 0.3 joins the two blocks of (a) below link_threshold 0.3


def test_designed_map_shapes():
    for name, (text, link) in bc.designed_maps().items():
        assert text.dtype == link.dtype == np.float32 and text.shape == link.shape, name
        assert text.shape[0] <= 64 and text.shape[1] <= 160 and text.shape[1] % 16 == 0, name
    nar = bc.narrow()
    assert sorted(v[0].shape for k, v in nar.items() if "mirror" not in k) == [(16, 16), (16, 48), (40, 48), (64, 16)]
    for name in ("16x48", "40x48"):
        text, link = nar[name]
        _, labels, _ = obox.get_det_boxes_core(text, link)
        k = labels[bc.NARROW_CUT_ROWS[0], bc.NARROW_CUT_X0]
        cut = 0
        for y in bc.NARROW_CUT_ROWS:
            assert (labels[y, bc.NARROW_CUT_X0:bc.NARROW_CUT_X1 + 1] == k).all()
            cut += any((y * 48 + x) % 64 == 0 for x in range(bc.NARROW_CUT_X0 + 1, bc.NARROW_CUT_X1 + 1))
        assert cut >= 3, name                               # rows on which a 64-pixel segment boundary falls inside the component
    for name, (text, link) in nar.items():                  # foreground on x = w - 1 of one row and on x = 0 of the next, not connected
        if "mirror" in name:
            continue
        _, labels, _ = obox.get_det_boxes_core(text, link)
        assert any(labels[y, -1] and labels[y + 1, 0] and labels[y, -1] != labels[y + 1, 0] for y in range(text.shape[0] - 1)), name


def test_page_seams_pages_are_independent():
    heat = bc.page_seams()
    assert heat.shape == (3, 16, 32, 2)
    assert (heat[0, 14:, 6:16, 0] > 0.4).all() and (heat[1, :2, 6:16, 0] > 0.4).all()
    assert (heat[1, 15, :, 0] > 0.4).all() and (heat[2, 0, :, 0] > 0.4).all()
    assert heat[0, 15, 31, 0] > 0.4 and heat[1, 0, 0, 0] > 0.4                      # consecutive pixels of the flattened batch
    per_page = []
    for p in range(3):
        alone = _oracle(heat[p, ..., 0].copy(), heat[p, ..., 1].copy(), 1.0, bc.SETTINGS[0])
        assert alone == _oracle(heat[p, ..., 0], heat[p, ..., 1], 1.0, bc.SETTINGS[0])    # a page of the batch == the same page alone
        per_page.append(alone)
    assert [len(x[0]) for x in per_page] == [2, 3, 2]
    # the fixture bites: read as ONE 48 x 32 map, the components join across both seams (7 -> 5)
    flat = heat.reshape(48, 32, 2)
    assert len(_oracle(flat[..., 0], flat[..., 1], 1.0, bc.SETTINGS[0])[0]) == 5


def test_wrap_blobs_are_where_the_docstring_says():
    """Index arithmetic only (plus two narrow bands of pixels): the 4M-pixel oracle run belongs to the GPU test."""
    H, W = bc.WRAP_H, bc.WRAP_W
    total = 2 * H * W
    assert bc.WRAP_ROUND == 16384 * 256 == 4194304 and total == 4325376 and bc.WRAP_ROUND < total < 2 * bc.WRAP_ROUND
    assert total % 64 == 0                                   # no partial wave at this size: the batch's last wave is a whole one
    first = lambda b: (b[0] * H + b[1]) * W + b[2]                                    # flattened index of a blob's first pixel
    last = lambda b: (b[0] * H + b[1] + b[3] - 1) * W + b[2] + b[4] - 1
    py, px = divmod(bc.WRAP_ROUND - H * W, W)
    assert (py, px) == (1442, 1280)
    through = [b for b in bc.WRAP_BLOBS if b[0] == 1 and b[1] == py and b[2] < px < b[2] + b[4] - 1]
    assert len(through) == 1 and through[0][4] > 64                                   # a horizontal run through the wrap pixel
    crossing = [b for b in bc.WRAP_BLOBS if b[0] == 1 and b[1] < py < b[1] + b[3] - 1 and b[4] <= 2]
    assert len(crossing) == 1 and first(crossing[0]) < bc.WRAP_ROUND < last(crossing[0])
    tail = [b for b in bc.WRAP_BLOBS if last(b) == total - 1]
    assert len(tail) == 1 and tail[0][4] == 64 and (tail[0][0], tail[0][1] + tail[0][3]) == (1, H)
    assert sum(last(b) < bc.WRAP_ROUND for b in bc.WRAP_BLOBS) >= 4 and sum(first(b) > bc.WRAP_ROUND for b in bc.WRAP_BLOBS) >= 2
    # blobs lie inside their page, hold at least 10 pixels, and no two touch (so: one component per blob, none across the page border)
    for i, a in enumerate(bc.WRAP_BLOBS):
        assert 0 <= a[1] and a[1] + a[3] <= H and 0 <= a[2] and a[2] + a[4] <= W and a[3] * a[4] >= 10 and a[5] >= 0.9
        for b in bc.WRAP_BLOBS[i + 1:]:
            if a[0] == b[0]:
                assert a[1] + a[3] < b[1] or b[1] + b[3] < a[1] or a[2] + a[4] < b[2] or b[2] + b[4] < a[2], (a, b)
    band = bc.wrap_rows(1, 1440, 1445)
    assert band.shape == (5, W, 2) and band[2, px, 0] == np.float32(0.9) and band[2, 1249, 0] == 0 and band[2, 1331, 0] == 0
    assert not band[1, 1240:1340, 0].any() and band[0, 1290, 0] == np.float32(0.9) and band[..., 1].max() == 0
    assert (band[:, 600:602, 0] == 1.0).all()
    band = bc.wrap_rows(1, H - 4, H)
    assert (band[:, W - 64:, 0] == np.float32(0.9)).all() and not band[:, :W - 64, 0].any()
    assert not bc.wrap_rows(0, 1440, 1445).any()
