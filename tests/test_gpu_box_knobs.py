"""-m gpu: the box stage off its defaults -- every (text_threshold, low_text, link_threshold) of tests/box_cases.py on maps designed
around the comparisons of csrc/ccl.hip, maps 16 and 48 pixels wide, components at page seams, a batch longer than one grid round of
the CCL kernels -- and the detector / the whole pipeline at mag_ratio 1.5 and 0.6.  Boxes are compared for equality, in order:
polygons and horizontal boxes as int lists, free boxes to 1e-9 (as test_gpu_pipeline.py::test_boxes_bit_exact_given_heatmap does)."""
import numpy as np
import pytest
import torch

import box_cases as bc
from test_gpu_pipeline import HEAT_TOL
from test_gpu_precision import _same_boxes

pytestmark = pytest.mark.gpu

RATIOS = (1.0, 1.5)
_ORACLE = {}


def _want(key, text, link, ratio, **kw):
    """The oracle's (polys, horizontal, free) for one map, computed once per (map, ratio, settings) and never modified."""
    from oracle import boxes as obox

    if key not in _ORACLE:
        oh, of, op = obox.detect_from_heatmap(text, link, ratio, **kw)
        _ORACLE[key] = ([list(map(int, p)) for p in op], [list(map(int, b)) for b in oh], [np.array(b, dtype=np.float64) for b in of])
    return _ORACLE[key]


def _assert_page(got, b, want, what):
    hori, free, polys = got
    assert polys[b] == want[0], what
    assert hori[b] == want[1], what
    assert len(free[b]) == len(want[2]), what
    for g, w in zip(free[b], want[2]):
        assert np.allclose(np.array(g, dtype=np.float64), w, rtol=0, atol=1e-9), what


def _dev(pages):
    """[(text, link)] of one shape -> float32 [B, h, w, 2] on the device."""
    return torch.from_numpy(np.stack([np.stack([t, l], -1) for t, l in pages])).cuda()


def test_designed_maps_at_every_setting(reader):
    maps = bc.designed_maps()
    by_shape = {}
    for name, (text, link) in maps.items():
        by_shape.setdefault(text.shape, []).append(name)
    groups = [names for names in by_shape.values() if len(names) > 1]
    assert len(groups) == 5 and sum(map(len, groups)) == len(maps) == 10         # edges + bridges, and each narrow map with its mirror
    single = {name: _dev([m]) for name, m in maps.items()}
    stacked = [(names, _dev([maps[n] for n in names])) for names in groups]
    n_free = n_polys = 0
    for s in bc.SETTINGS:
        kw = bc.setting_kw(s)
        for ratio in RATIOS:
            want = {name: _want((name, ratio, s), *maps[name], ratio, **kw) for name in maps}
            for name in maps:
                _assert_page(reader.boxes_from_heatmap(single[name], ratio, **kw), 0, want[name], (name, s, ratio))
                n_polys += len(want[name][0])
                n_free += len(want[name][2])
            for names, heat in stacked:                  # the same maps as pages of one batch: per page what the map gave alone
                got = reader.boxes_from_heatmap(heat, ratio, **kw)
                for b, name in enumerate(names):
                    _assert_page(got, b, want[name], (names, b, s, ratio))
    assert n_polys > 500 and n_free > 0


def test_page_seams(reader):
    heat = bc.page_seams()
    for order in ([0, 1, 2], [2, 1, 0]):
        d = torch.from_numpy(np.ascontiguousarray(heat[order])).cuda()
        for s in (bc.SETTINGS[0], bc.SETTINGS[3]):
            got = reader.boxes_from_heatmap(d, 1.0, min_size=0, **bc.setting_kw(s))
            for b, p in enumerate(order):
                want = _want(("seam", p, s), heat[p, ..., 0], heat[p, ..., 1], 1.0, min_size=0, **bc.setting_kw(s))
                _assert_page(got, b, want, (order, b, s))
            assert [len(x) for x in got[2]] == [[2, 3, 2][p] for p in order]


def test_grid_stride_wrap(reader):
    """More pixels than one grid round (16384 blocks of 256): the second round starts inside a horizontal run, below the upper part of a
    vertical stroke, and ends with the batch's last wave (tests/box_cases.py::WRAP_BLOBS).  One oracle run per page."""
    heat = bc.wrap_batch()
    assert heat.shape[0] * heat.shape[1] * heat.shape[2] > bc.WRAP_ROUND
    got = reader.boxes_from_heatmap(torch.from_numpy(heat).cuda(), 1.0)
    for p in range(2):
        want = _want(("wrap", p), heat[p, ..., 0], heat[p, ..., 1], 1.0)
        assert len(want[0]) == sum(b[0] == p for b in bc.WRAP_BLOBS)                  # one polygon per blob
        _assert_page(got, p, want, p)


# ---------------------------------------------------------------------------------------------------- mag_ratio
MAG_PAGE = dict(width=256, height=160, lines=3, margin=12, font_size=28, line_pitch=44)      # chosen with the oracle alone (seed 42)
MAGS = (1.5, 0.6)


@pytest.fixture(scope="module")
def mag_page():
    from bb_ocr_amd import synth

    return synth.page(42, **MAG_PAGE)[0]


@pytest.fixture(scope="module")
def mag_oracle(mag_page, oracle_reader):
    """{mag_ratio: (text map, link map, ratio)} of the page, computed once."""
    return {m: oracle_reader.heatmap(mag_page, mag_ratio=m) for m in MAGS}


def test_mag_ratio_heatmap(reader, mag_page, mag_oracle):
    """The detector's resize kernel ENLARGING a page (mag_ratio 1.5: 160 x 256 -> 240 x 384, ratio 1.5) and shrinking it (0.6) against the
    oracle's cv2-style resize + network: equal ratio and shape, text map within the bound of test_detector_resize_path (measured on an
    MI355X: 0.0156 at 1.5 and 0.0078 at 0.6, of 0.06)."""
    from oracle import boxes as obox

    rgb = torch.from_numpy(mag_page[None]).cuda()
    for m in MAGS:
        st, sl, r2 = mag_oracle[m]
        assert r2 == m and st.max() > 0.7
        oh, of, _ = obox.detect_from_heatmap(st, sl, r2)
        assert len(oh) + len(of) >= 3
        heat, ratio = reader.heatmap_device(rgb, mag_ratio=m)
        assert ratio == r2 and tuple(heat.shape) == (1,) + st.shape + (2,)
        got = heat[0].cpu().numpy()
        e_text, e_link = float(np.abs(got[..., 0] - st).max()), float(np.abs(got[..., 1] - sl).max())
        print(f"mag_ratio {m}: heat map {st.shape}, max |err| text {e_text:.5f} (bound {HEAT_TOL * 2}), link {e_link:.5f}")
        assert e_text <= HEAT_TOL * 2
    assert mag_oracle[1.5][0].shape == (128, 192) and mag_oracle[0.6][0].shape == (48, 80)


def _quads(hori, free, H, W):
    """What the recogniser stage reports for these boxes: horizontal ones clamped to the page as corner lists, then the free ones."""
    out = []
    for b in hori:
        x0, x1, y0, y1 = max(0, b[0]), min(b[1], W), max(0, b[2]), min(b[3], H)
        out.append([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    return out + [list(map(list, f)) for f in free]


def test_mag_ratio_end_to_end(reader, reader_exact, oracle_reader, mag_page):
    """mag_ratio through the whole pipeline: boxes scaled back by ``ratio`` > 1 and < 1 and the crops cut from them (exact mode against the
    oracle), pages of two shapes in one call, and readtext's own thresholds reaching the box stage."""
    from bb_ocr_amd import synth

    H, W = mag_page.shape[:2]
    for m in MAGS:                                       # exact mode against the oracle, as tests/test_gpu_precision.py checks it
        want = oracle_reader.readtext(mag_page, mag_ratio=m)
        got = reader_exact.readtext(mag_page, mag_ratio=m)
        assert len(want) >= 3
        assert _same_boxes(got, want), m
        for (_, tg, cg), (_, tw, cw) in zip(got, want):
            assert tg == tw
            assert abs(cg - float(cw)) <= 1e-3 * max(float(cw), 1e-3)
    # pages of two shapes in one call, enlarged: what each page gives on its own
    other = synth.page(43, width=272, height=176, lines=3, margin=16, font_size=32, line_pitch=48)[0]
    pages = [torch.from_numpy(mag_page).cuda(), torch.from_numpy(other).cuda()]
    alone = [reader.readtext_device(p[None], mag_ratio=1.5)[0] for p in pages]
    assert reader.readtext_pages(pages, mag_ratio=1.5) == alone
    assert all(len(a) >= 3 for a in alone)
    assert [reader.readtext_device(p[None])[0] for p in pages] != alone                     # mag_ratio is not a no-op on these pages
    # every page is checked under the call's mag_ratio before anything is queued, and the message names the page
    with pytest.raises(RuntimeError, match="page 1: page collapses"):
        reader.readtext_pages([pages[0], torch.zeros((2, 2, 3), dtype=torch.uint8, device="cuda")], mag_ratio=0.3)
    assert reader.readtext_pages(pages, mag_ratio=1.5) == alone
    # thresholds given to readtext reach the box stage: the boxes are those of boxes_from_heatmap on the call's own heat map
    kw = dict(text_threshold=0.5, link_threshold=0.2, mag_ratio=0.6)
    heat, ratio = reader.heatmap_device(pages[0][None], **kw)
    hori, free, _ = reader.boxes_from_heatmap(heat, ratio, **kw)
    got = reader.readtext(mag_page, **kw)
    want = _quads(hori[0], free[0], H, W)
    assert len(got) == len(want) >= 3
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g[0], dtype=np.float64), np.asarray(w, dtype=np.float64))
    dh, df, _ = reader.boxes_from_heatmap(heat, ratio, mag_ratio=0.6)
    assert (dh, df) != (hori, free)                      # ... and on this heat map the two thresholds change the boxes
