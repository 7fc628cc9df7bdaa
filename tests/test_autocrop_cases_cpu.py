"""CPU: the designed masks of tests/autocrop_cases.py have the structure they were designed for, on the reference alone
(tests/autocrop_ref.py), and each of a few planted defects of that reference changes what a named case expects -- so a device kernel
with the same defect cannot pass tests/test_gpu_autocrop.py."""
import numpy as np
import pytest
from scipy import ndimage

import autocrop_cases as cases
import autocrop_ref as ref

S8 = np.ones((3, 3), bool)
S4 = ndimage.generate_binary_structure(2, 1)


@pytest.fixture(scope="module")
def exp():
    return cases.expected()


def _n8(m):
    return ndimage.label(m, structure=S8)[1]


def _family(exp, prefix):
    got = {n: e for n, e in exp.items() if n.startswith(prefix)}
    assert got, prefix
    return got


def test_case_set_is_small_and_named_once(exp):
    assert set(exp) == set(cases.all_cases())
    assert 250 <= len(exp) <= 400 and max(e.mask.size for e in exp.values()) == 8 * 8230
    assert all(e.mask.dtype == bool and e.mask.ndim == 2 for e in exp.values())
    shapes = {e.mask.shape for e in exp.values()}
    assert set(cases.SHAPES) <= shapes and len(cases.SHAPES) == 62
    ww = lambda w: (w + 31) // 32
    assert {ww(w) for _, w in cases.SHAPES} >= {1, 2, 3, 4, 9, 258} and ww(cases.LONG_ROW[1]) > 256 and cases.TALL[0] > 4096
    assert {w % 32 for _, w in cases.SHAPES} >= {0, 1, 7, 31}


def test_fills(exp):
    fam = _family(exp, "fills/")
    assert len(fam) == 3 * len(cases.SHAPES) - 1
    for name, e in fam.items():
        H, W = e.mask.shape
        if name.endswith("/empty"):
            assert not e.mask.any() and not e.merged.any() and e.external[1] == [] and e.components[1] == []
            continue
        # the closing fills the hole, and the border never takes part in the erosion: the plane stays full down to 1 x 1
        assert e.mask.sum() == H * W - name.endswith("/minus_one")
        assert e.merged.all() and e.external[1] == [(0, 0, W, H)] and e.external[0].all()
        assert np.array_equal(e.components[0], e.mask)
        if name.endswith("/full") or min(H, W) > 2:
            assert e.components[1] == [(0, 0, W, H)]


def test_blocks(exp):
    fam = _family(exp, "blocks/")
    survivors_2x2 = {"tl": 21, "tr": 21, "bl": 21, "br": 21, "near01": 24, "near11": 32, "near22": 45}
    seen = set()
    for name, e in fam.items():
        _, shape, what = name.split("/")
        size, site = what.split("@")
        H, W = e.mask.shape
        ys, xs = np.nonzero(e.mask)
        s = int(size[0])
        assert e.mask.sum() == s * s and ys.max() - ys.min() == s - 1 and xs.max() - xs.min() == s - 1
        assert e.components[1] == [(int(xs.min()), int(ys.min()), s, s)]
        seen.add((site, int(xs.min()) // 32 != int(xs.max()) // 32, int(xs.max()) == W - 1, int(ys.min()) == 0, int(ys.max()) == H - 1))
        if s == 3:                                        # a lone block survives from 3x3 up, wherever it lies
            assert _n8(e.merged) == 1 and e.merged[e.mask].all() and len(e.external[1]) == 1, name
        elif shape in ("40x97", "12x65"):                 # 2x2: only where the border, which never erodes, stands in for the missing pixels
            assert int(e.merged.sum()) == survivors_2x2.get(site, 0), name
    assert {t[0] for t in seen if t[1]} >= {"bit31", "bit30", "right"}          # blocks astride a word boundary (W = 65, 97: the last word holds one bit)
    assert any(t[2] for t in seen) and any(t[3] for t in seen) and any(t[4] for t in seen)


def test_random_masks_are_not_trivial(exp):
    fam = _family(exp, "random/")
    assert len(fam) == 6 and {e.mask.shape for e in fam.values()} >= {cases.LONG_ROW, cases.TALL}
    for name, e in fam.items():
        d = float(e.merged.mean())
        print(f"{name}: merged density {d:.3f}, {_n8(e.merged)} merged components, {len(e.components[1])} raw components")
        assert 0.05 < d < 0.95, (name, d)                # the condition on RANDOM_SEED / RANDOM_P: the reference alone decides it
        assert e.mask.any()
    assert sum(len(e.external[1]) > 1 for e in fam.values()) >= 4


def test_sweeps_cross_the_join(exp):
    for prefix, join, gaps in (("hsweep/in_word/", cases.H_JOIN, cases.H_GAPS), ("hsweep/across_words/", cases.H_JOIN, cases.H_GAPS),
                               ("vsweep/top/", cases.V_JOIN, cases.V_GAPS), ("vsweep/bottom/", cases.V_JOIN, cases.V_GAPS)):
        fam = _family(exp, prefix)
        assert len(fam) == len(gaps) and min(gaps) < join < max(gaps) - 1
        for gap in gaps:
            e = fam[f"{prefix}gap{gap}"]
            assert _n8(e.mask) == 2 and len(e.components[1]) == 2
            assert _n8(e.merged) == len(e.external[1]) == (1 if gap <= join else 2), (prefix, gap)
    # where the gaps lie: inside word 1 / across words 1 | 2; rows 1 .. and .. H - 2
    for where, x0 in cases.H_SWEEP_X0.items():
        lo, hi = x0 + 3, x0 + 2 + max(cases.H_GAPS)
        assert (lo // 32 == hi // 32) == (where == "in_word")
    H = cases.V_SWEEP_SHAPE[0]
    assert all(np.nonzero(e.mask)[0].min() == 1 for n, e in exp.items() if n.startswith("vsweep/top/"))
    assert all(np.nonzero(e.mask)[0].max() == H - 2 for n, e in exp.items() if n.startswith("vsweep/bottom/"))


def test_diagonal_contacts(exp):
    fam = _family(exp, "diag/")
    assert len(fam) == 14
    W = cases.DIAG_SHAPE[1]
    for name, e in fam.items():
        ys, xs = np.nonzero(e.mask)
        # joined by one corner contact only, but for left_ul: there the left neighbour already joins the two rows
        assert _n8(e.mask) == 1 and ndimage.label(e.mask, structure=S4)[1] == (1 if name.endswith("left_ul") else 2), name
        assert e.components[1] == [(int(xs.min()), 1, int(np.ptp(xs)) + 1, 2)] and np.array_equal(e.components[0], e.mask)
        lower = int(xs[ys == 2].max())                   # the pixel that has to find its diagonal neighbour above
        if name.endswith("left_ur"):
            assert e.mask[2, lower - 1] and not e.mask[1, lower] and e.mask[1, lower + 1] and not e.mask[1, lower - 1]
        if name.endswith("left_ul"):
            assert e.mask[2, lower - 1] and not e.mask[1, lower] and e.mask[1, lower - 1]
    col = lambda n: sorted(set(np.nonzero(fam[n].mask)[1].tolist()))
    assert col("diag/word/backslash") == col("diag/word/slash") == [31, 32]
    assert col("diag/last/backslash") == col("diag/last/slash") == [W - 2, W - 1]
    assert col("diag/word/left_ur") == [30, 31, 32] and col("diag/word+1/left_ur") == [31, 32, 33] and col("diag/last/left_ur")[-1] == W - 1


def test_enclosure_cases(exp):
    closed, leak = exp["diamond/closed"], exp["diamond/leak"]
    assert ndimage.label(closed.mask, structure=S4)[1] == 25                 # the outline is closed by diagonal steps only
    assert _n8(closed.mask) == 2 and closed.components[1] == [(1, 1, 13, 13)] and not closed.components[0][7, 7]
    assert (closed.mask ^ leak.mask).sum() == 1 and _n8(leak.mask) == 2
    assert sorted(leak.components[1]) == [(1, 1, 13, 13), (7, 7, 1, 1)]      # one 4-connected leak: the inside is outer background
    rings = exp["rings/nested3"]
    assert _n8(rings.mask) == 4 and rings.components[1] == [(1, 1, 35, 19)] and rings.components[0].sum() == 2 * (35 + 19) - 4
    for side in ("top", "bottom", "left", "right"):
        e = exp[f"u/{side}"]
        H, W = e.mask.shape
        edge = np.zeros_like(e.mask)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        blab, nb = ndimage.label(~e.mask, structure=S4)
        assert nb == 2 and all((edge & (blab == k)).any() for k in (1, 2))   # the mouth is outer background of its own
        lab, nf = ndimage.label(e.mask, structure=S8)
        assert nf == 2 and len(e.components[1]) == 2 and e.components[0][e.mask].all()
        blob = [k for k in (1, 2) if not (edge & (lab == k)).any()]
        assert len(blob) == 1 and (lab == blob[0]).sum() == 4                # external without touching the edge
    for c in ("tl", "tr", "bl", "br"):
        e = exp[f"corner/{c}"]
        H, W = e.mask.shape
        edge = np.zeros_like(e.mask)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        ys, xs = np.nonzero(e.mask & edge)
        assert len(ys) == 1 and ys[0] in (0, H - 1) and xs[0] in (0, W - 1)
        assert _n8(e.mask) == 1 and ndimage.label(e.mask, structure=S4)[1] == 2 and len(e.components[1]) == 1
        assert e.components[1][0][2:] == (4, 4)


def test_chain_and_count_cases(exp):
    sp = exp["chain/spiral"]
    assert ndimage.label(sp.mask, structure=S4)[1] == 1 and sp.mask.sum() > 500 and sp.components[1] == [(0, 0, 33, 33)]
    nb = ndimage.convolve(sp.mask.astype(int), S4.astype(int), mode="constant")[sp.mask] - 1
    assert (nb <= 2).all() and (nb == 1).sum() == 2                          # a chain: two ends, no branch
    comb = exp["chain/comb"]
    assert _n8(comb.mask) == 2 and sorted(comb.components[1]) == [(0, 0, 65, 31), (0, 9, 65, 31)]
    cb = exp["checkerboard/12x33"]
    assert _n8(cb.mask) == 1 and ndimage.label(~cb.mask, structure=S4)[1] == (~cb.mask).sum() and cb.components[1] == [(0, 0, 33, 12)]
    lat = exp["lattice/11x33"]
    H, W = lat.mask.shape
    most = ((H + 1) // 2) * ((W + 1) // 2)                                   # no mask holds more 8-connected components
    assert _n8(lat.mask) == most == len(lat.components[1]) == lat.mask.sum() and all(b[2:] == (1, 1) for b in lat.components[1])
    ar = exp["area/extremes"]
    area = ar.mask.size
    assert _n8(ar.mask) == 3 and sorted(ar.components[1]) == [(20, 20, 200, 200), (250, 240, 1, 1)]
    assert 5 * 1 < 0.0001 * area and 200 * 200 > 5 * 0.10 * area             # far outside the 0.01 % .. 10 % window of the page path
    assert ref.crop_box(ar.components[1], *ar.mask.shape)[1] == []


@pytest.mark.parametrize("shape", cases.BAR_PAGES)
def test_bar_pages_have_structure(shape):
    st = ref.stages(cases.bar_page(shape))
    print(f"{shape}: composite {st['composite'].mean():.3f}, merged {st['merged'].mean():.3f}, {len(st['boxes'])} external components")
    assert shape[1] % 32 and len(st["boxes"]) >= 3 and 0.02 < st["merged"].mean() < 0.6
    box, kept = ref.crop_box(st["boxes"], *shape, margin=8)
    assert box is not None and len(kept) >= 3


# ---- planted defects of the reference: each must change what a named case expects

def _merged(m, erode):
    def variant(kw, kh):
        cw, ch = (kw - 1) * 2 + 1, (kh - 1) * 2 + 1
        return ref.dilate(ref.dilate(erode(erode(ref.dilate(m, cw, ch), cw, ch), 3, 3), 3, 3), 11, 3)

    return variant(9, 3) | variant(15, 5)


def _erode_border_takes_part(m, kw, kh):
    return ndimage.minimum_filter(m.view(np.uint8), size=(kh, kw), mode="constant", cval=0).astype(bool)


def _merged_without_tail_mask(m):
    """the rows as whole 32-bit words whose padding bits are pixels like any other"""
    H, W = m.shape
    wide = np.zeros((H, (W + 31) // 32 * 32), bool)
    wide[:, :W] = m
    return ref.merged_mask(wide)[:, :W]


def _labels(fg, skip_diagonals_beside_left=False):
    """union-find in the order of ac_ccl_merge_kernel: left, above, and the two diagonals above when the pixel above is not set"""
    H, W = fg.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    def union(a, b):
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)

    for y, x in zip(*np.nonzero(fg)):
        i = y * W + x
        wl = x > 0 and fg[y, x - 1]
        if wl:
            union(i, i - 1)
        if y > 0 and fg[y - 1, x]:
            union(i, i - W)
        elif y > 0 and not (skip_diagonals_beside_left and wl):
            if x > 0 and fg[y - 1, x - 1]:
                union(i, i - W - 1)
            if x + 1 < W and fg[y - 1, x + 1]:
                union(i, i - W + 1)
    lab = np.zeros((H, W), np.int64)
    roots = {}
    for y, x in zip(*np.nonzero(fg)):
        lab[y, x] = roots.setdefault(find(y * W + x), len(roots) + 1)
    return lab


def _external(fg, lab=None, bg=S4, edge_only=False):
    """autocrop_ref.external_components with its three rules open to change"""
    lab = ndimage.label(fg, structure=S8)[0] if lab is None else lab
    blab, _ = ndimage.label(~fg, structure=bg)
    edge = np.zeros_like(fg)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    outer_ids = np.unique(blab[edge & ~fg])
    outer = np.isin(blab, outer_ids[outer_ids > 0]) & (not edge_only)
    near = np.zeros_like(fg)
    near[:, 1:] |= outer[:, :-1]
    near[:, :-1] |= outer[:, 1:]
    near[1:, :] |= outer[:-1, :]
    near[:-1, :] |= outer[1:, :]
    ext_ids = np.unique(lab[fg & (edge | near)])
    ext_ids = ext_ids[ext_ids > 0]
    objs = ndimage.find_objects(lab)
    boxes = [(int(sx.start), int(sy.start), int(sx.stop - sx.start), int(sy.stop - sy.start)) for sy, sx in (objs[i - 1] for i in ext_ids)]
    return np.isin(lab, ext_ids), boxes


DEFECTS = {
    # name: (cases whose expectation it must change, mask -> what the defective reference gives, Expected -> what the reference gives)
    "erosion whose border takes part": (["fills/5x33/full", "fills/1x1/full", "blocks/40x97/2x2@tl"],
                                        lambda m: _merged(m, _erode_border_takes_part), lambda e: e.merged),
    "no tail mask": (["blocks/12x65/2x2@tr", "fills/5x1/full", "random/40x97/p0.01"], _merged_without_tail_mask, lambda e: e.merged),
    "4-connected foreground": (["diamond/closed", "diag/word/backslash", "diag/last/slash", "checkerboard/12x33"],
                               lambda m: sorted(_external(m, ndimage.label(m, structure=S4)[0])[1]), lambda e: sorted(e.components[1])),
    "8-connected background": (["diamond/closed"], lambda m: sorted(_external(m, bg=S8)[1]), lambda e: sorted(e.components[1])),
    "external = touches the edge only": (["u/top", "u/left", "lattice/11x33", "area/extremes"],
                                         lambda m: sorted(_external(m, edge_only=True)[1]), lambda e: sorted(e.components[1])),
    "diagonal links skipped beside a set left neighbour": (["diag/word/left_ur", "diag/word+1/left_ur", "diag/last/left_ur"],
                                                           lambda m: sorted(_external(m, _labels(m, True))[1]),
                                                           lambda e: sorted(e.components[1])),
}


def test_defect_models_equal_the_reference_when_switched_off(exp):
    for name in ("random/40x97/p0.01", "blocks/12x65/2x2@tr", "diamond/closed", "u/top", "chain/comb", "diag/word/left_ur", "lattice/11x33"):
        e = exp[name]
        assert np.array_equal(_merged(e.mask, ref.erode), e.merged)
        for lab in (None, _labels(e.mask)):
            mask, boxes = _external(e.mask, lab)
            assert np.array_equal(mask, e.components[0]) and sorted(boxes) == sorted(e.components[1])
    e = exp["fills/11x64/full"]                           # whole words: nothing for a tail mask to do
    assert np.array_equal(_merged_without_tail_mask(e.mask), e.merged)


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_caught_by_a_named_case(exp, defect):
    names, broken, good = DEFECTS[defect]
    for name in names:
        e = exp[name]
        got, want = broken(e.mask), good(e)
        assert not np.array_equal(got, want), f"{defect}: {name} would pass"
    caught = sum(not np.array_equal(broken(e.mask), good(e)) for e in exp.values() if e.mask.size <= 4096)
    print(f"{defect}: changes {caught} of the small cases, among them {names}")


def test_specific_defect_outcomes(exp):
    e = exp["diamond/closed"]
    assert len(_external(e.mask, ndimage.label(e.mask, structure=S4)[0])[1]) == 24       # every outline pixel its own box
    assert sorted(_external(e.mask, bg=S8)[1]) == [(1, 1, 13, 13), (7, 7, 1, 1)]
    assert _external(exp["u/top"].mask, edge_only=True)[1] == [(10, 0, 11, 9)]
