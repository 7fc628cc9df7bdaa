"""The case table of tests/test_gpu_preproc_routes.py: one row per call of bbocr_op_preprocess_stage, with the offsets of the source and
destination planes inside their buffers (so the low two pointer bits are chosen, not inherited from the allocator) and the kernel route
every launcher behind the stage must take.  Importable without torch: tests/test_preproc_routes_cpu.py checks the rows against the host
route functions (bbocr_host_pp_*_route) and that together they reach every member of the route enum.

Route keys of a row: "resize", "gauss", "clahe_hist", "clahe_apply", "unsharp" name the function of that stage; behind UNSHARP_PASSES_* the
six box passes run through scratch planes (aligned): "box_first" is the pass that reads the stage's source, "box_rest" the other five.
"resize_dword_rows" (1 / 0, no enum member): whether the tiled resize kernels are told to store their full tiles as whole dwords
(bbocr_host_pp_resize_dword_rows).
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "stage H W dh dw param so do routes")


def _c(stage, H, W, param, routes, so=0, do=0, dh=None, dw=None):
    return Case(stage, H, W, dh or H, dw or W, float(param), so, do, dict(routes))


FUSED = {"unsharp": "UNSHARP_FUSED"}
UNSHARP_PARAMS = ((5, 1.0), (7, 20), (7, 150))           # stage 5: radius, stage 7: percent (radius 1); both box radius 0
UNSHARP_H = (1, 2, 3, 4, 15, 16, 17, 18, 19, 20, 33)     # 1..3: top and bottom fix-ups on one strip; 15..19: `bottom` flips between strips 0 and 1


def _passes(so, do, W, r):
    """the rows' expectation for a plane the fused route refuses (derived by reading launch_pp_box_pass and launch_pp_unsharp)"""
    x4 = r == 0 and W % 4 == 0
    return {"unsharp": "UNSHARP_PASSES_BYTE" if (so | do) & 3 else "UNSHARP_PASSES_VEC",
            "box_first": "BOX0_X4" if x4 and so & 3 == 0 else "BOX_BYTE", "box_rest": "BOX0_X4" if x4 else "BOX_BYTE"}


GROUPS = {}
for _stage, _param in UNSHARP_PARAMS:
    _tag = f"s{_stage}_{_param:g}"
    # W = 4: one thread is both `first` and `last` of its row
    GROUPS[f"unsharp_fused_{_tag}"] = [_c(_stage, H, W, _param, FUSED) for H in UNSHARP_H for W in (4, 8, 12)]
    GROUPS[f"unsharp_misaligned_{_tag}"] = [_c(_stage, H, 8, _param, _passes(so, do, 8, 0), so=so, do=do)
                                            for H in UNSHARP_H for so, do in ((1, 0), (0, 2), (3, 3))]
    GROUPS[f"unsharp_wide_and_tail_{_tag}"] = (
        [_c(_stage, H, 1028, _param, FUSED) for H in (1, 17)]                                         # a second blockIdx.x
        # W % 4 != 0, aligned: byte box passes, then the dword combine with a tail of total & 3 = 1 or 3 pixels ...
        + [_c(_stage, H, W, _param, _passes(0, 0, W, 0)) for W in (1, 5, 9) for H in (1, 3, 17)]
        # ... and of 2 (no product of the sizes above leaves 2), and the byte-wise combine on the same planes
        + [_c(_stage, H, W, _param, _passes(0, 0, W, 0)) for H, W in ((2, 1), (2, 5))]
        + [_c(_stage, H, W, _param, _passes(1, 0, W, 0), so=1) for H, W in ((1, 1), (2, 5), (17, 9))])
# stage 5 with radius 2: box radius 1, the general box pass on every plane
GROUPS["unsharp_radius2"] = [_c(5, H, W, 2.0, _passes(so, 0, W, 1), so=so) for H, W in ((3, 4), (17, 8), (5, 9)) for so in (0, 1)]

GAUSS_SHAPES = ((1, 8), (2, 8), (1, 1), (1, 2), (2, 1), (3, 4), (5, 12), (17, 1028))
for _sigma in (3.0, 5.0):
    GROUPS[f"gauss_{_sigma:g}"] = (
        # W = 4 stays on the byte kernel: the x4 kernel's reflected neighbours need W >= 8
        [_c(1, H, W, _sigma, {"gauss": "GAUSS_X4" if W % 4 == 0 and W >= 8 else "GAUSS_BYTE"}) for H, W in GAUSS_SHAPES]
        + [_c(1, 5, 12, _sigma, {"gauss": "GAUSS_BYTE"}, so=2)])
# stage 2: the pixel sum through both kernels (the blur kernel with identity taps writes a scratch plane), then the byte lookup
GROUPS["contrast"] = [_c(2, 5, 12, 1.9, {"gauss": "GAUSS_X4"}), _c(2, 5, 12, 1.9, {"gauss": "GAUSS_BYTE"}, so=1),
                      _c(2, 1, 1, 1.9, {"gauss": "GAUSS_BYTE"}), _c(2, 1, 1, 1.9, {"gauss": "GAUSS_BYTE"}, so=1)]

CLAHE_SHAPES = (
    # H, W, apply route of the aligned plane
    (8, 8, "APPLY_VEC"),            # tiles of 1 x 1
    (9, 12, "APPLY_VEC"),           # both axes padded to 16: tiles 6 and 7 lie wholly in the reflected padding, tile width 2
    (12, 9, "APPLY_BYTE"),
    (16, 8, "APPLY_VEC"),           # tile width 1
    (15, 15, "APPLY_BYTE"),
    (128, 128, "APPLY_CELL_2"),     # exactly 1 << 14 pixels
    (127, 132, "APPLY_CELL_2"),
    (64, 260, "APPLY_CELL_2"),      # H divides the grid and is padded by a whole 8 rows because W does not
    (128, 124, "APPLY_VEC"),        # one dword column below 1 << 14
    (512, 32, "APPLY_CELL_8"),      # tile height 64, exactly 1 << 14 pixels
    (511, 36, "APPLY_CELL_8"),      # padded to 512 rows: tile height still 64
    (503, 36, "APPLY_CELL_2"),      # padded to 504 rows: tile height 63, the last below the 8-chunk threshold
    (4096, 8, "APPLY_CELL_32"),     # tile height 512, tile width 1
    (4097, 12, "APPLY_CELL_32"),    # padded: tile height 513, tile width 2
)
for _clip in (2.5, 40.0):
    GROUPS[f"clahe_{_clip:g}"] = (
        [_c(4, H, W, _clip, {"clahe_hist": "HIST_X4" if W % 4 == 0 else "HIST_BYTE", "clahe_apply": a}) for H, W, a in CLAHE_SHAPES]
        # the byte kernels on W % 4 == 0 planes
        + [_c(4, H, W, _clip, {"clahe_hist": "HIST_BYTE", "clahe_apply": "APPLY_BYTE"}, so=1) for H, W in ((128, 128), (9, 12))]
        + [_c(4, H, W, _clip, {"clahe_hist": "HIST_X4", "clahe_apply": "APPLY_BYTE"}, do=1) for H, W in ((128, 128), (9, 12))])
# smaller than the reflected padding of the 8 x 8 grid: BBOCR_ERR_ARG.  (4097, 8): H does not divide the grid, so W = 8 is padded by a whole
# 8 columns as well, as many as it has
CLAHE_REFUSED = ((4, 4), (7, 3), (3, 40), (4097, 8))

# (40, 40) -> n x n: the per-pixel kernel up to 20 (a tile's source window exceeds 128 columns), 16-row tiles from 21 (ceil(64 * 40 / 21) + 5 =
# 127), 32-row tiles from 42 (ceil(32 * 40 / 42) + 5 = 36 window rows)
RESIZE_BOUNDARIES = ((20, "RESIZE_PIXEL"), (21, "RESIZE_TILED16"), (41, "RESIZE_TILED16"), (42, "RESIZE_TILED32"))


def _rs(H, W, dh, dw, route, do=0):
    """a resize row; "resize_dword_rows": whether the tiled kernels store their full tiles as whole dwords (1) or byte-wise (0)"""
    routes = {"resize": route}
    if route != "RESIZE_PIXEL":
        routes["resize_dword_rows"] = int(dw % 4 == 0 and do % 4 == 0)
    return _c(0, H, W, 0, routes, do=do, dh=dh, dw=dw)


GROUPS["resize"] = [
    _rs(1, 1, 1, 1, "RESIZE_TILED16"),
    _rs(1, 4, 2, 6, "RESIZE_TILED32"),
    _rs(2, 2, 3, 3, "RESIZE_TILED32"),
    _rs(5, 7, 64, 64, "RESIZE_TILED32"),             # dw == 64: the tile leaves as whole dwords
    _rs(5, 7, 64, 64, "RESIZE_TILED32", do=1),       # ... which a misaligned destination refuses
    _rs(5, 7, 64, 68, "RESIZE_TILED32"),             # a full tile (dwords) and a ragged one (bytes)
    _rs(3, 300, 4, 450, "RESIZE_TILED32"),
    _rs(40, 40, 12, 12, "RESIZE_PIXEL"),
    _rs(40, 40, 28, 28, "RESIZE_TILED16"),
    _rs(8, 8, 8, 8, "RESIZE_TILED16"),               # scale 1: 32 rows + 5 exceed the 36-row window
] + [_rs(40, 40, n, n, r) for n, r in RESIZE_BOUNDARIES]

# byte kernels, pinned as such: brightness lookup and BGR2GRAY at odd pointers
GROUPS["lut_and_gray"] = [_c(3, 5, 9, 1.2, {}, so=1, do=1), _c(6, 5, 9, 0, {}, so=1, do=1)]

ALL_CASES = [c for g in GROUPS.values() for c in g]
UNSHARP_CASES = [c for c in ALL_CASES if c.stage in (5, 7)]


def unsharp_args(c):
    """(radius, percent) of an unsharp row"""
    return (c.param, 30) if c.stage == 5 else (1.0, int(c.param))


def routes_reported(lib, ids, c, src_bits=None, dst_bits=None):
    """what the host route functions say for the row's shape at these pointer bits (default: the row's offsets in 4-byte aligned buffers)"""
    sb = c.so & 3 if src_bits is None else src_bits
    db = c.do & 3 if dst_bits is None else dst_bits
    out, flags = {}, {}
    if c.stage == 0:
        out["resize"] = lib.bbocr_host_pp_resize_route(c.H, c.W, c.dh, c.dw)
        if ids[out["resize"]] != "RESIZE_PIXEL":
            flags["resize_dword_rows"] = lib.bbocr_host_pp_resize_dword_rows(c.dw, db)
    elif c.stage == 1:
        out["gauss"] = lib.bbocr_host_pp_gauss_route(c.H, c.W, sb, db)
    elif c.stage == 2:
        out["gauss"] = lib.bbocr_host_pp_gauss_route(c.H, c.W, sb, 0)
    elif c.stage == 4:
        out["clahe_hist"] = lib.bbocr_host_pp_clahe_hist_route(c.H, c.W, sb)
        out["clahe_apply"] = lib.bbocr_host_pp_clahe_apply_route(c.H, c.W, sb, db)
    elif c.stage in (5, 7):
        radius, _ = unsharp_args(c)
        out["unsharp"] = lib.bbocr_host_pp_unsharp_route(c.H, c.W, radius, sb, db)
        if ids[out["unsharp"]] != "UNSHARP_FUSED":
            r = lib.bbocr_host_pp_unsharp_box_radius(radius)
            out["box_first"] = lib.bbocr_host_pp_box_route(c.H, c.W, r, sb, 0)
            out["box_rest"] = lib.bbocr_host_pp_box_route(c.H, c.W, r, 0, 0)
    assert all(0 <= v < len(ids) for v in out.values()), (c, out)
    return {**{k: ids[v] for k, v in out.items()}, **flags}


def planes(c, seed=0):
    """the two source planes of a row: uniform noise, and zeros with 255 at the four corners, at the middle of each edge and along rows and
    columns 15, 16, 17 where they exist -- an impulse next to an edge shows every level's edge replication, the lines sit on the seam of
    the 16-row strips"""
    shape = (c.H, c.W, 3) if c.stage == 6 else (c.H, c.W)
    rng = np.random.default_rng([seed, c.stage, c.H, c.W, c.dh, c.dw])
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    d = np.zeros(shape, dtype=np.uint8)
    for y in (0, c.H // 2, c.H - 1):
        for x in (0, c.W // 2, c.W - 1):
            if (y in (0, c.H - 1)) or (x in (0, c.W - 1)):
                d[y, x] = 255
    for k in (15, 16, 17):
        if k < c.H:
            d[k] = 255
        if k < c.W:
            d[:, k] = 255
    return {"noise": noise, "designed": d}


def reference(c, a):
    """oracle/preprocess.py on plane `a` for the row's stage"""
    from oracle import preprocess as pp

    if c.stage == 0:
        return pp.resize_cubic_u8(a, c.dw, c.dh)
    if c.stage == 1:
        return pp.gaussian_blur3_u8(a, c.param)
    if c.stage == 2:
        return pp.pil_contrast_L(a, c.param)
    if c.stage == 3:
        return pp.pil_brightness_L(a, c.param)
    if c.stage == 4:
        return pp.clahe_u8(a, c.param, (8, 8))
    if c.stage == 6:
        return pp.bgr2gray(a)
    radius, percent = unsharp_args(c)
    return pp.pil_unsharp_L(a, radius, percent, 3)
