"""Designed masks for the auto-crop's rect morphology and component kernels (csrc/autocrop.hip), pure numpy.  Every family returns
``{name: bool mask}``; what a mask must give comes from ``autocrop_ref.merged_mask`` / ``autocrop_ref.external_components``, which take
any mask.  tests/test_autocrop_cases_cpu.py pins each family's structure on that reference; tests/test_gpu_autocrop.py runs every mask
through ``bbocr_op_autocrop_mask_stage``.

What the shapes are for (WW = packed 32-bit words per row): widths 1 .. 31 have WW = 1 and a partial word, 32 and 64 have none, 33, 65, 97
and 257 leave one valid bit in the last word and 63 leaves 31; 8 x 8230 has WW = 258, a second x-block of the word kernels; 4100 x 8 goes
past the 4096 rows of the y grid."""
import numpy as np

WIDTHS = (1, 7, 31, 32, 33, 63, 64, 65, 97, 257)
HEIGHTS = (1, 2, 5, 11, 12, 40)
LONG_ROW, TALL = (8, 8230), (4100, 8)
SHAPES = [(h, w) for h in HEIGHTS for w in WIDTHS] + [LONG_ROW, TALL]

# two 3x3 blocks join through the 29 x 9 closing (radii 14, 4): up to 28 empty columns / 8 empty rows between them
H_JOIN, V_JOIN = 28, 8
H_GAPS, V_GAPS = range(H_JOIN - 2, H_JOIN + 4), range(V_JOIN - 2, V_JOIN + 4)


def _tag(shape):
    return f"{shape[0]}x{shape[1]}"


def _block(shape, y, x, s):
    m = np.zeros(shape, bool)
    m[y:y + s, x:x + s] = True
    return m


def fills():
    """empty, full, and full minus the last valid bit of the middle row, on every shape (1 x 1 minus one is the empty mask again)"""
    out = {}
    for shape in SHAPES:
        out[f"fills/{_tag(shape)}/empty"] = np.zeros(shape, bool)
        out[f"fills/{_tag(shape)}/full"] = np.ones(shape, bool)
        if shape == (1, 1):
            continue
        m = np.ones(shape, bool)
        m[shape[0] // 2, shape[1] - 1] = False
        out[f"fills/{_tag(shape)}/minus_one"] = m
    return out


BLOCK_SHAPES = ((40, 97), (12, 65), (11, 63))
NEAR_CORNER = ((0, 0), (0, 1), (1, 1), (2, 2))                  # (y, x): where a 2x2 block survives because the border never erodes


def block_sites(shape, s):
    """{site: (y, x)} of one s x s block: the corners, the middle of each edge, one step off the right edge, astride bit 31 | 0 of the
    first two words, and near the top-left corner"""
    H, W = shape
    my, mx = (H - s) // 2, 44
    sites = {"tl": (0, 0), "tr": (0, W - s), "bl": (H - s, 0), "br": (H - s, W - s), "top": (0, mx), "bottom": (H - s, mx),
             "left": (my, 0), "right": (my, W - s), "right-1": (my, W - s - 1), "bit31": (my, 31)}
    if s == 3:
        sites["bit30"] = (my, 30)
    sites.update({f"near{y}{x}": (y, x) for y, x in NEAR_CORNER[1:]})
    return sites


def blocks():
    out = {}
    for shape in BLOCK_SHAPES:
        for s in (2, 3):
            for site, (y, x) in block_sites(shape, s).items():
                out[f"blocks/{_tag(shape)}/{s}x{s}@{site}"] = _block(shape, y, x, s)
    return out


RANDOM_SHAPES = ((40, 97), (12, 65), (5, 33), (64, 257), LONG_ROW, TALL)
RANDOM_SEED, RANDOM_P = 1, 0.01                                 # test_autocrop_cases_cpu.py: 0.05 < merged density < 0.95 on each


def random_masks():
    rng = np.random.default_rng(RANDOM_SEED)
    return {f"random/{_tag(shape)}/p{RANDOM_P}": rng.random(shape) < RANDOM_P for shape in RANDOM_SHAPES}


H_SWEEP_SHAPE = (30, 130)
H_SWEEP_X0 = {"in_word": 29, "across_words": 40}                # left block's first column: the gap lies in columns 32 .. 63 / crosses 63 | 64


def h_sweep():
    """two 3x3 blocks in a row, `gap` empty columns apart, well inside the plane"""
    out = {}
    for where, x0 in H_SWEEP_X0.items():
        for gap in H_GAPS:
            out[f"hsweep/{where}/gap{gap}"] = _block(H_SWEEP_SHAPE, 13, x0, 3) | _block(H_SWEEP_SHAPE, 13, x0 + 3 + gap, 3)
    return out


V_SWEEP_SHAPE = (40, 65)


def v_sweep():
    """two 3x3 blocks stacked, `gap` empty rows apart: the upper one on row 1, or the lower one ending on row H - 2"""
    H = V_SWEEP_SHAPE[0]
    out = {}
    for gap in V_GAPS:
        out[f"vsweep/top/gap{gap}"] = _block(V_SWEEP_SHAPE, 1, 30, 3) | _block(V_SWEEP_SHAPE, 4 + gap, 30, 3)
        out[f"vsweep/bottom/gap{gap}"] = _block(V_SWEEP_SHAPE, H - 4, 30, 3) | _block(V_SWEEP_SHAPE, H - 7 - gap, 30, 3)
    return out


def _draw(rows):
    return np.array([[c == "X" for c in r] for r in rows], bool)


def _at(shape, y, x, rows):
    m = np.zeros(shape, bool)
    d = _draw(rows)
    m[y:y + d.shape[0], x:x + d.shape[1]] = d
    return m


DIAG_SHAPE = (4, 40)
DIAG_COLUMNS = {"word": 31, "last": DIAG_SHAPE[1] - 2, "inner": 10}      # first column of the 2-wide contact: 31 | 32, W - 2 | W - 1


def diagonals():
    """two pixels that touch by a corner only, and the two three-pixel configurations where the pixel below has its left neighbour set:
    `left_ul` is joined through that neighbour (the kernel skips the upper-left link), `left_ur` only by its upper-right link"""
    out = {}
    for where, x in DIAG_COLUMNS.items():
        out[f"diag/{where}/backslash"] = _at(DIAG_SHAPE, 1, x, ["X.", ".X"])
        out[f"diag/{where}/slash"] = _at(DIAG_SHAPE, 1, x, [".X", "X."])
    for where, x in {"word": 31, "word+1": 32, "last": DIAG_SHAPE[1] - 2, "inner": 10}.items():
        out[f"diag/{where}/left_ul"] = _at(DIAG_SHAPE, 1, x - 1, ["X..", "XX."])
        out[f"diag/{where}/left_ur"] = _at(DIAG_SHAPE, 1, x - 1, ["..X", "XX."])
    return out


def diamond(leak=False):
    m = np.zeros((15, 15), bool)
    yy, xx = np.mgrid[:15, :15]
    m[np.abs(yy - 7) + np.abs(xx - 7) == 6] = True
    m[7, 7] = True
    if leak:
        m[3, 5] = False                                          # |dy| + |dx| = 4 + 2: not a vertex, the box stays
    return m


def _ring(m, y0, x0, y1, x1):
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True


def nested_rings():
    m = np.zeros((21, 37), bool)
    for k in (1, 3, 5):
        _ring(m, k, k, 20 - k, 36 - k)
    m[10, 18] = True
    return m


def u_shapes():
    """a U whose arms end on an edge, a 2x2 blob in its mouth that touches neither the U nor the edge"""
    base = np.zeros((12, 35), bool)
    base[0:8, 10] = base[0:8, 20] = True
    base[8, 10:21] = True
    base[3:5, 14:16] = True
    tall = np.zeros((35, 12), bool)
    tall[10, 0:8] = tall[20, 0:8] = True
    tall[10:21, 8] = True
    tall[14:16, 3:5] = True
    return {"u/top": base, "u/bottom": base[::-1].copy(), "u/left": tall, "u/right": tall[:, ::-1].copy()}


def corner_touch():
    """a blob that reaches the edge only through one diagonal step onto a corner pixel"""
    out = {}
    for name, (fy, fx) in {"tl": (False, False), "tr": (False, True), "bl": (True, False), "br": (True, True)}.items():
        m = np.zeros((9, 34), bool)
        m[0, 0] = True
        m[1:4, 1:4] = True
        out[f"corner/{name}"] = m[::-1 if fy else 1, ::-1 if fx else 1].copy()
    return out


def spiral(n=33):
    """a one-pixel square spiral with one-pixel gaps: one long 4-connected chain"""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        blocked = not (0 <= ny < n and 0 <= nx < n) or (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead])
        if blocked:
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead]):
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def comb():
    """a spine along the bottom row with a tooth on every fourth column, and the same hanging from the top row, the teeth interleaved
    one empty column apart: two components, each one long chain"""
    m = np.zeros((40, 65), bool)
    m[39, :] = True
    m[9:39, 0::4] = True
    m[0, :] = True
    m[1:31, 2::4] = True
    return m


def checkerboard():
    yy, xx = np.mgrid[:12, :33]
    return (yy + xx) % 2 == 0


def lattice():
    m = np.zeros((11, 33), bool)
    m[0::2, 0::2] = True
    return m


def area_extremes():
    """a frame whose box covers 59 % of the plane, one pixel outside it (0.0015 % of the plane) and one inside it"""
    m = np.zeros((256, 257), bool)
    _ring(m, 20, 20, 219, 219)
    m[240, 250] = True
    m[100, 100] = True
    return m


def components():
    out = dict(diagonals())
    out["diamond/closed"] = diamond()
    out["diamond/leak"] = diamond(leak=True)
    out["rings/nested3"] = nested_rings()
    out.update(u_shapes())
    out.update(corner_touch())
    out["chain/spiral"] = spiral()
    out["chain/comb"] = comb()
    out["checkerboard/12x33"] = checkerboard()
    out["lattice/11x33"] = lattice()
    out["area/extremes"] = area_extremes()
    return out


FAMILIES = {"fills": fills, "blocks": blocks, "random": random_masks, "hsweep": h_sweep, "vsweep": v_sweep, "components": components}


def all_cases():
    out = {}
    for f in FAMILIES.values():
        cases = f()
        assert not set(cases) & set(out)
        out.update(cases)
    return out


BAR_PAGES = ((150, 77), (140, 131), (180, 250))                 # W % 32 = 13, 3, 26


def bar_page(shape, seed=0):
    """a u8 page for the whole chain: light paper, a few dark bars more than the closing's reach apart, so that the merged mask is
    sparse and has several components (test_autocrop_cases_cpu.py pins both)"""
    H, W = shape
    rng = np.random.default_rng(seed)
    img = np.full(shape, 230, np.uint8)
    for y in range(14, H - 10, 32):
        w = int(rng.integers(10, 24))
        x = int(rng.integers(4, W - w - 4))
        img[y:y + 5, x:x + w] = 25
    return img


class Expected:
    """what the reference gives for one mask: the merged mask, (external mask, boxes) of the merged mask and of the mask itself"""

    def __init__(self, mask):
        import autocrop_ref as ref

        self.mask = mask
        self.merged = ref.merged_mask(mask)
        self.external = ref.external_components(self.merged)
        self.components = ref.external_components(mask)


_EXPECTED = {}


def expected():
    """{name: Expected} of every case, computed once per process (a quarter of a second) and shared by the tests; read-only"""
    if not _EXPECTED:
        for name, mask in all_cases().items():
            mask.setflags(write=False)
            _EXPECTED[name] = Expected(mask)
    return _EXPECTED
