"""-m gpu: every fused launch of the fast-mode detector, pool5, the BiLSTM recurrence and the recogniser's conv stack, ONE stage at a time with the production plans and
packed side tables of a live context (tools/micro/stage_shim.hip), against the fp64 reference of its own operation (tests/stage_ref.py) under
the tolerance rule stated there.  An L2 norm over a heat-map cannot see an error confined to a page border, a tile seam, the first pixel of the
second page of a batch or one time step of 79; these checks are per element, and a failure names the element and the region it lies in.

The exact mode's split-fp16 stages follow in the second half: rows of craft_forward_exact's conv table, the five pair kernels, every stage of the
recogniser's conv stack alone, xproj / lin / pred and lstm_exact_kernel, under the split-stage rule (stage_ref.EXACT_RULE).

Last, the crop stage into the wide layout every production pass uses (stage_crops_wide), bit exact against oracle/recog.py in all three modes.

hipErrorNotSupported (801) from a stage is a failure: production would silently take its fallback path on that shape.
Set BBOCR_STAGE_STATS=<file> to collect one JSON line per case (the table of DESIGN.md section 5)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3


@pytest.fixture(scope="module")
def shim_path(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    lib = os.path.join(ROOT, "bb-ocr_amd")
    so = str(tmp_path_factory.mktemp("stage_shim") / "stage_shim.so")
    cc = subprocess.run([hipcc, "-O2", "-std=c++20", "-shared", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(lib, "csrc"), "-I" + os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tools", "micro", "stage_shim.hip"), "-L" + lib, "-lbbocr", "-Wl,-rpath," + lib, "-o", so],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert cc.returncode == 0, cc.stdout.decode()[-2000:]
    return so


@pytest.fixture(scope="module")
def stage_states():
    from bb_ocr_amd import weights

    return R.craft_state(SEED), weights.synthetic_crnn_state(SEED)


class Stage:
    """a Reader of one precision + the shim bound to its context"""

    def __init__(self, so, states, el):
        import bb_ocr_amd

        self.el, self.dtype = el, R.DTYPES["fp16" if el == "exact" else el]     # exact: split fp16, stored values are [hi | lo] fp16 pairs
        self.reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=states, precision=el)      # loads libbbocr.so (after torch's HIP runtime)
        self.lib = C.CDLL(so)
        self.lib.stage_shim_error.restype = C.c_char_p
        self.W = R.Weights(states[0], "f32" if el == "exact" else el)
        self.RW = R.Weights(states[1], "f32" if el == "exact" else el)            # the recogniser's conv stack
        self.crnn = states[1]
        self.h = self.reader._h
        assert self.lib.stage_shim_det_el(self.h) == self.lib.stage_shim_rec_el(self.h) == (0 if el == "bf16" else 1)

    def call(self, fn, *args):
        """tensors go as (pointer, element count); synchronises torch's stream first (the library runs on its own non-blocking one)"""
        a = []
        for x in args:
            if torch.is_tensor(x):
                assert x.is_cuda and x.is_contiguous()
                a += [C.c_void_p(x.data_ptr()), C.c_size_t(x.numel())]
            elif x is None:                                   # an output the stage does not write
                a += [C.c_void_p(None), C.c_size_t(0)]
            else:
                a.append(x)
        torch.cuda.synchronize()
        rc = getattr(self.lib, fn)(self.h, *a)
        assert rc == 0, f"{fn}: status {rc}" + (" (hipErrorNotSupported: production would take the fallback path)" if rc == 801 else "") + \
            f" {self.lib.stage_shim_error().decode()}"

    def twice(self, run):
        """run() -> output tensor (NaN-filled before the launch); the two runs must agree bit for bit"""
        a, b = run(), run()
        v = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
        assert torch.equal(v(a), v(b)), f"two runs on the same input differ in {int((v(a) != v(b)).sum())} of {a.numel()} values"
        return a.cpu()

    def out(self, shape, dtype=None):
        return torch.full(shape, float("nan"), dtype=dtype or self.dtype, device="cuda")


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def st(request, shim_path, stage_states):
    s = Stage(shim_path, stage_states, request.param)
    yield s
    s.reader.close()


@pytest.fixture(scope="module")
def st_exact(shim_path, stage_states):
    s = Stage(shim_path, stage_states, "exact")       # the precision of conftest's reader_exact
    yield s
    s.reader.close()


def _act(shape, el, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(R.DTYPES[el])


def _record(stage, el, case, stats):
    path = os.environ.get("BBOCR_STAGE_STATS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"stage": stage, "el": el, "case": case, **stats}) + "\n")


def _check(st, stage, case, got, refs, el_out, **kw):
    _record(stage, st.el, case, R.check(got, *refs, el_out, f"{stage} {st.el} {case}", **kw))


# ------------------------------------------------------------------------------------------------ conv1_1 in conv1_2's prologue + 2x2 pool
@pytest.mark.parametrize("content", ["random", "zeros", "white"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("geom", [(17, 33, 32, 64), (32, 32, 32, 32), (50, 70, 64, 96), (96, 128, 96, 128), (1, 1, 32, 32)])
def test_c11_conv1_2_pool(st, geom, N, content):
    Hi, Wi, H32, W32 = geom
    g = torch.Generator().manual_seed(100 + Hi)
    rgb = {"random": lambda: torch.randint(0, 256, (N, Hi, Wi, 3), generator=g, dtype=torch.uint8),
           "zeros": lambda: torch.zeros((N, Hi, Wi, 3), dtype=torch.uint8),
           "white": lambda: torch.full((N, Hi, Wi, 3), 255, dtype=torch.uint8)}[content]()
    d = rgb.cuda()

    def run():
        o = st.out((N, H32 // 2, W32 // 2, 64))
        st.call("stage_c11_conv1_2_pool", d, N, Hi, Wi, H32, W32, o)
        return o

    got = st.twice(run)
    beyond = torch.ones((H32 // 2, W32 // 2), dtype=torch.bool)
    beyond[:Hi // 2, :Wi // 2] = False                  # pooled pixels whose 2x2 window touches the canvas beyond the page
    _check(st, "c11+conv1_2+pool", f"{N}x{Hi}x{Wi} on {H32}x{W32} {content}", got, R.refs_c11(st.W, rgb, Hi, Wi, H32, W32, st.el), st.el, beyond=beyond)


# ------------------------------------------------------------------------------------------------ two-source 1x1 (upconv1.conv.0)
@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 7, 5), (2, 16, 24)])
def test_up1a_two_sources(st, shape):
    N, H, W = shape
    f7, s4 = _act((N, H, W, 1024), st.el, 200), _act((N, H, W, 512), st.el, 201)
    df, ds = f7.cuda(), s4.cuda()

    def run():
        o = st.out((N, H, W, 512))
        st.call("stage_up1a", df, ds, N, H, W, o)
        return o

    rq = R.up1a(st.W, f7, s4, st.el)
    _check(st, "up1a", f"{N}x{H}x{W}", st.twice(run), (rq, rq, 0.0), st.el)


# ------------------------------------------------------------------------------------------------ 1x1 + up-sampling added in the epilogue
@pytest.mark.parametrize("shape", [(1, 4, 4), (3, 12, 20), (2, 40, 56), (1, 64, 96)])
@pytest.mark.parametrize("level", [2, 3, 4])
def test_addup(st, level, shape):
    N, H, W = shape
    cs, co = {2: (512, 256), 3: (256, 128), 4: (128, 64)}[level]
    skip, z = _act((N, H, W, cs), st.el, 300 + level), _act((N, H // 2, W // 2, co), st.el, 310 + level)
    dk, dz = skip.cuda(), z.cuda()

    def run():
        o = st.out((N, H, W, co))
        st.call("stage_addup", level, dk, dz, N, H, W, o)
        return o

    rq = R.addup(st.W, level, skip, z, st.el)
    _check(st, f"addup up{level}s", f"{N}x{H}x{W}", st.twice(run), (rq, rq, 0.0), st.el)


# ------------------------------------------------------------------------------------------------ upconv3 3x3 with upconv4's y-half 1x1 behind it
@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 24, 40), (1, 56, 72)])
def test_up3b_post_w(st, shape):
    N, H, W = shape
    u3a = _act((N, H, W, 128), st.el, 400)
    d = u3a.cuda()

    def run():
        o = st.out((N, H, W, 64))
        st.call("stage_up3b_post", d, N, H, W, o)
        return o

    _check(st, "up3b+post_w", f"{N}x{H}x{W}", st.twice(run), R.refs_up3b_post(st.W, u3a, st.el), st.el)


# ------------------------------------------------------------------------------------------------ upconv4 as one launch
@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 48, 64), (4, 240, 320)])
def test_up4_fused(st, shape):
    N, H, W = shape
    s1, z = _act((N, H, W, 128), st.el, 500), _act((N, H // 2, W // 2, 64), st.el, 501)
    ds, dz = s1.cuda(), z.cuda()

    def run():
        o = st.out((N, H, W, 32))
        st.call("stage_up4_fused", ds, dz, N, H, W, o)
        return o

    _check(st, "up4 fused", f"{N}x{H}x{W}", st.twice(run), R.refs_up4(st.W, s1, z, st.el), st.el)


# ------------------------------------------------------------------------------------------------ conv_cls.4 + classifier tail
@pytest.mark.parametrize("shape,scale", [((1, 16, 16), 1.0), ((2, 40, 56), 1.0), ((1, 112, 176), 1.0), ((2, 40, 56), 6.0)])
def test_cls_tail(st, shape, scale):
    N, H, W = shape
    c2 = _act((N, H, W, 32), st.el, 600, scale)
    d = c2.cuda()

    def run():
        o = st.out((N, H, W, 2), torch.float32)
        st.call("stage_cls_tail", d, N, H, W, o)
        return o

    refs = R.refs_cls_tail(st.W, c2, st.el)
    if scale > 1.0:             # the pushed case: both ReLUs clip on a sizeable share of the values
        w4, b4 = st.W.cls4()
        w1, b1, _, _ = st.W.tail()
        y = R.conv(R.nchw(c2.double()), w4, b4, pad=1)
        hpre = R.conv(torch.relu(y), w1, b1)
        assert 0.2 < float((y < 0).double().mean()) < 0.8 and 0.2 < float((hpre < 0).double().mean()) < 0.8
    _check(st, "cls4+tail", f"{N}x{H}x{W} x{scale:g}", st.twice(run), refs, None)


# ------------------------------------------------------------------------------------------------ pool5
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 10), (1, 30, 40)])
def test_pool5_bit_exact(st, shape):
    N, H, W = shape
    x = (torch.rand((N, H, W, 512), generator=torch.Generator().manual_seed(700)) * 8 - 4).to(st.dtype)
    d = x.cuda()

    def run():
        o = st.out((N, H, W, 512))
        st.call("stage_pool5", d, N, H, W, o)
        return o

    got, want = st.twice(run), R.pool5(x)
    assert (want < 0).any()
    diff = got.view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), f"pool5 {st.el} {shape}: {int(diff.sum())} values differ; by region {R.localise(diff)}"


# ------------------------------------------------------------------------------------------------ BiLSTM recurrence, mixed tile table
def _tiles(cap):
    return [(cap, 15), (3, 79), (1, 15), (cap, 255), (5, 639)]     # (sequences, T): T = imgW / 4 - 1 of the buckets 64, 320, 1024, 2560


@pytest.mark.parametrize("sigma", [1.5, 0.3])
@pytest.mark.parametrize("layer", [0, 1])
def test_bilstm_mixed_tiles(st, layer, sigma):
    TILES = _tiles(st.lib.stage_shim_tile_seqs(st.h))     # the tile capacity is production's, not a constant of the test
    assert TILES[0][0] >= 1
    perm = torch.tensor([st.lib.stage_shim_xproj_channel(d, g, u) for d in range(2) for g in range(4) for u in range(256)], dtype=torch.long)
    assert sorted(perm.tolist()) == list(range(2048))
    gen = torch.Generator().manual_seed(800 + layer)
    xs = [R.rnd(torch.randn((n, T, 2, 1024), generator=gen, dtype=torch.float64) * sigma, st.el) for n, T in TILES]
    rows = sum(n * T for n, T in TILES)
    rows_pad = (rows + 255) // 256 * 256                 # bbocr_crnn_logits' rows_pad: the kernel prefetches x two steps ahead
    xproj = torch.zeros((rows_pad, 2048), dtype=torch.float64)
    table, row0 = [], 0
    for (n, T), x in zip(TILES, xs):
        xproj[row0:row0 + n * T, perm] = x.reshape(n * T, 2048)
        table.append((row0, n, T, 0))
        row0 += n * T
    dx = xproj.to(st.dtype).cuda()

    def launch(entries):
        o = st.out((rows_pad, 512))
        t = np.ascontiguousarray(np.array(entries, dtype=np.int32))
        torch.cuda.synchronize()
        rc = st.lib.stage_lstm(st.h, layer, C.c_void_p(dx.data_ptr()), C.c_void_p(o.data_ptr()), C.c_size_t(rows_pad), t.ctypes.data_as(C.POINTER(C.c_int)), len(entries))
        assert rc == 0, f"stage_lstm: status {rc} {st.lib.stage_shim_error().decode()}"
        return o

    got = st.twice(lambda: launch(table))
    assert torch.isnan(got[rows:].float()).all()         # nothing is written behind the last sequence
    # tiles are independent: the same sequences, one tile per launch, give the same rows bit for bit
    for k, (r0, n, T, _) in enumerate(table):
        alone = launch([table[k]]).cpu()
        assert torch.equal(alone[r0:r0 + n * T].view(torch.int16), got[r0:r0 + n * T].view(torch.int16)), f"tile {k} differs when launched alone"
    wf, wb = R.lstm_weights(st.crnn, layer, st.el)
    rq, rn = [], []
    for x in xs:
        q, nq, _ = R.refs_bilstm(wf, wb, x, st.el)
        rq.append(q.reshape(-1, 512))
        rn.append(nq.reshape(-1, 512))
    rq, rn = torch.cat(rq), torch.cat(rn)
    E = 2.0 * (rq - rn).abs().max().item()
    g64 = got[:rows].double()
    try:
        _check(st, f"bilstm layer {layer}", f"sigma {sigma:g}", g64, (rq, rn, E), st.el, index_names=("row", "channel (fwd 0-255 | bwd 256-511)"))
    except AssertionError as e:
        tight, _ = R.bounds(rq, rn, E, st.el)
        miss = ~((g64 - rq).abs() <= tight)
        where = []
        for k, (r0, n, T, _) in enumerate(table):
            m = miss[r0:r0 + n * T].reshape(n, T, 2, 256)
            if m.any():
                s, t, d, _u = [int(v[0]) for v in torch.nonzero(m, as_tuple=True)]
                where.append(f"tile {k} ({n} x T={T}, first row {r0}): {int(m.sum())} beyond tight, first at sequence {s}, t {t}, {'bwd' if d else 'fwd'}")
        raise AssertionError(str(e) + "; " + "; ".join(where)) from None


# ------------------------------------------------------------------------------------------------ recogniser conv stack over the wide image
REC_PARTS = {"A": R.REC_PART_A, "B": R.REC_PART_B}
REC_ALONE = [1, 6, 0, 19]       # part A's crops also run as parts of their own: the first 64 (box 1), a 128 (box 6), the 320 (box 0), the last 64 (box 19)
SPLIT_LO_SCALE = 2048.0


class RecPlan:
    """rec_plan_part's layout of `widths` (box order), from production: slot / row0 per BOX, the plan's order, the totals"""

    def __init__(self, st, widths):
        n = len(widths)
        arr = lambda: (C.c_int * n)()
        self.widths, self.cw = list(widths), (C.c_int * n)(*widths)
        slot, row0, order, cols, rows = arr(), arr(), arr(), C.c_int(), C.c_int()
        rc = st.lib.stage_rec_plan(self.cw, n, slot, row0, order, C.byref(cols), C.byref(rows))
        assert rc == 0, f"stage_rec_plan: status {rc} {st.lib.stage_shim_error().decode()}"
        self.order, self.cols, self.rows = list(order), cols.value, rows.value
        assert sorted(self.order) == list(range(n))
        self.slot, self.row0 = [0] * n, [0] * n
        for k, i in enumerate(self.order):
            self.slot[i], self.row0[i] = slot[k], row0[k]

    def gap_columns(self, s):
        """the separator columns at a horizontal down-scale of 2^s"""
        m = torch.zeros(self.cols >> s, dtype=torch.bool)
        for sl, w in zip(self.slot, self.widths):
            m[(sl + w) >> s:(sl + w + R.REC_GAP) >> s] = True
        return m


def _rec_run(st, plan, first, last, wide_in, extra_rows=8):
    """stages first..last on the device -> (output tensor on the host after two agreeing runs, its per-stage shape).  After stage 7 the
    output has extra_rows NaN rows behind the part's."""
    m = 2 if st.el == "exact" else 1
    if last == 7:
        shape = (plan.rows + extra_rows, 256 * m)
    else:
        H, s, Cc = R.REC_IN[last + 1]
        shape = (H, (plan.cols >> s) - (1 if last == 6 else 0), Cc * m)
    d = wide_in.contiguous().cuda()

    def run():
        o = st.out(shape)
        st.call("stage_rec_features", plan.cw, len(plan.widths), first, last, d, o)
        return o

    return st.twice(run)


def _rec_crops(plan, last, out):
    """per-box views of a stage output: the crop's columns (last < 7) / rows (last = 7)"""
    if last == 7:
        return [out[r:r + w // 4 - 1] for r, w in zip(plan.row0, plan.widths)]
    s = R.REC_IN[last + 1][1]
    return [out[:, sl >> s:(sl >> s) + R.rec_in_shape(last + 1, w)[1]] for sl, w in zip(plan.slot, plan.widths)]


def _rec_structure(st, plan, first, last, out, wide_of, name):
    """checks 2, 3 and 4: separators +0 bit for bit, the gather's rows, every REC_ALONE crop alone = the same crop inside the part"""
    bits = out.view(torch.int16)
    if last <= 5:
        gap = plan.gap_columns(R.REC_IN[last + 1][1])
        dirty = (bits[:, gap] != 0).any(dim=2).any(dim=0)
        cols = torch.nonzero(gap).flatten()[dirty].tolist()
        assert not cols, f"{name}: separator columns {cols[:8]} of stage {last}'s output are not +0 (crop edges at {sorted(plan.slot)[:4]}...)"
    if last == 7:
        assert torch.isnan(out[plan.rows:].float()).all(), f"{name}: rows behind the part's {plan.rows} were written"
        assert not torch.isnan(out[:plan.rows].float()).any(), f"{name}: some of the part's {plan.rows} rows were not written"
    if len(plan.widths) > 1:
        inside = _rec_crops(plan, last, bits)
        for i in REC_ALONE:
            solo = RecPlan(st, [plan.widths[i]])
            got = _rec_crops(solo, last, _rec_run(st, solo, first, last, wide_of(solo, [i])).view(torch.int16))[0]
            diff = got != inside[i]
            assert not diff.any(), f"{name}: crop {i} (bucket {plan.widths[i]}) run as a part of its own differs from the same crop inside the part in " \
                f"{int(diff.sum())} values; " + R.rec_where(diff.reshape(-1), [plan.widths[i]], [tuple(diff.shape) if diff.dim() == 3 else (1,) + tuple(diff.shape)], [i])


@pytest.mark.parametrize("part", ["A", "B"])
@pytest.mark.parametrize("rng", R.REC_RANGES, ids=lambda r: f"{r[0]}-{r[1]}")
def test_rec_features_stages(st, rng, part):
    """Stages first..last of crnn_features_stages over a part of mixed width buckets against each crop's OWN fp64 reference (a crop alone with
    ordinary zero padding: tests/stage_ref.py never sees the wide layout), per element; separators, gather rows and crop independence bit for
    bit.  Single stages have E = 0 and carry the numerical weight; the pairs (k, k + 1) are where a clear left out after stage k would show in
    values; the chain 0..7 has an allowance seven |W| maps deep that decides nothing (E ~ 4e6 for bf16) and, as torch-fp32 itself misses the 1e-3 cap
    behind seven roundings, a cap of twice torch-fp32's own share on the same part (R.rec_chain_cap); there the placement -- rows, T, crop
    order -- is also checked without a tolerance (R.rec_misplaced)."""
    first, last = rng
    widths = REC_PARTS[part]
    plan = RecPlan(st, widths)
    assert (plan.slot, plan.row0) == tuple([v[plan.order.index(i)] for i in range(len(widths))] for v in R.rec_plan_like(widths)[:2])
    assert (plan.order, plan.cols, plan.rows) == R.rec_plan_like(widths)[2:] and plan.cols == {"A": 1744, "B": 68}[part]
    xs = R.rec_inputs(widths, first, st.el, plan.order)
    wide_of = lambda pl, boxes: R.rec_wide_pack(pl.slot, pl.cols, [xs[i] for i in boxes], first, torch.float64)[0].to(st.dtype)
    name = f"rec {first}..{last} {st.el} part {part}"
    out = _rec_run(st, plan, first, last, wide_of(plan, range(len(widths))))
    _rec_structure(st, plan, first, last, out, wide_of, name)
    got = [g[None] if last < 7 else g[None, None] for g in _rec_crops(plan, last, out)]
    refs = [R.refs_rec(st.RW, x, first, last, st.el) for x in xs]
    rq, rn = R.rec_flat([r[0] for r in refs]), R.rec_flat([r[1] for r in refs])
    E = 0.0 if first == last else R.rec_flat([r[2] for r in refs])
    g64 = R.rec_flat(got)
    cap = 1e-3
    if rng == (0, 7):
        cap, standin = R.rec_chain_cap(st.RW, widths, xs, rq, st.el)
        print(f"[stage] {name}: torch-fp32's own share beyond tight {standin:.3g}, cap {cap:.3g}")
    try:
        _check(st, f"rec {first}..{last}", f"part {part}", g64, (rq, rn, E), st.el, index_names=("element of the part",), cap=cap)
    except AssertionError as e:
        tight, allow = R.bounds(rq, rn, E, st.el)
        shapes = [tuple(r[0].shape[1:]) for r in refs]
        miss_a, miss_t = ~((g64 - rn).abs() <= allow), ~((g64 - rq).abs() <= tight)
        raise AssertionError(f"{e}; beyond the allowance: {R.rec_where(miss_a, widths, shapes) or 'none'}; beyond the tight bound: "
                             f"{R.rec_where(miss_t, widths, shapes) or 'none'}") from None
    if rng == (0, 7):
        bad = R.rec_misplaced(got, [r[0] for r in refs], widths)
        assert not bad, f"{name}: " + "; ".join(bad)


def _pair_value(t, Cc):
    """[.., 2 Cc] fp16 pairs [hi | lo] -> fp64 values hi + lo / SPLIT_LO_SCALE"""
    return t[..., :Cc].double() + t[..., Cc:].double() / SPLIT_LO_SCALE


@pytest.mark.parametrize("part", ["A", "B"])
def test_rec_features_exact(st_exact, part):
    """Exact mode (split fp16: crnn_conv0_kernel<REC_SPLIT> on the codes 1 + grey, [hi | lo] pairs, the split 3-row mean): separators after
    stages 0..5, gather rows and crop independence bit for bit, and the chain 0..7 against the fp64 network on the fp32-normalised pixels:
    relative L2 <= 2e-5 per crop (the mode's bound in test_crnn_logits_fp16_and_exact) and per time step -- unless torch-fp32, which this mode
    promises to follow, is itself beyond 1e-5 on some step, then twice its worst step (on these inputs it is about 3e-7: the bound is 2e-5)."""
    st = st_exact
    widths = REC_PARTS[part]
    plan = RecPlan(st, widths)
    px = R.rec_pixels(widths, R.REC_SEED, plan.order)
    codes = [(g.to(torch.int16) + 1)[None, :, :, None] for g in px]
    wide_of = lambda pl, boxes: R.rec_wide_pack(pl.slot, pl.cols, [codes[i] for i in boxes], 0, torch.int16)[0]
    for last in range(8):
        name = f"rec 0..{last} exact part {part}"
        out = _rec_run(st, plan, 0, last, wide_of(plan, range(len(widths))))
        _rec_structure(st, plan, 0, last, out, wide_of, name)
    worst32 = worst_crop = worst_step = 0.0
    for i, (g, rows) in enumerate(zip(px, _rec_crops(plan, 7, out))):
        x = R.rec_normalise(g, "f32")
        ref = R.rec_chain(st.RW, x, 0, 7, None, q=False)[0, 0]
        r32 = R.rec_chain(st.RW, x, 0, 7, None, q=False, dt=torch.float32)[0, 0].double()
        got = _pair_value(rows, 256)
        worst32 = max(worst32, float(((r32 - ref).norm(dim=1) / ref.norm(dim=1)).max()))
        crop, step = float((got - ref).norm() / ref.norm()), (got - ref).norm(dim=1) / ref.norm(dim=1)
        worst_crop, worst_step = max(worst_crop, crop), max(worst_step, float(step.max()))
        print(f"[stage] rec exact part {part} crop {i} (bucket {widths[i]}): relative L2 {crop:.3g}, worst time step {float(step.max()):.3g} at t = {int(step.argmax())}")
    bound = 2e-5 if worst32 <= 1e-5 else 2.0 * worst32
    print(f"[stage] rec exact part {part}: worst crop {worst_crop:.3g}, worst time step {worst_step:.3g}; torch-fp32's worst time step {worst32:.3g}, bound {bound:.3g}")
    _record("rec 0..7", "exact", f"part {part}", {"worst_crop": worst_crop, "worst_step": worst_step, "fp32_worst_step": worst32, "step_bound": bound})
    assert worst_crop <= 2e-5, f"{name}: a crop's relative L2 {worst_crop:.3g} > 2e-5"
    assert worst_step <= bound, f"{name}: a time step's relative L2 {worst_step:.3g} > {bound:.3g}"


# ================================================================================================ exact mode: split-fp16 stages, one at a time
# The rule (R.EXACT_RULE): |got - ref| <= u |ref| + (2^-21 + 2 q32) S + 2^-35 per element, q32 from the reference's own float32 stand-in.
def _exact_stats(stage, case, stats):
    _record(stage, "exact", case, stats)


def test_exact_table_is_the_references_table(st_exact):
    """craft_forward_exact's conv table (detector.cpp), row by row, is R.EXACT_CONVS -- whose order the CPU suite proves against
    oracle.nets.CRAFT; a row deleted or moved in production changes what the pass runs, and this test and the cases below with it"""
    st = st_exact
    assert st.lib.stage_exact_rows() == len(R.EXACT_CONVS)
    for i, (name, ck, bk, relu_out, store, pool, pool_relu, keep_full, K, dil, _) in enumerate(R.EXACT_CONVS):
        nm, info = C.create_string_buffer(16), (C.c_int * 8)()
        rc = st.lib.stage_exact_row_info(st.h, i, nm, info)
        assert rc == 0, f"stage_exact_row_info: status {rc} {st.lib.stage_shim_error().decode()}"
        w, _b = st.W.layer(ck, bk)
        assert (nm.value.decode(), list(info)) == (name, [w.shape[1], int(relu_out), store, pool, int(pool_relu), int(keep_full), K, dil]), (i, name)
        assert store == w.shape[0] and K == w.shape[2]


@pytest.mark.parametrize("name,shape,route", R.EXACT_CONV_CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s, _ in R.EXACT_CONV_CASES])
def test_exact_conv_rows(st_exact, name, shape, route):
    """Rows of the exact detector's conv table on random pair tensors, through craft_exact_conv.  Route per case (launch_conv_el):
    conv1_2 1x16x16 / 3x34x50: 3x3 DMA, BN 64, pooled shared epilogue;  conv2_2 2x18x30: 3x3 DMA, BN 128, pooled shared epilogue with store_full and
    pool_relu (both outputs checked);  conv3_1 1x19x37: 3x3 DMA, BN 128, plain pair epilogue, two cout tiles;  fc6 1x2x2 / 2x15x20 / 1x13x6: the
    dilated sub-lattice path (a.sub, a.stack, the magic-number row division);  fc7 2x7x5, up1a 1x2x2 / 3x7x5: 1x1 DMA (K = 3,072 / 4,608);
    up4b 2x16x32, cls4 1x16x16 / 2x24x40: 16x16 tiles (18x18 patch) and so the <= 32-cout instantiation -- up4b with 32 stored couts and six
    k-chunks, cls4 with 16 and three;  up4b 2x18x30: 8x32 tiles (10x34 patch), the ordinary three-deep ring of the BN 64 3x3 DMA kernel."""
    st = st_exact
    a_pair, outs = R.exact_conv_case(st.W, name, shape)
    row = R.EXACT_ROW[name]
    _, _, _, _, store, pool, _, keep_full, _, _, _ = R.EXACT_CONVS[row]
    N, H, W = shape
    d = a_pair.cuda()
    main = "pool" if pool else "full"
    shp = {k: tuple(o["ref"].shape[:3]) + (2 * store,) for k, o in outs.items()}
    n_main = int(np.prod(shp[main]))

    def run():
        o = st.out(shp[main])
        f = st.out(shp["full"]) if keep_full else None
        st.call("stage_exact_conv", row, d, N, H, W, o, f)
        return torch.cat([o.reshape(-1)] + ([f.reshape(-1)] if keep_full else []))

    flat = st.twice(run)
    got = {main: flat[:n_main].reshape(shp[main])}
    if keep_full:
        got["full"] = flat[n_main:].reshape(shp["full"])
    for k, o in outs.items():
        assert o["q32"] <= R.Q32_MAX
        case = f"{N}x{H}x{W}" + (f" {k}" if len(outs) > 1 else "")
        _exact_stats(f"exact {name}", case, R.split_check(R.pair_decode(got[k]), o["ref"], o["S"], o["q32"], R.U_PAIR, f"exact {name} {case} [{route}]"))


@pytest.mark.parametrize("content", ["random", "zeros", "white"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("geom", R.C11_GEOMS)
def test_exact_conv1_1(st_exact, geom, N, content):
    """pair_conv1_1: a canvas pixel beyond the page is a normalised raw zero, a pixel beyond the canvas the conv's zero padding"""
    st = st_exact
    Hi, Wi, H32, W32 = geom
    rgb = R.c11_pages(geom, N, content)
    d = rgb.cuda()

    def run():
        o = st.out((N, H32, W32, 128))
        st.call("stage_exact_conv1_1", d, N, Hi, Wi, H32, W32, o)
        return o

    got = R.pair_decode(st.twice(run))
    r = R.exact_c11(st.W, rgb, Hi, Wi, H32, W32)
    q32 = R.split_q32(r["standin"], r["ref"], r["S"])
    assert q32 <= R.Q32_MAX
    case = f"{N}x{Hi}x{Wi} on {H32}x{W32} {content}"
    _exact_stats("exact conv1_1", case, R.split_check(got, r["ref"], r["S"], q32, R.U_PAIR, f"exact conv1_1 {case}"))


def _bits_equal(got, want, name):
    diff = got.view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.numel()} 16-bit values differ; by region {R.localise(diff)}"


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 10), (1, 30, 40)])
@pytest.mark.parametrize("op", ["relu", "pool5"])
def test_exact_pair_selection_kernels(st_exact, op, shape):
    """pair_relu / pair_maxpool3x3s1 are selections on the decoded value: bit for bit the numpy restatement decode -> select -> encode, and the
    decoded output is exactly the selected input value"""
    st = st_exact
    N, H, W = shape
    x = R.pair_plane(shape, 700)
    d = x.cuda()

    def run():
        o = st.out((N, H, W, 1024))
        st.call(f"stage_exact_{op}", d, N, H, W, 512, o)
        return o

    got = st.twice(run)
    want = R.pair_relu(x) if op == "relu" else R.pair_pool5(x)
    _bits_equal(got, want, f"exact {op} {shape}")
    v = R.pair_decode(x)
    sel = torch.clamp(v, min=0) if op == "relu" else R.nhwc(torch.nn.functional.max_pool2d(R.nchw(v), 3, 1, 1))
    assert torch.equal(R.pair_decode(got), sel)


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 3, 5)])
def test_exact_upcat_same_size(st_exact, shape):
    """upcat(f7, s4): a plain channel concat of two pair tensors, bit for bit"""
    st = st_exact
    N, H, W = shape
    y, sk = R.upcat_same_inputs(shape)
    dy, ds = y.cuda(), sk.cuda()

    def run():
        o = st.out((N, H, W, 2 * 1536))
        st.call("stage_exact_upcat", dy, H, W, 1024, ds, 512, N, H, W, o)
        return o

    got = st.twice(run)
    _bits_equal(got, R.pair_upcat_same(y, sk), f"exact upcat same size {shape}")
    assert torch.equal(R.pair_decode(got), torch.cat([R.pair_decode(y), R.pair_decode(sk)], dim=-1))


@pytest.mark.parametrize("shape,chans", [((1, 1, 1), (256, 512)), ((2, 3, 5), (128, 256)), ((1, 20, 28), (64, 128))])
def test_exact_upcat_upsampling(st_exact, shape, chans):
    """cat([F.interpolate(y, 2x, bilinear, align_corners = False), skip]): the up-sampled channels against the fp64 blend of the decoded values,
    bound 2^-22 |ref| + 2^-23 (blend of the four |neighbours|); the skip's channels bit for bit"""
    st = st_exact
    N, h, w = shape
    Cy, Cs = chans
    g = torch.Generator().manual_seed(720)
    y, sk = R.pair_pack(torch.randn((N, h, w, Cy), generator=g) * 3), R.pair_pack(torch.randn((N, 2 * h, 2 * w, Cs), generator=g) * 3)
    dy, ds = y.cuda(), sk.cuda()

    def run():
        o = st.out((N, 2 * h, 2 * w, 2 * (Cy + Cs)))
        st.call("stage_exact_upcat", dy, h, w, Cy, ds, Cs, N, 2 * h, 2 * w, o)
        return o

    got = st.twice(run)
    hi, lo = R.pair_halves(got)
    # the skip's channels pass through decode -> encode like every value here: the VALUE is the input's exactly, the bits those of the re-encoded
    # value (a pair whose lo is exactly half an ulp of its hi re-encodes to the neighbouring hi: 2 of 61,440 values of the 2x3x5 case)
    skip_out = torch.cat([hi[..., Cy:], lo[..., Cy:]], dim=-1).contiguous()
    _bits_equal(skip_out, R.pair_pack(R.pair_decode(sk, dt=torch.float32)), f"exact upcat {shape}: skip channels")
    assert torch.equal(R.pair_decode(skip_out), R.pair_decode(sk))
    ref, blend = R.pair_upcat_up(y)
    val = R.pair_value(hi[..., :Cy], lo[..., :Cy])
    bound = R.upcat_up_bound(ref, blend)
    err = (val - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"[stage] exact upcat 2x {shape}: max |got - ref| / bound {worst:.3g}")
    _exact_stats("exact upcat 2x", f"{N}x{h}x{w}", {"worst": worst})
    miss = ~(err <= bound)
    assert not miss.any(), f"exact upcat 2x {shape}: {int(miss.sum())} up-sampled values beyond the bound (worst {worst:.3g} x); by region {R.localise(miss)}"


@pytest.mark.parametrize("shape,scale", [((1, 16, 16), 1.0), ((2, 40, 56), 1.0), ((2, 40, 56), 6.0)])
def test_exact_cls_tail(st_exact, shape, scale):
    st = st_exact
    N, H, W = shape
    c3 = R.pair_pack(torch.randn((N, H, W, 16), generator=torch.Generator().manual_seed(600)).abs() * scale)
    d = c3.cuda()

    def run():
        o = st.out((N, H, W, 2), torch.float32)
        st.call("stage_exact_cls_tail", d, N, H, W, o)
        return o

    got = st.twice(run).double()
    r = R.exact_cls_tail(st.W, c3)
    q32 = R.split_q32(r["standin"], r["ref"], r["S"])
    assert q32 <= R.Q32_MAX
    case = f"{N}x{H}x{W} x{scale:g}"
    _exact_stats("exact cls tail", case, R.split_check(got, r["ref"], r["S"], q32, R.U_F32, f"exact cls tail {case}"))


# ------------------------------------------------------------------------------------------------ exact mode: the sequence half
SEQ_ROWS, SEQ_ROWS_PAD = 300, 512


def _xproj_perm(st):
    perm = torch.tensor([st.lib.stage_shim_xproj_channel(d, g, u) for d in range(2) for g in range(4) for u in range(256)], dtype=torch.long)
    assert sorted(perm.tolist()) == list(range(2048))
    return perm


@pytest.mark.parametrize("which,layer", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)], ids=["xproj0", "xproj1", "lin0", "lin1", "pred"])
def test_exact_sequence_gemms(st_exact, which, layer):
    """xproj[l], lin[l] and pred through crnn_sequence's own helpers on 300 rows padded to 512.  lin reads the LSTM's pair, whose lo half is
    UNSCALED (its plan is the one packed with lo_scale 1); pred's columns 97..111 belong to no class and are not read."""
    st = st_exact
    w, b, lo_scale = R.seq_gemm_weights(st.crnn, which, layer, _xproj_perm(st))
    K, cout = w.shape[1], w.shape[0]
    g = torch.Generator().manual_seed(860 + 10 * which + layer)
    v = torch.randn((SEQ_ROWS_PAD, K), generator=g)
    v = torch.tanh(v) if which == 1 else v
    v[SEQ_ROWS:] = 0
    a_pair = R.pair_pack(v, lo_scale)
    d = a_pair.cuda()
    f32 = which != 1
    width = {0: 2048, 1: 512, 2: 112}[which]

    def run():
        o = st.out((SEQ_ROWS_PAD, width), torch.float32 if f32 else None)
        torch.cuda.synchronize()
        rc = st.lib.stage_exact_seq_gemm(st.h, which, layer, C.c_void_p(d.data_ptr()), C.c_size_t(d.numel()), C.c_size_t(SEQ_ROWS_PAD), C.c_void_p(o.data_ptr()),
                                         C.c_size_t(o.numel()))
        assert rc == 0, f"stage_exact_seq_gemm: status {rc} {st.lib.stage_shim_error().decode()}"
        return o

    out = st.twice(run)
    pre = R.split_conv(w, b, a_pair.reshape(1, SEQ_ROWS_PAD // 256, 256, 2 * K), lo_scale=lo_scale)
    rows = lambda t: R.nhwc(t).reshape(SEQ_ROWS_PAD, cout)
    ref, S = rows(pre["ref"]), rows(pre["S"])
    q32 = R.split_q32(rows(pre["standin"]), ref, S)
    assert q32 <= R.Q32_MAX
    got = out.double()[:, :cout] if f32 else R.pair_decode(out)
    name = f"exact {('xproj', 'lin', 'pred')[which]}" + ("" if which == 2 else f"[{layer}]")
    _exact_stats(name, f"{SEQ_ROWS} rows", R.split_check(got, ref, S, q32, R.U_F32 if f32 else R.U_PAIR, name))


@pytest.mark.parametrize("sigma", [1.5, 0.3])
@pytest.mark.parametrize("layer", [0, 1])
def test_exact_bilstm_mixed_tiles(st_exact, layer, sigma):
    """lstm_exact_kernel on a mixed tile table built from production's tile capacity: nothing written behind the last row, every tile alone
    equals itself in the table bit for bit, and per tile max |got - ref| <= 8 max |fp32 - ref| + 2^-22 (R.EXACT_RULE); the output pair is
    decoded with lo scale 1"""
    st = st_exact
    cap = st.lib.stage_shim_tile_seqs(st.h)
    assert cap >= 1
    tiles = R.EXACT_TILES(cap)
    perm = _xproj_perm(st)
    xs = R.exact_lstm_inputs(cap, layer, sigma)
    rows = sum(n * T for n, T in tiles)
    rows_pad = (rows + 255) // 256 * 256
    xproj = torch.zeros((rows_pad, 2048), dtype=torch.float32)
    table, row0 = [], 0
    for (n, T), x in zip(tiles, xs):
        xproj[row0:row0 + n * T, perm] = x.reshape(n * T, 2048)
        table.append((row0, n, T, 0))
        row0 += n * T
    dx = xproj.cuda()

    def launch(entries):
        o = st.out((rows_pad, 1024))
        t = np.ascontiguousarray(np.array(entries, dtype=np.int32))
        torch.cuda.synchronize()
        rc = st.lib.stage_lstm(st.h, layer, C.c_void_p(dx.data_ptr()), C.c_void_p(o.data_ptr()), C.c_size_t(rows_pad), t.ctypes.data_as(C.POINTER(C.c_int)), len(entries))
        assert rc == 0, f"stage_lstm: status {rc} {st.lib.stage_shim_error().decode()}"
        return o

    got = st.twice(lambda: launch(table))
    assert torch.isnan(got[rows:].float()).all()         # nothing is written behind the last sequence
    for k, (r0, n, T, _) in enumerate(table):
        alone = launch([table[k]]).cpu()
        assert torch.equal(alone[r0:r0 + n * T].view(torch.int16), got[r0:r0 + n * T].view(torch.int16)), f"tile {k} differs when launched alone"
    wf, wb = R.lstm_weights(st.crnn, layer, "exact")
    val = R.pair_decode(got[:rows], 1.0)
    worst, standin_worst, problems = 0.0, 0.0, []
    for k, ((r0, n, T, _), x) in enumerate(zip(table, xs)):
        _model, ref, bound = R.refs_bilstm(wf, wb, x, "exact")
        standin = R.bilstm(wf, wb, x, "exact", True, torch.float32)
        standin_worst = max(standin_worst, float((standin - ref).abs().max()) / bound)
        err = (val[r0:r0 + n * T].reshape(n, T, 512) - ref).abs()
        ok = torch.isfinite(err) & (err <= bound)
        worst = max(worst, float(torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf"))).max()) / bound)
        if not ok.all():
            s, t, ch = [int(v[0]) for v in torch.nonzero(~ok, as_tuple=True)]
            problems.append(f"tile {k} ({n} x T={T}, first row {r0}): {int((~ok).sum())} beyond {bound:.3g}, first at sequence {s}, t {t}, {'bwd' if ch >= 256 else 'fwd'} unit {ch % 256}")
    print(f"[stage] exact bilstm layer {layer} sigma {sigma:g}: max |got - ref| / bound {worst:.3g}, the float32 split stand-in's {standin_worst:.3g}")
    _exact_stats(f"exact bilstm layer {layer}", f"sigma {sigma:g}", {"worst": worst, "standin": standin_worst})
    assert not problems, "; ".join(problems)


@pytest.mark.parametrize("part", ["A", "B"])
@pytest.mark.parametrize("k", range(R.REC_STAGES))
def test_exact_rec_stage_alone(st_exact, k, part):
    """every stage of crnn_features_stages ALONE in the exact mode, parts A and B, per element under R.EXACT_RULE against each crop's own fp64
    reference: stage 0 takes the codes 1 + grey (crnn_conv0_kernel<REC_SPLIT>, a float32 FMA chain), stages 1..6 are split plans on pair
    tensors, stage 7 the float32 3-row mean on the decoded pairs + gather.  (Separators, gather rows and crop independence: bit for bit in
    test_rec_features_exact.)"""
    st = st_exact
    widths = REC_PARTS[part]
    plan = RecPlan(st, widths)
    xs = R.exact_rec_inputs(widths, k, plan.order)
    if k == 0:
        codes = [(g.to(torch.int16) + 1)[None, :, :, None] for g in R.rec_pixels(widths, R.REC_SEED, plan.order)]
        wide = R.rec_wide_pack(plan.slot, plan.cols, codes, 0, torch.int16)[0]
    else:
        wide = R.rec_wide_pack_pair(plan.slot, plan.cols, xs, k)
    out = _rec_run(st, plan, k, k, wide)
    got = R.rec_flat([R.pair_decode(g) for g in _rec_crops(plan, k, out)])
    p = R.exact_rec_part(st.RW, k, xs)
    assert p["q32"] <= R.Q32_MAX
    name = f"exact rec stage {k} part {part}"
    try:
        stats = R.split_check(got, p["ref"], p["S"], p["q32"], R.U_PAIR, name)
    except AssertionError as e:
        miss = ~((got - p["ref"]).abs() <= R.split_bound(p["ref"], p["S"], p["q32"], R.U_PAIR))
        raise AssertionError(f"{e}; {R.rec_where(miss, widths, p['shapes'])}") from None
    _exact_stats(f"exact rec stage {k}", f"part {part}", stats)


# ------------------------------------------------------------------------------------------------ the crop stage into the wide layout
def _crops_wide(st, contrast):
    """what every production pass runs -- all crops of a part side by side in ONE [64][cols] image, slot = first column, REC_GAP zero
    columns after each crop -- planned and launched by the production functions (stage_crops_wide) on the shared cases of
    tests/crop_cases.py, bit exact against oracle/recog.py at each crop's own padded width; contrast > 0: the LUTs of the contrast retry"""
    import crop_cases as cc

    el = st.el
    nh, nf = len(cc.HORI), len(cc.FREE)
    harr = (C.c_int * (4 * nh))(*[int(v) for b in cc.HORI for v in b])
    farr = (C.c_double * (8 * nf))(*[float(v) for q in cc.FREE for p in q for v in p])
    box, slot, imgw = ((C.c_int * (nh + nf))() for _ in range(3))
    n, cols = C.c_int(), C.c_int()
    rc = st.lib.stage_crops_wide_plan(cc.H, cc.W, harr, nh, farr, nf, box, slot, imgw, C.byref(n), C.byref(cols))
    assert rc == 0, st.lib.stage_shim_error().decode()
    n, cols = n.value, cols.value
    items = cc.stage_a_cases()
    kept = [k for k, it in enumerate(items) if it]
    assert sorted(box[:n]) == kept, "the plan keeps other boxes than the oracle"
    at = 0
    for i in range(n):                         # the crops tile the image: slot, imgW columns, REC_GAP columns, the next slot
        assert slot[i] == at and imgw[i] == items[box[i]][1], (i, slot[i], at, imgw[i], cc.describe(box[i]))
        at += imgw[i] + R.REC_GAP
    assert at == cols
    regimes = [cc.classify(*cc.source_size(k)) for k in box[:n]]
    assert len(set(imgw[:n])) >= 3 and any(r[1] for r in regimes) and any(k >= nh for k in box[:n])     # widths, a tall crop, a warped one
    d = torch.from_numpy(cc.make_page().copy()).cuda()
    out = torch.full((64, cols), cc.SENTINEL, dtype=torch.int16, device="cuda")
    st.call("stage_crops_wide", d, cc.H, cc.W, harr, nh, farr, nf, C.c_double(contrast), out)
    got = out.cpu().numpy()
    for i in range(n):
        k, s, w = box[i], slot[i], imgw[i]
        what = f"wide layout {el}, contrast {contrast}, crop {i} at columns [{s}, {s + w}) = {cc.describe(k)}"
        cc.assert_same(got[:, s:s + w], cc.to_el(cc.reference(k, None, contrast), el), what)
        gap = got[:, s + w:s + w + R.REC_GAP]
        assert not gap.any(), f"{what}: the {R.REC_GAP} columns behind it are not zero, first at (row, column) {cc.first_diff(gap, np.zeros_like(gap))}"
    assert not (got == cc.SENTINEL).any(), f"wide layout {el}: sentinel left at (row, column) {tuple(np.argwhere(got == cc.SENTINEL)[0])}"


@pytest.mark.parametrize("contrast", [0.0, 0.5])
def test_crops_wide_layout(st, contrast):
    _crops_wide(st, contrast)


@pytest.mark.parametrize("contrast", [0.0, 0.5])
def test_crops_wide_layout_exact(st_exact, contrast):
    _crops_wide(st_exact, contrast)
