"""CPU: which conv kernel a launch takes, from a dry run of the launch code itself (bbocr_host_conv_route walks launch_conv's dispatch and
returns before the first HIP call), and what that dispatch promises the kernels.

* every row of tests/conv_route_cases.py takes the route it names, in both element types; the refusals are refused;
* every id of the route enum is reached by a row or listed as stage-only with the stage test that runs it;
* over 2,400 derandomised hypothesis examples: whenever the dispatch accepts a shape, the geometry it settled satisfies what the kernels assume
  (tile and patch sizes, staging parts against taps, LDS, coverage, the pooling tile rule, the magic division of the stacked phase images);
* the rows' references stay inside the per-element rule of tests/stage_ref.py::check on their own (torch-fp32 standing in for the kernel), and
  seven planted defects each fail it on the named row's inputs.
"""
import os
import sys

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import conv_route_cases as cc  # noqa: E402
import stage_ref as R  # noqa: E402

SETTINGS = dict(deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
ELS = {"bf16": 0, "fp16": 1}
HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


# ---------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_expected_route(lib, name, el):
    c = cc.BY_NAME[name]
    rc, got = cc.dry_route(lib, c, ELS[el])
    assert rc == 0 and got["status"] == 0, (rc, got)
    assert got["el"] == ELS[el]
    assert (got["OH"], got["OW"]) == ((1, c.N * c.H * c.W) if got["id"].startswith("DMA1X1") else cc.out_hw(c))
    assert not cc.route_mismatch(c.route, got), f"{name}: expected != dry run: {cc.route_mismatch(c.route, got)}; dry run: {got}"
    assert got["id"].startswith("GEN") == (c.family == "generic")


@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("row", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_refusals(lib, row, el):
    name, N, H, W, Cin, Cout, KH, KW, pad, dil, _ = row
    c = cc._c(name, "refused", N, H, W, Cin, Cout, KH, KW, pad, dil, {}, "")
    rc, got = cc.dry_route(lib, c, ELS[el])
    assert rc == -2                                              # BBOCR_ERR_HIP: what bbocr_op_conv2d returns for a refused launch
    assert got["id"] == "NONE" and got["status"] == HIP_INVALID_VALUE and got["grid"] == 0


def test_coverage_of_the_route_enum():
    from bb_ocr_amd import _lib

    ids = set(_lib.CONV_ROUTE_IDS[1:])
    by_rows = {c.route["id"] for c in cc.CASES}
    stage_only = set(cc.STAGE_ONLY)
    assert by_rows <= ids and stage_only <= ids
    assert not (by_rows & stage_only), "a stage-only id that a row reaches"
    assert ids - by_rows - stage_only == set(), f"route ids nothing accounts for: {sorted(ids - by_rows - stage_only)}"
    src = open(os.path.join(ROOT, "tests", "test_gpu_stages.py")).read()
    for test in list(cc.STAGE_ONLY.values()) + list(cc.STAGE_ONLY_SWITCHES.values()):
        assert f"def {test}(" in src, test
    # every instantiation of the generic kernel: 2 tile widths x 3 PITER (x 2 element types: test_expected_route)
    assert {c.route["id"] for c in cc.CASES if c.family == "generic"} == {f"GEN{bn}_P{p}" for bn in (64, 128) for p in (4, 8, 16)}
    assert any(c.N == 2 for c in cc.CASES if c.family == "generic") and any(c.N == 2 for c in cc.CASES if c.family == "dma")


def test_header_and_binding_agree():
    from bb_ocr_amd import _lib

    header = open(os.path.join(ROOT, "include", "bbocr.h")).read()
    enum = header[header.index("BBOCR_ROUTE_NONE = 0"):header.index("BBOCR_ROUTE_COUNT")]
    import re

    names = re.findall(r"BBOCR_ROUTE_([A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert tuple(names) == _lib.CONV_ROUTE_IDS
    struct = header[header.index("typedef struct bbocr_conv_route {"):header.index("} bbocr_conv_route;")]
    fields = []
    for decl in re.findall(r"\bint ([^;]+);", re.sub(r"/\*.*?\*/", "", struct, flags=re.S)):
        fields += [f.strip() for f in decl.split(",")]
    assert tuple(fields) == _lib.CONV_ROUTE_FIELDS


# ---------------------------------------------------------------------------------------------------- invariants of every accepted shape
def _invariants(a, r):
    """a: the arguments; r: the dry run's route of an ACCEPTED shape"""
    N, H, W, Cin, Cout, KH, KW, pad, dil, pool, f32, full = a
    OH, OW = H + 2 * pad - (KH - 1) * dil, W + 2 * pad - (KW - 1) * dil
    fam = r["id"]
    bn = r["wn"] * 64
    assert r["threads"] == r["wm"] * r["wn"] * 64 and r["wm"] * r["mf"] * 16 == 256           # 256 output pixels per workgroup
    assert r["TH"] * r["TW"] == 256
    assert r["nchunks"] == Cin // 32 and r["ntaps"] == KH * KW and r["ntiles_n"] * bn >= Cout
    assert 0 < r["lds_bytes"] <= 160 * 1024
    if fam.startswith("DMA1X1"):
        assert (r["OH"], r["OW"]) == (1, N * H * W) and r["tiles_x"] * 256 >= N * H * W > (r["tiles_x"] - 1) * 256 and r["tiles_y"] == 1
        assert r["grid"] == r["tiles_x"] * r["ntiles_n"]
        return
    assert (r["OH"], r["OW"]) == (OH, OW)
    d = 1 if r["sub"] > 1 else dil                             # the sub-lattice route runs plain 3x3 convs on the phase images
    assert r["PH"] == r["TH"] + (KH - 1) * d and r["PW"] == r["TW"] + (KW - 1) * d
    assert r["PH"] * r["PW"] <= r["NP"] and r["NP"] % 16 == 0
    if fam.startswith("GEN"):
        assert r["piter"] * 64 >= r["NP"] and r["piter"] in (4, 8, 16)
        nparts = r["piter"] // 4
        assert (r["ntaps"] - 1) // nparts >= 1 if r["ntaps"] >= 3 else nparts == 1
        assert r["lds_bytes"] == 2 * bn * 64 + 2 * r["NP"] * 64
    else:
        assert r["NP"] == r["npb"] * 64 and r["nps"] >= r["PH"] * r["PW"] and r["nps"] <= r["NP"]
    if r["sub"] > 1:
        s, LH, LW = r["sub"], -(-OH // r["sub"]), -(-OW // r["sub"])
        assert s == dil and r["stack"] == LH and not pool
        assert r["tiles_x"] * r["TW"] >= LW and r["tiles_y"] * r["TH"] >= s * s * (LH + 1)
        magic = ((1 << 20) + LH) // (LH + 1)
        for vy in range(r["tiles_y"] * r["TH"] + r["PH"]):      # every virtual row a tile's patch can name
            assert (vy * magic) >> 20 == vy // (LH + 1), (vy, LH)
    else:
        assert r["tiles_x"] * r["TW"] >= OW > (r["tiles_x"] - 1) * r["TW"] and r["tiles_y"] * r["TH"] >= OH > (r["tiles_y"] - 1) * r["TH"]
    if pool:
        # a wave's fragments must hold both rows of a pooled pair: the tile rule of launch_conv_el
        assert r["TH"] % 2 == 0 and r["TW"] % 16 == 0 and (8 if bn == 128 else 4) % (2 * (r["TW"] // 16)) == 0
    tiles = N * r["tiles_x"] * r["tiles_y"]
    if r["persistent"]:
        assert r["grid"] == tiles and r["ntiles_n"] == 1         # dry run: the tile count; the launch caps it
    else:
        assert r["grid"] == tiles * r["ntiles_n"]


@st.composite
def _shape(draw):
    KH = draw(st.integers(1, 7))
    KW = KH if draw(st.integers(0, 3)) else draw(st.integers(1, 7))
    dil = draw(st.sampled_from([1, 1, 1, 2, 2, 3, 4, 5, 6, 6, 7, 8, 9]))
    pad = draw(st.sampled_from([0, 1, dil, dil, draw(st.integers(0, 8))]))
    pad = min(pad, 8)
    pool = draw(st.sampled_from([0, 0, 1, 2]))
    f32 = 0 if pool else draw(st.integers(0, 1))
    return (draw(st.integers(1, 3)), draw(st.integers(1, 80)), draw(st.integers(1, 80)), draw(st.sampled_from([32, 64, 96, 128, 160, 256])),
            draw(st.integers(1, 300)), KH, KW, pad, dil, pool, f32, draw(st.integers(0, 1)) if pool else 0)


_seen = {"accepted": 0, "refused": 0, "ids": set()}


@settings(max_examples=2400, **SETTINGS)
@given(a=_shape())
def _sweep(lib, a):
    N, H, W, Cin, Cout, KH, KW, pad, dil, pool, f32, full = a
    c = cc._c("sweep", "sweep", N, H, W, Cin, Cout, KH, KW, pad, dil, {}, "", out_f32=f32, pool_mode=pool, store_full=full)
    routes = [cc.dry_route(lib, c, el) for el in (0, 1)]
    assert {k: v for k, v in routes[0][1].items() if k != "el"} == {k: v for k, v in routes[1][1].items() if k != "el"}    # the element type picks no route
    rc, r = routes[0]
    if rc != 0:
        assert rc == -2 and r["id"] == "NONE" and r["status"] != 0
        _seen["refused"] += 1
        return
    _seen["accepted"] += 1
    _seen["ids"].add(r["id"])
    _invariants(a, r)


def test_invariants_of_accepted_shapes(lib):
    _seen.update(accepted=0, refused=0, ids=set())
    _sweep(lib=lib)
    print(f"sweep: {_seen['accepted']} accepted, {_seen['refused']} refused, ids {sorted(_seen['ids'])}")
    # not vacuous: most examples are accepted, a fair share refused, and the sweep alone reaches every instantiation of the generic kernel
    assert _seen["accepted"] >= 1200 and _seen["refused"] >= 50, _seen
    assert {i for i in _seen["ids"] if i.startswith("GEN")} == {f"GEN{bn}_P{p}" for bn in (64, 128) for p in (4, 8, 16)}, _seen["ids"]


# ---------------------------------------------------------------------------------------------------- references and planted defects
def _refs(c, el):
    x, w, b = cc.inputs(c, el)
    return x, w, b, cc.reference(c, x, w, b)


@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("name", [c.name for c in cc.CASES if c.name != "resw_persistent"] + ["resw_persistent"])
def test_reference_alone_stays_inside_the_rule(name, el):
    """torch's fp32 convolution, rounded to the output type, stands in for the kernel: with ref_q = ref_nq = the fp64 convolution of the same
    rounded operands, E = 0 and the 1e-3 cap it must pass -- the inputs leave the rule's whole budget to the kernel"""
    c = cc.BY_NAME[name]
    x, w, b, (full, pooled) = _refs(c, el)
    sf, sp = cc.reference(c, x, w, b, dt=torch.float32)
    eo = cc.el_out(c, el)
    want_full, want_pool = cc.outputs_checked(c)
    if want_full:
        got = R.round_out(sf.double(), eo)
        if c.exact:
            assert torch.equal(got, full), "the exact row's operands must make fp32 accumulation exact"
        R.check(got, full, full, 0.0, eo, f"{name} {el} stand-in", cap=1e-3)
    if want_pool:
        R.check(R.round_out(sp.double(), el), pooled, pooled, 0.0, el, f"{name} {el} stand-in pooled", cap=1e-3)


DEFECTS = [
    # defect, row, which output shows it
    ("dil1", "g_dil2_pad1", "full"),
    ("pad_off", "g_1x1_pad1", "full"),
    ("last_tap", "g_1x3", "full"),
    ("chunk_reuse", "g_3x3_valid", "full"),
    ("pool_off", "g_1x1_pool", "pooled"),
    ("no_relu_in", "g_relu_in", "full"),
    ("stale_part", "g_3x3_valid", "full"),
]


@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("defect,name,which", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_fails_the_rule(lib, defect, name, which, el):
    c = cc.BY_NAME[name]
    x, w, b, (full, pooled) = _refs(c, el)
    _, r = cc.dry_route(lib, c, ELS[el])
    geom = (r["TH"], r["TW"], r["PH"], r["PW"])
    if defect == "stale_part":
        assert r["PH"] * r["PW"] > 256 and c.Cin >= 64            # there ARE slots 256.. and a previous chunk
    # the tap-by-tap convolution is the operation when nothing is planted ...
    if defect != "pool_off":
        clean = R.nhwc(cc.conv_taps(c, x, w, b, torch.float64, None, geom))
        assert (clean - full).abs().max() <= 1e-12 * max(1.0, full.abs().max().item())
    # ... and misses the rule with the defect
    mf, mp = cc.reference(c, x, w, b, mut=defect, geom=geom)
    ref, mutated = (full, mf) if which == "full" else (pooled, mp)
    eo = cc.el_out(c, el) if which == "full" else el
    assert R.fails_allowance(R.round_out(mutated, eo), ref, ref, 0.0, eo)
    with pytest.raises(AssertionError):
        R.check(R.round_out(mutated, eo), ref, ref, 0.0, eo, f"{name} {el} {defect}", cap=1e-3)
