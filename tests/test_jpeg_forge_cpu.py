"""Baseline JPEG files no libjpeg encoder writes, without a GPU.  tests/jpeg_forge.py transcodes files Pillow wrote into other dialects of
the format; the coefficients do not change, so every forged file must decode to its source's pixels.
  list A  legal files: Pillow decodes them to the source's pixels, ``bbocr_host_jpeg_plan`` equals the restatement's parse field by field,
          the restatement's pixels equal Pillow's and the model of the device passes ends with status word 0;
  list B  files the plan refuses, each with its reason, in C and in the restatement; the invalid Huffman tables are the ones Pillow raises on;
  list C  bytes behind the last MCU of a restart segment: Pillow decodes them, the model's status word says what the device must say.
test_gpu_jpeg_forge.py runs the same lists on the device."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import jpeg_chroma_ref as K
import jpeg_entropy_ref as J
import jpeg_forge as F
import jpeg_progressive_ref as P
from test_jpeg_decode_cpu import c_plan, lib, picture, pillow_pixels, save  # noqa: F401  (lib: a fixture)

SIZES = [(19, 17), (47, 33), (56, 40)]                            # width x height: partial MCUs on both axes, and whole ones
KINDS = ["L", "420"]                                              # every variant; "444", "422", "440": the table and restart variants
CLASS_SIZE = (47, 33)
BIG = (200, 120)                                                  # the long scans: 16-bit codes and skewed tables on noise
LANES = 64                                                        # kernels.h JD_LANES


@functools.lru_cache(maxsize=None)
def source(kind, size, quality=90):
    """a file Pillow wrote (4:4:0: the transposition of one), noise"""
    w, h = size
    if kind == "L":
        return save(picture("noise", w, h, "L"), quality=quality)
    if kind == "440":
        return K.make_440(save(picture("noise", h, w, "RGB"), quality=quality, subsampling=1))
    return save(picture("noise", w, h, "RGB"), quality=quality, subsampling={"420": 2, "444": 0, "422": 1}[kind])


def _pair(dc, ac):
    """one table pair for every component"""
    return lambda nc: dict(tables={(0, 0): dc, (1, 0): ac}, select=[(0, 0)] * nc)


def _by_frequency(symbols):
    return lambda f: F.unary(sorted(symbols, key=lambda s: (-f.get(s, 0), s)))


def table_variants(nc):
    std = {(0, 0): F.standard(0), (1, 0): F.standard(1), (0, 1): F.standard(0, True), (1, 1): F.standard(1, True)}
    swapped = {(0, 1): F.standard(0), (1, 1): F.standard(1), (0, 0): F.standard(0, True), (1, 0): F.standard(1, True)}
    both = [(0, 0), (1, 0)] + ([(0, 1), (1, 1)] if nc == 3 else [])
    out = {
        "ids-swapped": dict(tables={k: v for k, v in swapped.items() if nc == 3 or k[1] == 1}, select=[(1, 1), (0, 0), (0, 0)][:nc]),
        "ids-crossed": dict(tables={k: v for k, v in {(0, 0): std[(0, 0)], (1, 1): std[(1, 0)], (0, 1): std[(0, 1)], (1, 0): std[(1, 1)]}.items()
                                    if nc == 3 or k in ((0, 0), (1, 1))}, select=[(0, 1), (1, 0), (1, 0)][:nc]),
        "one-pair": _pair(F.standard(0), F.standard(1))(nc),
        "one-dht": dict(dht="one"),
        "one-dht-before-sof": dict(dht="one", dht_where="before"),
        "twice-after-sof": dict(dht_twice="after"),
        "twice-before-sof": dict(dht_twice="before"),
        "flat-4-8": _pair(F.flat(4, F.DC_SYMBOLS), F.flat(8, F.AC_SYMBOLS))(nc),
        "flat-10": dict(_pair(F.flat(10, F.DC_SYMBOLS), F.flat(10, F.AC_SYMBOLS))(nc), dht="one"),
        "flat-16": _pair(F.flat(16, F.DC_SYMBOLS), F.flat(16, F.AC_SYMBOLS))(nc),
        "optimal": dict(tables={k: F.optimal for k in both}),
        "skewed": _pair(lambda f: F.skewed(f, F.standard(0)[0], F.DC_SYMBOLS), lambda f: F.skewed(f, F.standard(1)[0], F.AC_SYMBOLS))(nc),
        "unary": _pair(_by_frequency(F.DC_SYMBOLS), _by_frequency(F.AC_SYMBOLS))(nc),
    }
    return out


def odd_interval(mcux, nmcu):
    """the smallest interval above 1 that divides neither the MCUs of a row nor those of the file"""
    return next(v for v in range(2, nmcu + 2) if mcux % v and nmcu % v)


def restart_variants(mcux, nmcu):
    return {
        "ri-1": dict(dri=1),
        "ri-row": dict(dri=mcux),
        "ri-odd": dict(dri=odd_interval(mcux, nmcu)),
        "ri-nmcu": dict(dri=nmcu),
        "ri-more": dict(dri=nmcu + 7),
        "ri-65535": dict(dri=65535),
        "ri-0": dict(dri=[0]),
        "ri-3-then-0": dict(dri=[3, 0]),
        "ri-twice": dict(dri=[1, mcux]),
        "fill-rst-eoi": dict(dri=mcux, fill={F.RST: 2, F.EOI: 3}),
        "fill-rst-ri-1": dict(dri=1, fill={F.RST: 1}),
    }


def other_variants(nc):
    out = {
        "fill-eoi": dict(fill={F.EOI: 2}),
        "fill-dqt": dict(fill={0xDB: 3}),
        "fill-every-header": dict(fill={m: 1 for m in (0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA)}, dri=[0]),
        "dqt-ids-2-3": dict(dqt_ids=[2, 3, 3][:nc]),
        "dqt-one-segment": dict(dqt="one", dqt_ids=[3, 0, 0][:nc]),
        "dqt-redefined": dict(dqt_twice=True),
        "comp-ids-0-1-2": dict(comp_ids=[0, 1, 2][:nc]),
        "comp-ids-10-20-30": dict(comp_ids=[10, 20, 30][:nc]),
        "max-app-and-com": dict(extra=[(0xDB, 0xFE, b"c" * 65533), (0xC0, 0xED, b"p" * 65533), (0xDA, 0xE2, bytes(65533))], trailer=b"behind\xff\xd9"),
    }
    if nc == 3:
        out["comp-ids-rgb-under-jfif"] = dict(comp_ids=[82, 71, 66])      # libjpeg lets JFIF win: YCbCr
        out["adobe-transform-1"] = dict(marking="adobe1")
    return out


def _geometry(data):
    plan = K.parse(data)
    return plan["components"], plan["mcu_cols"], plan["mcu_cols"] * plan["mcu_rows"]


@functools.lru_cache(maxsize=None)
def list_a(kind, size):
    """[(name, forged file)] of one source; its pixels: ``pillow_pixels(source(kind, size))``"""
    src = source(kind, size)
    nc, mcux, nmcu = _geometry(src)
    variants = dict(table_variants(nc), **restart_variants(mcux, nmcu))
    if kind in KINDS:
        variants.update(other_variants(nc))
    out = [("%s-%dx%d-%s" % (kind, size[0], size[1], name), F.forge(src, **kw)) for name, kw in variants.items()]
    if kind == "420":                                             # one quantisation table for all components: a source whose tables are equal
        out.append(("%s-%dx%d-dqt-shared" % ((kind,) + size), F.forge(source(kind, size, 100), dqt_ids=[0, 0, 0])))
    return out


def pixels_of(name, kind, size):
    return pillow_pixels(source(kind, size, 100) if name.endswith("dqt-shared") else source(kind, size))


@functools.lru_cache(maxsize=None)
def big():
    """[(name, forged file)]: the long scans, 200 x 120 noise with 16-bit codes and with skewed tables, grey and 4:2:0"""
    out = []
    for kind in KINDS:
        nc = 1 if kind == "L" else 3
        for name in ("flat-16", "skewed"):
            out.append(("%s-big-%s" % (kind, name), kind, F.forge(source(kind, BIG, 95), **table_variants(nc)[name])))
    return out


def sources_a():
    return [(k, s) for s in SIZES for k in KINDS] + [(k, CLASS_SIZE) for k in ("444", "422", "440")]


def model(data, plan, S=1024):
    """(coef, states, cross-group passes, status word) of the device model over the plan's own MCU layout"""
    return J.device_model(data, plan, S, group=LANES, status=True, stream=K.Stream(data, plan))


def assert_plans_agree(want, got, name):
    cls = want["chroma"]
    assert (got.supported, got.reason, got.chroma) == (0 if cls else 1, J.SAMPLING if cls else J.OK, cls), name
    assert (got.width, got.height, got.components) == (want["width"], want["height"], want["components"]), name
    assert [tuple(s) for s in got.sampling][:got.components] == want["sampling"], name
    assert (got.restart_interval, got.mcu_cols, got.mcu_rows, got.segments) == (want["restart_interval"], want["mcu_cols"], want["mcu_rows"],
                                                                               len(want["segments"])), name
    assert (got.scan_offset, got.scan_bytes) == (want["scan_offset"], want["scan_bytes"]), name


# ------------------------------------------------------------------------------------------------ list A
@pytest.mark.parametrize("kind,size", sources_a())
def test_list_a_decodes_everywhere(lib, kind, size):
    files = list_a(kind, size)
    assert len(files) == (24 if kind not in KINDS else 33 if kind == "L" else 36)
    for name, data in files:
        want = pixels_of(name, kind, size)
        assert want.shape[:2] == (size[1], size[0])
        assert np.array_equal(pillow_pixels(data), want), name                       # Pillow: the syntax is legal and means the same
        plan = K.parse(data)
        assert plan["supported"] or plan["chroma"], (name, plan)
        assert (plan["chroma"] != 0) == (kind not in KINDS), name
        assert_plans_agree(plan, c_plan(lib, data), name)
        coef, _ = K.decode_coefficients(data, plan)
        assert np.array_equal(K.planes_to_pixels(K.component_planes(coef, plan), plan), want), name
        m_coef, _, _, word = model(data, plan)
        assert word == 0 and np.array_equal(m_coef, coef), (name, word)
        if size == SIZES[0]:                                      # and cut every 32 bits, the shortest the stage entry point takes
            assert model(data, plan, 32)[3] == 0, name


def test_the_long_scans(lib):
    for name, kind, data in big():
        want = pillow_pixels(source(kind, BIG, 95))
        assert np.array_equal(pillow_pixels(data), want), name
        plan = K.parse(data)
        assert_plans_agree(plan, c_plan(lib, data), name)
        assert np.array_equal(K.decode_pixels(data, plan), want), name
        for S in (1024, 32):
            if S == 32 and kind != "L":
                # one table pair for three components: a lane that enters in the wrong block of the MCU never finds the right one by
                # itself, so every one of the model's ~320 cross-group passes changes a state -- half a minute here; the device test
                # holds these files' stages against the sequential decoder at S = 32 all the same
                continue
            coef, states = K.decode_coefficients(data, plan, S)
            m_coef, m_states, passes, word = model(data, plan, S)
            assert word == 0 and np.array_equal(m_coef, coef) and np.array_equal(m_states, states), (name, S)
            assert len(states) > 2 * LANES and (passes > 1 or S != 32), (name, S, len(states), passes)


def _code_lengths(data):
    """per (class, id) the selected tables' {symbol: length} and the symbol frequencies of the file"""
    plan = K.parse(data)
    freq = F.frequencies(data)
    return {k: ({s: l for s, (_, l) in F.codes_of(plan["huff"][k]).items()}, f) for k, f in freq.items()}


def test_the_matrix_is_not_degenerate():
    files = [(n, d) for k, s in sources_a() for n, d in list_a(k, s)] + [(n, d) for n, _, d in big()]
    assert len({d for _, d in files}) == len(files)                                  # no two variants are the same file
    longer_than_9 = most_frequent_ac_is_16 = 0
    for name, data in files:
        if not any(t in name for t in ("flat-10", "flat-16", "skewed")):
            continue
        tabs = _code_lengths(data)
        longer_than_9 += all(lengths[s] > 9 for lengths, f in tabs.values() for s in f)          # the look-ahead never hits
        most_frequent_ac_is_16 += any(k[0] == 1 and lengths[max(f, key=f.get)] == 16 for k, (lengths, f) in tabs.items())
    assert longer_than_9 >= 2 * len(sources_a()) and most_frequent_ac_is_16 >= 2 * len(sources_a())
    plans = {n: K.parse(d) for n, d in files}
    assert sum(len(p["segments"]) > 8 for p in plans.values()) >= 8                  # RSTn wraps past 7
    assert any(len(p["segments"]) > 8 and p["restart_interval"] == 1 for p in plans.values())
    for kind, size in sources_a():                                                   # the restart variants are what their names say
        _, mcux, nmcu = _geometry(source(kind, size))
        by = {n.split("x", 1)[1].split("-", 1)[1]: plans[n] for n, _ in list_a(kind, size)}
        assert [by[k]["restart_interval"] for k in ("ri-1", "ri-row", "ri-nmcu", "ri-more", "ri-65535", "ri-0", "ri-3-then-0", "ri-twice")] == \
            [1, mcux, nmcu, nmcu + 7, 65535, 0, 0, mcux], (kind, size)
        odd = by["ri-odd"]["restart_interval"]
        assert mcux % odd and nmcu % odd and 1 < odd < nmcu, (kind, size)
        assert [len(by[k]["segments"]) for k in ("ri-1", "ri-nmcu", "ri-more", "ri-0")] == [nmcu, 1, 1, 1]
    for name, data in files:                                                         # fill bytes stand where the names say
        if "fill-rst-eoi" in name:
            assert b"\xff\xff\xff\xd0" in data and data.endswith(b"\xff\xff\xff\xff\xd9"), name
        if "fill-rst-ri-1" in name:
            assert b"\xff\xff\xd0" in data and b"\xff\xff\xff\xd0" not in data, name


# ------------------------------------------------------------------------------------------------ list B
def list_b():
    """[(name, file, reason, Pillow must raise)]"""
    out = []
    for kind in KINDS:
        src = source(kind, (47, 33))
        nc = 1 if kind == "L" else 3
        for name, (cls, table) in F.invalid_tables().items():
            out.append(("%s-%s" % (kind, name), F.forge(src, dht_override={(cls, 0): table}), J.TABLES, True))
        out.append((kind + "-dht-id-2", F.forge(src, tables={(0, 2): F.standard(0), (1, 2): F.standard(1)}, select=[(2, 2)] * nc), J.TABLES, False))
        out.append((kind + "-dqt-16-bit", F.forge(src, dqt16=True), J.PRECISION, False))
    src = source("420", (47, 33))
    out.append(("adobe-transform-0", F.forge(src, marking="adobe0"), J.COLORSPACE, False))
    out.append(("no-marking", F.forge(src, marking="none"), J.COLORSPACE, False))
    out.append(("sos-out-of-frame-order", F.forge(src, sos_order=[1, 0, 2]), J.MULTISCAN, False))
    return out


def pillow_raises(data):
    from PIL import Image

    try:
        Image.open(io.BytesIO(data)).load()
    except (OSError, SyntaxError):
        return True
    return False


def test_list_b_is_refused_with_its_reason(lib):
    cases = list_b()
    assert len(cases) == 2 * (len(F.invalid_tables()) + 2) + 3
    for name, data, reason, must_raise in cases:
        assert J.parse(data) == dict(supported=False, reason=reason), name
        got = c_plan(lib, data)
        assert (got.supported, got.reason, got.chroma) == (0, reason, 0), name
        if must_raise:
            assert pillow_raises(data), name                      # the set refused is the set libjpeg refuses
    # an invalid table the scan does not select is no reason: libjpeg derives the tables a scan names
    src = source("420", (47, 33))
    for name, (cls, table) in F.invalid_tables().items():
        spare = bytes([(cls << 4) | 1]) + bytes(table[0]) + bytes(table[1])
        data = F.forge(src, extra=[(0xDA, 0xC4, spare)], **_pair(F.standard(0), F.standard(1))(3))
        assert not pillow_raises(data) and np.array_equal(pillow_pixels(data), pillow_pixels(src)), name
        assert J.parse(data)["supported"] and c_plan(lib, data).supported == 1, name


def test_tables_at_the_edge_of_the_rule_are_taken(lib):
    """the longest legal codes beside the refused ones: 15 codes of 4 bits, 255 of 8 bits (all but the all-ones code), and a DC table
    that names category 15"""
    src = source("L", (47, 33))
    want = pillow_pixels(src)
    ac255 = F.AC_SYMBOLS + [s for s in range(256) if s not in F.AC_SYMBOLS][:255 - len(F.AC_SYMBOLS)]
    for dc, ac in ((F.flat(4, list(range(15))), F.flat(8, ac255)), (F.flat(4, F.DC_SYMBOLS + [15]), F.standard(1))):
        data = F.forge(src, **_pair(dc, ac)(1))
        assert np.array_equal(pillow_pixels(data), want)
        plan = J.parse(data)
        assert plan["supported"] and c_plan(lib, data).supported == 1
        assert np.array_equal(J.decode_pixels(data, plan), want) and model(data, K.parse(data))[3] == 0


def test_progressive_file_with_an_all_ones_table_is_refused(lib):
    from bb_ocr_amd import _lib

    good = save(picture("noise", 47, 33, "RGB"), quality=90, progressive=True)
    table = F.invalid_tables()["dc-sixteen-4-bit-codes"][1]
    bad = F.replace_dht(good, 0, 0, table)
    assert pillow_raises(bad) and not pillow_raises(good)
    for data, reason in ((good, P.OK), (bad, P.TABLES)):
        p = _lib.bbocr_jpeg_progressive_plan()
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        assert lib.bbocr_host_jpeg_progressive_plan(buf, len(data), C.byref(p)) == 0
        assert (p.supported, p.reason) == (int(reason == P.OK), reason)
        want = P.parse(data)
        assert (want["supported"], want["reason"]) == (reason == P.OK, reason)


# ------------------------------------------------------------------------------------------------ list C
PADS = {"1-zero": bytes(1), "4-zeros": bytes(4), "64-zeros": bytes(64), "64-pattern": bytes((37 * k + 11) % 251 for k in range(64))}


@functools.lru_cache(maxsize=None)
def list_c():
    """[(name, kind, size, forged file)]: bytes behind the last MCU of the last segment, and of a middle segment of a restart file"""
    out = []
    for kind, size in (("L", (47, 33)), ("420", (56, 40)), ("422", CLASS_SIZE)):
        src = source(kind, size)
        _, mcux, _ = _geometry(src)
        for pname, pad in PADS.items():
            out.append(("%s-last-%s" % (kind, pname), kind, size, F.forge(src, pad=(-1, pad))))
            out.append(("%s-middle-%s" % (kind, pname), kind, size, F.forge(src, dri=mcux, pad=(1, pad))))
    return out


def test_list_c_pillow_decodes_and_the_model_names_the_status(lib):
    words = {}
    for name, kind, size, data in list_c():
        assert np.array_equal(pillow_pixels(data), pillow_pixels(source(kind, size))), name
        plan = K.parse(data)
        assert_plans_agree(plan, c_plan(lib, data), name)
        assert len(plan["segments"]) == (1 if "-last-" in name else plan["mcu_rows"]), name
        coef, _, _, word = model(data, plan)
        words[name] = word
        assert word in (0, J.ERR_COUNT), (name, word)             # never a missing code, never lost synchronisation: only the count
        if word == 0:                                             # the coefficients do not depend on the restart interval
            assert np.array_equal(coef, K.decode_coefficients(source(kind, size), K.parse(source(kind, size)))[0]), name
    assert 0 in words.values() and J.ERR_COUNT in words.values(), words              # the list spans the rule
