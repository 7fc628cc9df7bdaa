"""The device TIFF decoder without a card: the restatement (tests/tiff_decode_ref.py) against ``reader.decode_file`` (Pillow plus the stated
gray rule) over Pillow's own files, the hand-built files and the hand-written code streams; ``bbocr_host_tiff_plan`` through ctypes against
the restatement's walk -- every field, every refusal reason --; the damage list; the ABI exports."""
import ctypes as C
import warnings

import numpy as np
import pytest

import tiff_decode_ref as R


@pytest.fixture(scope="module")
def matrix():
    return R.matrix()


def host_decode(f):
    from bb_ocr_amd.reader import decode_file

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return decode_file(f)


def lib_plan(f):
    from bb_ocr_amd.reader import tiff_plan

    p = tiff_plan(f)
    return {k: int(getattr(p, k)) for k in R.PLAN_FIELDS}


def test_matrix_covers_every_combination(matrix):
    names = [n for n, _ in matrix]
    assert len(names) == len(set(names)) == len(list(R.combos())) * len(R.SHAPES) == 28 * 4
    for mode, comp, pred in R.combos():
        mine = [n for n in names if n.startswith("%s-%s-p%d-" % (mode, comp, pred))]
        assert {n.rsplit("-", 1)[1] for n in mine} == set(R.STRIPPINGS), (mode, comp, pred)
    # Pillow did what the names say: the codec, the predictor, and one / a few / one-row strips
    comp_of = {"raw": (1,), "packbits": (32773,), "tiff_lzw": (5,), "tiff_adobe_deflate": (8,)}
    for name, f in matrix:
        mode, comp, pred, shape, strip = name.split("-")
        pl = R.plan(f)
        h = pl["height"]
        assert pl["supported"] and pl["compression"] in comp_of[comp] and pl["predictor"] == int(pred[1]), name
        # (Pillow's uncompressed writer always writes one strip: the hand-built files hold the raw files of several)
        one = strip == "one" or h == 1 or comp == "raw"
        assert (pl["strips"] == 1) if one else (pl["strips"] == h if strip == "many" else 1 < pl["strips"] <= 4), (name, pl)
    few = [R.plan(f) for n, f in matrix if n.endswith("few")]
    assert any(p["height"] % p["rows_per_strip"] for p in few)                     # a last strip shorter than the others


def test_restatement_equals_decode_file(matrix):
    for name, f in matrix + R.handbuilt():
        d = R.decode(f)
        rgb, gray = host_decode(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        pl = d["plan"]
        assert len(d["stage0"]) == len(d["stage1"]) == pl["height"] * pl["row_bytes"], name
        assert (d["stage0"] == d["stage1"]) == (pl["predictor"] == 1) or pl["width"] == 1, name


def test_handbuilt_files_are_what_they_claim():
    plans = {n: R.plan(f) for n, f in R.handbuilt()}
    assert all(p["supported"] for p in plans.values())
    assert plans["mm_L_lzw"]["big_endian"] == 1 and plans["phot0_1bit"]["bits"] == 1 and plans["phot0_8bit"]["photometric"] == 0
    assert plans["rows_absent"]["strips"] == 1 == plans["rows_max"]["strips"] and plans["one_row_strips_packbits"]["strips"] == 23
    assert plans["rgbx_extra0_lzw_p2"]["extra_sample"] == 0 and plans["rgba_extra2_raw"]["extra_sample"] == 2


def test_handwritten_streams_agree_with_pillow():
    """a stream Pillow accepts decodes to the same bytes; one it refuses would belong on the damage list -- none does"""
    for (name, comp, strip, (w, h)), (_, f) in zip(R.handwritten(), R.handwritten_files()):
        want = R.decode_strip(comp, strip, w * h)
        assert R.decode(f)["gray"].tobytes() == want, name
        rgb, gray = host_decode(f)
        assert gray.tobytes() == want, name
    # the streams hold what their names say
    by = {n: s for n, _, s, _ in R.handwritten()}
    codes = []
    R.unlzw(by["lzw_table_fills_and_clears"], 7000, codes)
    clears = [i for i, (c, _) in enumerate(codes) if c == 256]
    # 3836 codes between the Clears: the encoder defined entries 258 .. 4093, one per code, and the decoder reads the Clear with 12 bits
    assert clears[:2] == [0, 4094 - 258 + 1] and codes[clears[1]][1] == 12 and {w for _, w in codes} == {9, 10, 11, 12}
    for edge in (511, 1023, 2047):
        codes = []
        R.unlzw(by["lzw_width_edge_%d" % edge], len(R.unlzw_all(by["lzw_width_edge_%d" % edge])), codes)
        tail = codes[-4:]                                                          # newest entry | its successor, KwKwK, a literal: old | new width
        assert [c for c, _ in tail] == [edge - 2, edge - 1, edge + 1, 65] and tail[0][1] + 1 == tail[1][1] == tail[2][1], (edge, tail)


def test_lzw_encoder_round_trip_and_libtiff():
    rng = np.random.default_rng(0)
    for n, levels in ((1, 256), (300, 2), (5000, 4), (9000, 256)):
        data = rng.integers(0, levels, n, dtype=np.uint8).tobytes()
        assert R.unlzw(R.lzw_encode(data), n) == data and R.unpackbits(R.packbits_encode(data), n) == data
        assert host_decode(R.wrap_strip(5, R.lzw_encode(data), n if n < 300 else 100, 1 if n < 300 else n // 100))[1].tobytes() == data


def test_damage_list():
    for name, f in R.damaged():
        assert R.plan(f)["supported"], name
        with pytest.raises(R.Damaged):
            R.decode(f)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_equals_the_walk_field_by_field(matrix):
    files = matrix + R.handbuilt() + R.handwritten_files() + R.damaged()
    for name, f in files:
        want = R.plan(f)
        assert want["supported"] == 1 and lib_plan(f) == want, name


def test_plan_refuses_reason_by_reason():
    seen = set()
    for name, f, reason in R.refusals():
        want = R.plan(f)
        assert want["reason"] == reason and not want["supported"], (name, R.REASONS[want["reason"]])
        assert lib_plan(f) == want, name
        seen.add(reason)
    assert seen == set(range(1, len(R.REASONS)))                                   # every reason of bbocr.h on a file of its own


def test_refused_files_keep_the_host_path():
    from bb_ocr_amd.reader import tiff_page

    assert all(tiff_page(f) is None for _, f, _ in R.refusals())
    assert tiff_page(R.handbuilt()[0][1]).shape == (23, 37, 3)
    assert tiff_page(b"") is None and tiff_page("/no/such/file.tif") is None


def test_reason_constants_match_the_header():
    import os
    import re

    from bb_ocr_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bbocr.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"BBOCR_TIFF_(\w+) = (\d+)", text)}
    assert header == {n: i for i, n in enumerate(R.REASONS)} == {n: getattr(_lib, "TIFF_" + n) for n in R.REASONS}


def test_abi_exports():
    from bb_ocr_amd import _lib

    lib = _lib.load()
    for name in ("bbocr_host_tiff_plan", "bbocr_tiff_decode", "bbocr_op_tiff_decode_stage"):
        assert getattr(lib, name) is not None
    plan = _lib.bbocr_tiff_plan()
    assert lib.bbocr_host_tiff_plan(None, 0, C.byref(plan)) == -1 and lib.bbocr_host_tiff_plan(b"II*\0", 4, None) == -1      # BBOCR_ERR_ARG


def test_option_is_off_by_default(monkeypatch):
    from bb_ocr_amd import reader as M

    monkeypatch.delenv("BBOCR_TIFF_DECODE", raising=False)
    assert M.tiff_decode_enabled() is False and M.tiff_decode_enabled(True) is True
    monkeypatch.setenv("BBOCR_TIFF_DECODE", "1")
    assert M.tiff_decode_enabled() is True and M.tiff_decode_enabled(False) is False
