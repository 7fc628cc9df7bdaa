"""The device BMP decoder without a card: the restatement (tests/bmp_decode_ref.py) against ``reader.decode_file`` (Pillow plus the stated
gray rule) over Pillow's own files and the hand-built ones -- every header size, depth, mask layout and direction, the sub-byte widths --;
``bbocr_host_bmp_plan`` through ctypes against the restatement's walk -- every field, every refusal reason --; the classes that are
stricter than Pillow; the ABI exports."""
import ctypes as C
import io
import warnings

import numpy as np
import pytest

import bmp_decode_ref as R


@pytest.fixture(scope="module")
def good():
    return R.matrix() + R.handbuilt()


def host_decode(f):
    from bb_ocr_amd.reader import decode_file

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return decode_file(f)


def lib_plan(f):
    from bb_ocr_amd.reader import bmp_plan

    p = bmp_plan(f)
    return {k: int(getattr(p, k)) for k in R.PLAN_FIELDS}


def test_restatement_equals_decode_file(good):
    from PIL import Image

    seen, modes = set(), set()
    for name, f in good:
        d = R.decode(f)
        rgb, gray = host_decode(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        pl = d["plan"]
        mode = Image.open(io.BytesIO(f)).mode
        assert mode == {R.MODE_P: "P", R.MODE_1: "1", R.MODE_L: "L"}.get(pl["mode"], mode) and (pl["mode"] != R.MODE_RGB or mode in ("RGB", "RGBA")), name
        seen.add((pl["header_size"], pl["bits"], pl["top_down"]))
        modes.add(mode)
    assert modes == {"1", "L", "P", "RGB", "RGBA"}
    assert seen >= {(hs, bits, top) for hs in (12, 40, 52, 56, 64, 108, 124) for bits in (1, 4, 8, 16, 24, 32) for top in (0, 1) if hs != 12 or not top}
    widths = {(R.plan(f)["width"], R.plan(f)["bits"]) for _, f in good}
    assert widths >= {(w, bits) for w in (1, 7, 8, 9, 31, 32, 33) for bits in (1, 4)}
    layouts = {(R.plan(f)["r_at"], R.plan(f)["g_at"], R.plan(f)["b_at"]) for n, f in good if n.startswith("masks32_")}
    assert layouts == set(R.MASKS32.values()) and len([n for n, _ in good if n.startswith("masks32_")]) == 3 * 4 + 2 * 4


def test_every_16_bit_value_expands_as_pillow_does(good):
    by = dict(good)
    for name in ("all_555", "all_565"):
        d = R.decode(by[name])
        assert np.array_equal(d["rgb"], host_decode(by[name])[0]) and d["rgb"].shape == (256, 256, 3)
    assert R.decode(by["all_565"])["rgb"].reshape(-1, 3)[0x07E0].tolist() == [0, 255, 0]


def test_plan_equals_the_walk_field_by_field(good):
    for name, f in good:
        want = R.plan(f)
        assert want["supported"] == 1 and lib_plan(f) == want, name
    by = {n: R.plan(f) for n, f in good}
    assert by["offset_at_the_table"]["data_offset"] == 54 + 1024 and by["offset_0"]["data_offset"] == 54 and by["offset_0_with_table"]["data_offset"] == 54 + 64
    assert by["gap_before_rows"]["data_offset"] == 64 and by["colors_field_0"]["colors"] == 16 and by["gray_ramp_8bit_16_entries"]["mode"] == R.MODE_L
    assert by["white_then_black"]["mode"] == R.MODE_P and by["w9_1bit_bw"]["mode"] == R.MODE_1 and by["h12_bottom_4"]["table_entry"] == 3


def test_plan_refuses_reason_by_reason():
    seen = set()
    for name, f, reason in R.refusals():
        want = R.plan(f)
        assert want["reason"] == reason and not want["supported"], (name, R.REASONS[want["reason"]])
        assert lib_plan(f) == want, name
        seen.add(reason)
    assert seen == set(range(1, len(R.REASONS)))                                   # every reason of bbocr.h on a file of its own


def test_stricter_than_pillow_classes_are_the_named_ones():
    """a refused file keeps the host path whatever Pillow makes of it.  The ones Pillow reads: a file short of less than a row, and the
    black-then-white tables on 4 or 8 bits, whose rows Pillow reads as 1-bit samples (the image is not the file's)"""
    accepted = set()
    for name, f, reason in R.refusals():
        try:
            host_decode(f)
            accepted.add(name)
        except Exception:
            pass
    assert accepted == {"rows_cut", "black_white_8bit", "black_white_4bit"}
    for name, f, reason in R.refusals():                                           # a colour table above 256 entries: Pillow opens the file ...
        if name.startswith("table_of_3") or name.startswith("table_of_257") or name.startswith("table_of_65536"):
            from PIL import Image

            assert reason == R.PALETTE and Image.open(io.BytesIO(f)).mode == "P", name
            with pytest.raises(ValueError, match="invalid palette size"):          # ... and raises when it loads it
                host_decode(f)
    by = dict(R.handbuilt())
    assert R.plan(by["gray_ramp_8bit_300_entries"])["mode"] == R.MODE_L and R.plan(by["h40_bottom_8"])["colors"] == 256      # what Pillow reads stays
    with pytest.raises(Exception):                                                 # a whole row missing: Pillow raises
        host_decode(R.bmp_file(13, 7, 24, seed=1, cut=40))


def test_refused_files_keep_the_host_path():
    from bb_ocr_amd.reader import bmp_page

    assert all(bmp_page(f) is None for _, f, _ in R.refusals())
    assert bmp_page(R.handbuilt()[0][1]).shape == (7, 13, 3)
    assert bmp_page(b"") is None and bmp_page("/no/such/file.bmp") is None


def test_reason_constants_match_the_header():
    import os
    import re

    from bb_ocr_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bbocr.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"BBOCR_BMP_(\w+) = (\d+)", text)}
    assert header == {n: i for i, n in enumerate(R.REASONS)} == {n: getattr(_lib, "BMP_" + n) for n in R.REASONS}


def test_abi_exports():
    from bb_ocr_amd import _lib

    lib = _lib.load()
    for name in ("bbocr_host_bmp_plan", "bbocr_bmp_decode"):
        assert getattr(lib, name) is not None
    plan = _lib.bbocr_bmp_plan()
    assert lib.bbocr_host_bmp_plan(None, 0, C.byref(plan)) == -1 and lib.bbocr_host_bmp_plan(b"BM", 2, None) == -1      # BBOCR_ERR_ARG


def test_option_is_off_by_default(monkeypatch):
    from bb_ocr_amd import reader as M

    monkeypatch.delenv("BBOCR_BMP_DECODE", raising=False)
    assert M.bmp_decode_enabled() is False and M.bmp_decode_enabled(True) is True
    monkeypatch.setenv("BBOCR_BMP_DECODE", "1")
    assert M.bmp_decode_enabled() is True and M.bmp_decode_enabled(False) is False
