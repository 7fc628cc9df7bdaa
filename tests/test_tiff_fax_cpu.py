"""The CCITT codec of the device TIFF decoder without a card: the restatement (tests/tiff_fax_ref.py) against ``reader.decode_file`` (Pillow
with libtiff) over Pillow's own files of all three schemes and over the module's hand-built files; the encoder's round trip and its streams
as Pillow reads them; ``bbocr_host_tiff_fax_plan`` through ctypes against the restatement's walk -- every field, every reason --;
``bbocr_host_tiff_plan`` unchanged on every fax file; the damage list; the constants and the ABI exports."""
import ctypes as C
import io
import os
import re
import warnings

import numpy as np
import pytest

import tiff_decode_ref as R
import tiff_fax_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_decode(f):
    from bb_ocr_amd.reader import decode_file

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return decode_file(f)


def lib_plans(f):
    from bb_ocr_amd.reader import tiff_fax_plan

    p, x = tiff_fax_plan(f)
    return {k: int(getattr(p, k)) for k in R.PLAN_FIELDS}, {k: int(getattr(x, k)) for k in F.FAX_FIELDS}


def lib_plain_plan(f):
    from bb_ocr_amd.reader import tiff_plan

    p = tiff_plan(f)
    return {k: int(getattr(p, k)) for k in R.PLAN_FIELDS}


@pytest.fixture(scope="module")
def pillow_files():
    """[(name, file)]: Pillow's own writer -- compression 2, 3 and 4, T4Options 0, 1, 4 and 5, fill order 1 and 2 -- on a small text page
    and on the 1280 x 960 page it cuts into three strips"""
    from PIL import Image

    out = []
    for tag, page in (("small", F.text_page(200, 60, 3)), ("page", F.text_page(1280, 960, 4))):
        for comp in ("tiff_ccitt", "group3", "group4"):
            for info in ({}, {292: 1}, {292: 4}, {292: 5}, {266: 2}):
                if comp == "group3" or 292 not in info:
                    b = io.BytesIO()
                    Image.fromarray(page == 0).save(b, "TIFF", compression=comp, tiffinfo=info)
                    out.append(("%s-%s-%s" % (tag, comp, info), b.getvalue()))
    return out


def test_tables_are_prefix_free_and_complete():
    for colour in (0, 1):
        words = F.code_set(colour)
        assert [r for _, r in words] == list(range(64)) + [64 * k for k in range(1, 41)]
        bits = [b for b, _ in words] + [F.EOL, F.EXT_1D]
        assert all(i == j or not b.startswith(a) for i, a in enumerate(bits) for j, b in enumerate(bits)), colour
        assert max(len(b) for b, _ in words) == (12 if colour == 0 else 13)
    modes = list(F.MODES.values()) + [F.EXT_2D]
    assert all(i == j or not b.startswith(a) for i, a in enumerate(modes) for j, b in enumerate(modes))


def test_pillows_own_files(pillow_files):
    seen = set()
    for name, f in pillow_files:
        pl, fax = F.fax_plan(f)
        assert pl["supported"] and fax["reason"] == F.FAX_OK, name
        seen.add((fax["scheme"], fax["t4_options"], fax["fill_order"]))
        d = F.decode(f)
        rgb, gray = host_decode(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        if name.startswith("page"):
            assert pl["strips"] == 3 and (pl["width"], pl["height"]) == (1280, 960), (name, pl)
    assert seen == {(2, 0, 1), (2, 0, 2), (3, 0, 1), (3, 1, 1), (3, 4, 1), (3, 5, 1), (3, 0, 2), (4, 0, 1), (4, 0, 2)}


def test_restatement_equals_decode_file_on_the_modules_files():
    files = F.designed_files() + F.handbuilt() + F.handwritten_files()
    plans = [F.fax_plan(f) for _, f in files]
    # photometric 0 and 1, both byte orders, one strip, one-row strips, a shorter last strip, K = 1, 2 and none, both fill orders
    assert {p["photometric"] for p, _ in plans} == {0, 1} and {p["big_endian"] for p, _ in plans} == {0, 1}
    assert any(p["strips"] == 1 for p, _ in plans) and any(p["rows_per_strip"] == 1 and p["height"] > 1 for p, _ in plans)
    assert any(p["height"] % p["rows_per_strip"] for p, _ in plans) and {x["fill_order"] for _, x in plans} == {1, 2}
    for name, f in files:
        d = F.decode(f)
        rgb, gray = host_decode(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        assert len(d["stage0"]) == d["plan"]["height"] * d["plan"]["row_bytes"], name
    for name, scheme, opt, bits, (w, h), rows in F.handwritten():
        assert F.decode_strip(F.to_bytes(bits), w, h, scheme, opt) == F.pack_rows(rows), name


def test_designed_pages_hold_every_code_and_mode():
    pages = dict(F.designed())
    for colour in (0, 1):
        codes = []
        a = pages["every_length"]
        F.decode_strip(F.encode_strip(a, 2), a.shape[1], a.shape[0], 2, codes=codes)
        assert {r for c, r in codes if c == colour} == set(range(64)) | {64 * k for k in range(1, 41)}
    modes = []
    a = pages["modes"]
    F.decode_strip(F.encode_strip(a, 4), a.shape[1], a.shape[0], 4, codes=modes)
    assert set(F.MODES) <= {m for m in modes if isinstance(m, str)}
    assert {name[1:] for name, _ in F.designed() if name[0] == "w"} == {"1", "7", "8", "9", "63", "64", "65", "1728", "2561"}
    assert pages["every_length"].shape[1] > 5120 and pages["dots_64x16"].shape == (16, 64) and pages["text_640x96"].shape == (96, 640)
    assert all(3 <= a.shape[0] <= 12 for n, a in F.designed() if n[0] == "w")


def test_encoder_round_trip_and_pillow_reads_it():
    rng = np.random.default_rng(0)
    for W, H in ((1, 5), (13, 9), (64, 7), (300, 11), (2700, 3)):
        a = (rng.integers(0, 8, (H, W)) == 0).astype(np.uint8)
        a[H // 2] = a[H // 2 - 1]
        want = F.pack_rows(a)
        for scheme, opt, k, tail, fo in ((2, 0, None, False, 1), (3, 0, None, True, 2), (3, 4, None, False, 1), (3, 1, 1, True, 1), (3, 1, 2, False, 2),
                                         (3, 5, None, True, 1), (4, 0, None, False, 1), (4, 0, None, True, 2)):
            strip = F.encode_strip(a, scheme, opt, k, tail, fo)
            assert F.decode_strip(strip, W, H, scheme, opt, fo) == want, (W, scheme, opt, k)
            f = F.fax_file(a, scheme, opt, strips=[strip], fill_order=fo if fo == 2 else None, photometric=0)
            gray = host_decode(f)[1]
            assert np.array_equal(gray, (1 - a) * 255), (W, scheme, opt, k, tail, fo)


def test_damage_list():
    for name, f in F.damaged():
        pl, fax = F.fax_plan(f)
        assert pl["supported"] and fax["scheme"] in (2, 3, 4), name
        with pytest.raises(F.Damaged):
            F.decode(f)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_equals_the_walk_field_by_field(pillow_files):
    files = F.designed_files() + F.handbuilt() + F.handwritten_files() + F.damaged() + pillow_files
    for name, f in files:
        pl, fax = F.fax_plan(f)
        assert pl["supported"] == 1 and pl["reason"] == R.OK and fax["scheme"] == pl["compression"] and lib_plans(f) == (pl, fax), name
    for name, f in R.matrix()[::5] + R.handbuilt() + R.damaged():          # files of the plain plan: the same plan, scheme 0
        pl, fax = F.fax_plan(f)
        assert pl == R.plan(f) and pl["supported"] and fax == dict(scheme=0, t4_options=0, fill_order=1, reason=F.FAX_OK), name
        assert lib_plans(f) == (pl, fax), name


def test_plan_refuses_reason_by_reason():
    seen = set()
    for name, f, plain, reason in F.fax_refusals():
        pl, fax = F.fax_plan(f)
        assert (pl["reason"], fax["reason"], pl["supported"]) == (plain, reason, 0), (name, R.REASONS[pl["reason"]], F.FAX_REASONS[fax["reason"]])
        assert lib_plans(f) == (pl, fax), name
        seen.add(reason)
    assert seen == set(range(1, len(F.FAX_REASONS)))                       # every reason of bbocr.h on a file of its own
    for name, f, reason in R.refusals():                                   # the plain plan's refusals: carried, but for CCITT and fill order
        pl, fax = F.fax_plan(f)
        assert lib_plans(f) == (pl, fax), name
        if reason not in (R.CCITT, R.FILL_ORDER):
            assert (pl, fax["reason"]) == (R.plan(f), F.FAX_PLAIN), name


def test_the_plain_plan_is_unchanged_on_every_fax_file(pillow_files):
    from bb_ocr_amd.reader import tiff_page

    files = F.designed_files()[::3] + F.handbuilt() + F.damaged() + pillow_files + [(n, f) for n, f, _, _ in F.fax_refusals()]
    for name, f in files:
        want = R.plan(f)
        assert lib_plain_plan(f) == want, name
        if F.fax_plan(f)[1]["scheme"]:
            assert want["reason"] == R.CCITT and tiff_page(f) is None, name
    page = tiff_page(F.handbuilt()[0][1], fax=True)
    assert page is not None and page.fax and page.shape == (12, 65, 3)
    lzw = tiff_page(R.handbuilt()[0][1], fax=True)
    assert lzw is not None and not lzw.fax and tiff_page(R.handbuilt()[0][1]).fax is False
    assert all(tiff_page(f, fax=True) is None for _, f, _, _ in F.fax_refusals())


def test_constants_match_the_header():
    from bb_ocr_amd import _lib

    text = open(os.path.join(ROOT, "include", "bbocr.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"BBOCR_FAX_(\w+) = (\d+)", text)}
    assert header == {n: i for i, n in enumerate(F.FAX_REASONS)} == {n: getattr(_lib, "FAX_" + n) for n in F.FAX_REASONS}
    limit = int(re.search(r"#define BBOCR_FAX_MAX_WIDTH (\d+)", text).group(1))
    assert limit == F.MAX_WIDTH == _lib.FAX_MAX_WIDTH and limit >= 10000
    codec = open(os.path.join(ROOT, "bb-ocr_amd", "csrc", "tiff_fax.h")).read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"TIFFC_ERR_FAX_(\w+) = 1 << (\d+)", codec)}
    assert sorted(bits.values()) == list(range(18, 18 + len(bits))) and len(bits) == 5      # they continue tiff_codecs.h's, which end at 1 << 17
    # the header's code words are the restatement's
    words = re.findall(r"\{0x([0-9A-F]+),(\d+)\}", codec)
    assert len(words) == 208
    for colour in (0, 1):
        mine = [(int(c, 16), int(n)) for c, n in words[104 * colour:104 * colour + 104]]
        assert mine == [(int(b, 2), len(b)) for b, _ in F.code_set(colour)], colour


def test_abi_exports():
    from bb_ocr_amd import _lib

    lib = _lib.load()
    for name in ("bbocr_host_tiff_fax_plan", "bbocr_tiff_decode_fax", "bbocr_op_tiff_fax_decode_stage"):
        assert getattr(lib, name) is not None
    plan, fax = _lib.bbocr_tiff_plan(), _lib.bbocr_tiff_fax()
    assert C.sizeof(fax) == 32
    assert lib.bbocr_host_tiff_fax_plan(None, 0, C.byref(plan), C.byref(fax)) == -1                                  # BBOCR_ERR_ARG
    assert lib.bbocr_host_tiff_fax_plan(b"II*\0", 4, None, C.byref(fax)) == -1 and lib.bbocr_host_tiff_fax_plan(b"II*\0", 4, C.byref(plan), None) == -1


def test_option_levels(monkeypatch):
    from bb_ocr_amd import reader as M

    monkeypatch.delenv("BBOCR_TIFF_DECODE", raising=False)
    assert M.tiff_decode_enabled() is False and M.tiff_decode_enabled(True) is True and M.tiff_decode_enabled("fax") == "fax"
    assert M.tiff_decode_enabled(" FAX ") == "fax" and M.tiff_decode_enabled(False) is False
    assert M.tiff_fax("fax") and not M.tiff_fax(True) and not M.tiff_fax("1") and not M.tiff_fax(False) and not M.tiff_fax(None)
    monkeypatch.setenv("BBOCR_TIFF_DECODE", "1")
    assert M.tiff_decode_enabled() is True and not M.tiff_fax(None) and M.tiff_decode_enabled(False) is False
    monkeypatch.setenv("BBOCR_TIFF_DECODE", "fax")
    assert M.tiff_decode_enabled() == "fax" and M.tiff_fax(None) and bool(M.tiff_decode_enabled()) and M.tiff_decode_enabled(True) is True
