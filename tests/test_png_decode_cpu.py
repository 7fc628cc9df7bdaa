"""The device PNG decoder without a card: the restatement (tests/png_decode_ref.py) against ``reader.decode_file`` (Pillow plus the stated
gray rule), ``bbocr_host_png_plan`` through ctypes -- every field, every refusal reason --, and the hand-written deflate streams and the
damage list against ``zlib.decompress``, which proves that the former are sound and the latter are not."""
import glob
import os
import struct
import zlib

import numpy as np
import pytest

import png_decode_ref as R
import png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_images", "*.png"))) + [
    os.path.join(ROOT, "tests", "golden", "trace", "example_15_image2_original.png")]
PLAN_FIELDS = ("width", "height", "bit_depth", "color_type", "channels", "bpp", "row_bytes", "palette_entries", "idat_chunks", "idat_bytes",
               "supported", "reason")


@pytest.fixture(scope="module")
def matrix():
    return R.matrix()


def written_files():
    """files of the device PNG writer's restatement (png_ref.png_file): chunks of dynamic and stored blocks, an iCCP chunk"""
    rng = np.random.default_rng(3)
    gray = np.repeat(rng.integers(0, 256, (40, 9), dtype=np.uint8), 7, axis=1)
    rgb = rng.integers(0, 256, (33, 70, 3), dtype=np.uint8)
    rgb[5:20] = 77
    return [("written_gray", png_ref.png_file(gray)), ("written_rgb", png_ref.png_file(rgb, icc=b"profile" * 20))]


def test_matrix_holds_every_axis_value_per_pair(matrix):
    names = [n for n, _ in matrix]
    assert len(names) == len(set(names)) == len(R.PAIRS) * len(R.WIDTHS) * len(R.HEIGHTS)
    want = set()
    for depth, ct in R.PAIRS:
        p = "d%dt%d" % (depth, ct)
        want |= {(p, "w%d" % w) for w in R.WIDTHS} | {(p, "h%d" % h) for h in R.HEIGHTS} | {(p, "%s%d" % f) for f in R.FILTER_PLANS}
        want |= {(p, c) for c in R.COMPRESSORS} | {(p, s) for s in R.SPLITS}
    assert R.axis_values(names) == want
    gpu = [n for n, _ in R.matrix(R.GPU_WIDTHS, R.GPU_HEIGHTS)]          # the GPU tests' part: the same, at its widths and heights
    skipped = {"w%d" % w for w in set(R.WIDTHS) - set(R.GPU_WIDTHS)} | {"h%d" % h for h in set(R.HEIGHTS) - set(R.GPU_HEIGHTS)}
    assert R.axis_values(gpu) == {v for v in want if v[1] not in skipped}


def test_restatement_equals_decode_file(matrix):
    from bb_ocr_amd.reader import decode_file

    for name, f in matrix + written_files():
        d = R.decode(f)
        rgb, gray = decode_file(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        assert len(d["stage0"]) == d["plan"]["height"] * (1 + d["plan"]["row_bytes"]) and d["stage1"].shape == (d["plan"]["height"], 1 + d["plan"]["row_bytes"])


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_restatement_equals_decode_file_on_stored_files(path):
    from bb_ocr_amd.reader import decode_file

    d = R.decode(open(path, "rb").read())
    rgb, gray = decode_file(path)
    assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray)


# ------------------------------------------------------------------------------------------------ the plan
def _zlib_header(cm=8, cinfo=7, fdict=0, fcheck_ok=True):
    b0 = (cinfo << 4) | cm
    b1 = fdict << 5
    b1 += (31 - ((b0 << 8) | b1) % 31) % 31
    if not fcheck_ok:
        b1 ^= 1
    return bytes([b0, b1])


def refusals():
    """[(name, file, the BBOCR_PNG_* reason)] -- every reason, each on a file built to trigger it"""
    rng = np.random.default_rng(11)
    raw = b"".join(b"\x00" + rng.integers(0, 4, 10, dtype=np.uint8).tobytes() for _ in range(6))        # 6 rows of 10 bytes
    z = zlib.compress(raw)
    pal = R.palette_of(8, 0)
    parts = [("IHDR", R.ihdr(10, 6, 8, 3)), ("gAMA", R.chunk(b"gAMA", struct.pack(">I", 45455))), ("PLTE", R.chunk(b"PLTE", pal)),
             ("tRNS", R.chunk(b"tRNS", b"\x00\x80")), ("IDAT", R.chunk(b"IDAT", z[:9])), ("IDAT2", R.chunk(b"IDAT", z[9:])), ("IEND", R.chunk(b"IEND", b""))]
    good = R.SIG + b"".join(c for _, c in parts)
    assert R.plan(good)["supported"] == 1
    out = [("no_signature", b"\xff\xd8\xff\xe0" + good[4:], R.NOT_PNG), ("empty", b"", R.NOT_PNG), ("seven_bytes", R.SIG[:7], R.NOT_PNG),
           ("signature_alone", R.SIG, R.TRUNCATED), ("no_iend", good[:-12], R.TRUNCATED)]
    at = 8
    for name, c in parts:                                                  # a file cut inside each chunk kind: in its header, payload and CRC
        for cut in (3, 8 + (len(c) - 12) // 2, len(c) - 2):
            out.append(("cut_in_%s_at_%d" % (name, cut), good[:at + cut], R.TRUNCATED))
        at += len(c)
    at = 8
    for name, c in parts:
        flipped = bytearray(good)
        flipped[at + len(c) - 1] ^= 0x40
        out.append(("crc_" + name, bytes(flipped), R.CRC))                # the ancillary chunks too: Pillow refuses such a file
        at += len(c)

    def gray(w, h, depth=8, ct=0, lace=0, idat=None, **kw):
        return R.png_bytes(w, h, depth, ct, [z] if idat is None else idat, lace=lace, **kw)

    out += [("zero_width", gray(0, 6), R.DIMENSIONS), ("zero_height", gray(10, 0), R.DIMENSIONS),
            ("oversized", gray(2 ** 31 - 1, 2), R.DIMENSIONS), ("oversized_rows", gray(2 ** 16, 2 ** 15), R.DIMENSIONS),
            ("wide_1_bit", gray(2 ** 31 - 8, 1, 1), R.DIMENSIONS), ("pixels_above_pillows_limit", gray(R.MAX_PIXELS // 2 + 1, 2, 1), R.DIMENSIONS),
            ("depth_16", gray(10, 6, 16), R.DEPTH), ("depth_16_rgb", gray(10, 6, 16, 2), R.DEPTH), ("depth_4_rgb", gray(10, 6, 4, 2), R.DEPTH),
            ("depth_3", gray(10, 6, 3), R.DEPTH), ("depth_16_palette", gray(10, 6, 16, 3), R.DEPTH), ("adam7", gray(10, 6, lace=1), R.INTERLACE),
            ("adam7_written", R.adam7_file(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)), R.INTERLACE),
            ("colour_type_5", gray(10, 6, 8, 5), R.HEADER), ("interlace_2", gray(10, 6, lace=2), R.HEADER),
            ("palette_missing", gray(10, 6, 8, 3), R.PALETTE),
            ("palette_behind_idat", R.SIG + R.ihdr(10, 6, 8, 3) + R.chunk(b"IDAT", z) + R.chunk(b"PLTE", pal) + R.chunk(b"IEND", b""), R.PALETTE),
            ("palette_twice", gray(10, 6, 8, 3, palette=pal, after_plte=R.chunk(b"PLTE", pal)), R.PALETTE),
            ("palette_of_4_bytes", gray(10, 6, 8, 3, palette=pal[:4]), R.PALETTE),
            ("idat_not_consecutive", R.SIG + R.ihdr(10, 6, 8, 0) + R.chunk(b"IDAT", z[:5]) + R.chunk(b"tEXt", b"a\x00b") + R.chunk(b"IDAT", z[5:])
             + R.chunk(b"IEND", b""), R.IDAT_ORDER),
            ("apng", gray(10, 6, before_plte=R.chunk(b"acTL", struct.pack(">II", 1, 0))), R.APNG),
            ("ihdr_second", R.SIG + R.chunk(b"gAMA", struct.pack(">I", 45455)) + good[8:], R.HEADER),
            ("ihdr_of_12_bytes", R.SIG + R.chunk(b"IHDR", b"\x00" * 12) + good[33:], R.HEADER), ("ihdr_twice", R.SIG + R.ihdr(10, 6, 8, 0) + good[8:], R.HEADER),
            ("no_idat", R.SIG + R.ihdr(10, 6, 8, 0) + R.chunk(b"IEND", b""), R.HEADER)]
    body = z[2:]
    out += [("zlib_method_7", gray(10, 6, idat=[_zlib_header(cm=7) + body]), R.ZLIB), ("zlib_window_64k", gray(10, 6, idat=[_zlib_header(cinfo=8) + body]), R.ZLIB),
            ("zlib_fdict", gray(10, 6, idat=[_zlib_header(fdict=1) + b"\x00\x00\x00\x01" + body]), R.ZLIB),
            ("zlib_fcheck", gray(10, 6, idat=[_zlib_header(fcheck_ok=False) + body]), R.ZLIB), ("zlib_of_one_byte", gray(10, 6, idat=[z[:1]]), R.ZLIB),
            ("zlib_fdict_split", gray(10, 6, idat=[b"\x78", b"", bytes([_zlib_header(fdict=1)[1]]) + body]), R.ZLIB)]
    assert R.plan(gray(10, 6, idat=[_zlib_header(cinfo=0) + body]))["supported"] == 1                  # a 256-byte window is legal
    assert R.plan(gray(R.MAX_PIXELS // 2, 2, 1))["supported"] == 1                                      # Pillow's limit itself is inside
    return out


def _c_plan(data):
    from bb_ocr_amd import reader

    p = reader.png_plan(data)
    return {k: int(getattr(p, k)) for k in PLAN_FIELDS}


def test_host_plan_fields_on_the_matrix(matrix):
    for name, f in matrix + written_files() + [(p, open(p, "rb").read()) for p in GOLDEN]:
        want = R.plan(f)
        assert want["supported"] == 1 and _c_plan(f) == want, name
    f = next(f for n, f in matrix if n.startswith("d4t3_9x65_"))
    assert {k: R.plan(f)[k] for k in PLAN_FIELDS[:8]} == dict(width=9, height=65, bit_depth=4, color_type=3, channels=1, bpp=1, row_bytes=5, palette_entries=16)
    bytewise = next(f for n, f in matrix if n.endswith("_bytes") and n.startswith("d8t6_65x129"))
    assert R.plan(bytewise)["idat_chunks"] == R.plan(bytewise)["idat_bytes"] > 100 and R.plan(bytewise)["bpp"] == 4


def test_host_plan_refusals():
    cases = refusals()
    assert {r for _, _, r in cases} == set(range(1, 12))                   # every reason of bbocr.h
    for name, f, reason in cases:
        want = R.plan(f)
        assert want["reason"] == reason and want["supported"] == 0, (name, want)
        assert _c_plan(f) == want, name
        from bb_ocr_amd import reader
        assert reader.png_page(f) is None, name
    from bb_ocr_amd import _lib
    assert [_lib.PNG_OK, _lib.PNG_NOT_PNG, _lib.PNG_TRUNCATED, _lib.PNG_CRC, _lib.PNG_DIMENSIONS, _lib.PNG_DEPTH, _lib.PNG_INTERLACE, _lib.PNG_PALETTE,
            _lib.PNG_IDAT_ORDER, _lib.PNG_APNG, _lib.PNG_ZLIB, _lib.PNG_HEADER] == list(range(12))
    header = open(os.path.join(ROOT, "include", "bbocr.h")).read()
    for k, name in enumerate(("OK", "NOT_PNG", "TRUNCATED", "CRC", "DIMENSIONS", "DEPTH", "INTERLACE", "PALETTE", "IDAT_ORDER", "APNG", "ZLIB", "HEADER")):
        assert "BBOCR_PNG_%s = %d" % (name, k) in header


def test_png_page_and_option_default(matrix, monkeypatch):
    from bb_ocr_amd import reader

    name, f = matrix[100]
    page = reader.png_page(f)
    pl = R.plan(f)
    assert page.shape == (pl["height"], pl["width"], 3) and page.data == f
    assert reader.png_page(b"\xff\xd8\xff") is None and reader.png_page("/nonexistent/file.png") is None
    monkeypatch.delenv("BBOCR_PNG_DECODE", raising=False)
    assert reader.png_decode_enabled(None) is False and reader.png_decode_enabled(True) is True
    monkeypatch.setenv("BBOCR_PNG_DECODE", "1")
    assert reader.png_decode_enabled(None) is True and reader.png_decode_enabled(False) is False
    monkeypatch.setenv("BBOCR_PNG_DEVICE", "1")                            # the encoder's switch is another one
    monkeypatch.setenv("BBOCR_PNG_DECODE", "0")
    assert reader.png_decode_enabled(None) is False


# ------------------------------------------------------------------------------------------------ the streams
def test_handwritten_streams_are_sound():
    streams = R.handwritten()
    names = [n for n, _, _ in streams]
    for want in ("distance_32768", "length_258_and_3", "stored_0_and_65535_unaligned", "empty_dynamic_block", "hclen_4",
                 "repeat_crosses_into_distances", "single_distance_code", "no_distance_code", "code_of_15_bits", "stored_fixed_dynamic"):
        assert want in names
    assert {"distance_%d_below_length" % d for d in (1, 2, 3, 63, 64, 65)} <= set(names)
    for name, z, data in streams:
        d = zlib.decompressobj()
        assert d.decompress(z) == data and d.eof and not d.unused_data, name
        f = R.wrap_stream(z, len(data))
        assert R.plan(f)["supported"] == 1 and R.plan(f)["height"] * (1 + R.plan(f)["row_bytes"]) == len(data), name
    assert len(dict((n, d) for n, _, d in streams)["stored_0_and_65535_unaligned"]) == 65538


def test_damage_list_is_damaged():
    cases = R.damaged()
    assert [n for n, _, _ in cases] == ["truncated_at_a_third", "block_type_3", "len_nlen_mismatch", "oversubscribed_code", "incomplete_code",
                                        "distance_too_far", "wrong_adler", "one_byte_too_many", "one_byte_too_few", "filter_byte_5"]
    for name, z, length in cases:
        f = R.wrap_stream(z, length, 3)
        assert R.plan(f)["supported"] == 1, name                           # the plan cannot know: the device must answer with a status
        with pytest.raises(R.Refused):
            R.decode(f)
        if name == "filter_byte_5":
            assert len(zlib.decompress(z)) == length and zlib.decompress(z)[200] == 5
            continue
        try:
            d = zlib.decompressobj()
            got = d.decompress(z)
            assert not d.eof or len(got) != length, name
        except zlib.error:
            pass
