"""4:4:4, 4:2:2 and 4:4:0 JPEG files without a GPU: the restatement of tests/jpeg_chroma_ref.py equals the installed Pillow /
libjpeg-turbo bit for bit; ``bbocr_host_jpeg_plan`` (csrc/jpegdec.cpp) equals its plan field by field, ``chroma`` included, while
``supported`` and ``reason`` stay what they were; and ``device_decode="chroma"`` -- nothing else -- routes such a file to the device
decoder (``reader.jpeg_page``, ``extractor_batch.read_files`` with the recording Reader of test_read_files_cpu.py)."""
import functools

import numpy as np
import pytest

import jpeg_chroma_ref as K
import jpeg_entropy_ref as J
import orient_ref as R
from test_jpeg_decode_cpu import c_plan, lib, picture, pillow_pixels, save  # noqa: F401  (lib: a fixture)

# width x height: 1x1 .. 4x4 hold one- and two-sample chroma rows (replication instead of the h2v1 filter) and one-row planes; 5x17, 17x9,
# 33x47, 131x67 end in partial MCUs on either or both axes; 16x8 is exactly one 4:2:2 MCU; the larger ones hold several restart segments
SIZES = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 17), (16, 8), (17, 9), (33, 47), (64, 48), (131, 67), (200, 120)]
CONTENTS = ["noise", "gradient"]
SETTINGS = [dict(quality=90), dict(quality=35, optimize=True), dict(quality=95, restart_marker_rows=1), dict(quality=75, restart_marker_blocks=3)]
SUBSAMPLING = {K.C444: 0, K.C422: 1}                              # Pillow's ``subsampling`` of the classes it writes


@functools.lru_cache(maxsize=None)
def matrix(size=None):
    """[(name, chroma class, file bytes)]: 11 sizes x 2 contents x (4:4:4 and 4:2:2 in 4 settings each, 4:4:0 from the first 4:2:2 setting
    of the transposed size) = 198 files"""
    out = []
    for (w, h) in ([size] if size else SIZES):
        for content in CONTENTS:
            for cls, sub in SUBSAMPLING.items():
                for si, s in enumerate(SETTINGS):
                    out.append(("%dx%d-%s-c%d-s%d" % (w, h, content, cls, si), cls, save(picture(content, w, h, "RGB"), subsampling=sub, **s)))
            src = save(picture(content, h, w, "RGB"), subsampling=1, **SETTINGS[0])
            out.append(("%dx%d-%s-c%d" % (w, h, content, K.C440), K.C440, K.make_440(src)))
    return out


@functools.lru_cache(maxsize=None)
def stage_input(name):
    """(file bytes, S) of one of the four inputs of the stage tests: 256x384 noise at quality 95 as 4:4:4 and as 4:2:2 (more than two
    workgroups of 1024-bit subsequences), its 4:4:0 transposition, and the flat page as 4:2:2 cut every 32 bits (the periodic stream a lane
    entering out of phase never leaves)"""
    if name == "noise440":
        return K.make_440(save(picture("noise", 384, 256, "RGB"), quality=95, subsampling=1)), 0
    content, sub, S = {"noise444": ("noise", 0, 0), "noise422": ("noise", 1, 0), "flat422": ("flat", 1, 32)}[name]
    return save(picture(content, 256, 384, "RGB"), quality=95, subsampling=sub), S


@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_pillow_on_the_matrix(size):
    files = matrix(size)
    assert len(files) == 18
    for name, cls, data in files:
        plan = K.parse(data)
        assert (plan["chroma"], plan["supported"], plan["reason"]) == (cls, False, J.SAMPLING), name
        assert J.parse(data) == dict(supported=False, reason=J.SAMPLING), name          # the yardstick of today's scope refuses it
        assert (plan["width"], plan["height"]) == size and plan["sampling"] == [K.LUMA[cls], (1, 1), (1, 1)], name
        want = pillow_pixels(data)
        assert want.shape == (size[1], size[0], 3), name
        assert np.array_equal(K.decode_pixels(data, plan), want), name


def test_the_440_files_are_what_pillow_reads_as_1x2():
    import io

    from PIL import Image

    for name, cls, data in matrix((33, 47)):
        if cls == K.C440:
            assert [l[1:3] for l in Image.open(io.BytesIO(data)).layer] == [(1, 2), (1, 1), (1, 1)], name


def test_matrix_holds_every_path_of_the_upsamplers_and_restart_files():
    plans = [(cls, K.parse(d)) for _, cls, d in matrix()]
    assert len(plans) == 198
    assert sum(p["restart_interval"] > 0 for _, p in plans) == 88
    assert max(len(p["segments"]) for _, p in plans) > 30
    narrow = [p for c, p in plans if c == K.C422 and -(-p["width"] // 2) <= 2]       # h2v1 replication
    wide = [p for c, p in plans if c == K.C422 and -(-p["width"] // 2) > 2]
    assert narrow and wide and any(p["width"] % 16 for p in wide) and any(p["height"] % 16 for c, p in plans if c == K.C440)


def test_restatement_inside_todays_scope_is_the_existing_one():
    for mode in ("RGB", "L"):
        data = save(picture("noise", 47, 33, mode), quality=90)
        plan = K.parse(data)
        assert plan["supported"] and plan["chroma"] == 0
        assert np.array_equal(K.decode_pixels(data, plan), J.decode_pixels(data))
        assert np.array_equal(K.decode_coefficients(data, plan)[0], J.decode_coefficients(data, plan)[0])


@pytest.mark.parametrize("size", SIZES)
def test_plan_equals_the_restatement(lib, size):
    for name, cls, data in matrix(size):
        want, got = K.parse(data), c_plan(lib, data)
        assert (got.supported, got.reason, got.chroma) == (0, J.SAMPLING, cls), name
        assert (got.width, got.height, got.components) == (want["width"], want["height"], 3), name
        assert [tuple(s) for s in got.sampling] == want["sampling"], name
        assert (got.restart_interval, got.mcu_cols, got.mcu_rows, got.segments) == (want["restart_interval"], want["mcu_cols"], want["mcu_rows"],
                                                                                   len(want["segments"])), name
        assert (got.scan_offset, got.scan_bytes) == (want["scan_offset"], want["scan_bytes"]), name
        assert got.orientation == 1 and list(got.reserved) == [0, 0], name
    o = c_plan(lib, R.with_orientation(matrix(size)[0][2], 6, "MM"))
    assert (o.orientation, o.chroma, o.supported) == (6, K.C444, 0)


def test_chroma_is_zero_for_everything_else(lib):
    from PIL import Image

    img = picture("gradient", 64, 48, "RGB")
    f444 = save(img, quality=90, subsampling=0)
    sof = b"\xff\xc0\x00\x11\x08\x00\x30\x00\x40\x03\x01"
    assert f444.count(sof + b"\x11") == 1
    f411 = f444.replace(sof + b"\x11", sof + b"\x41")
    cases = [
        (save(img, quality=90, subsampling=0, progressive=True), 0, J.SOF),
        (save(Image.fromarray(np.zeros((48, 64, 4), np.uint8), "CMYK"), quality=90), 0, J.COMPONENTS),
        (save(img, quality=90), 1, J.OK),
        (save(img.convert("L"), quality=90), 1, J.OK),
        (f444[:-2], 0, J.SAMPLING),                              # a 4:4:4 file that fails a later check (no EOI) stays refused ...
        (f411, 0, J.SAMPLING),                                   # 4:1:1: a sampling outside the three classes
    ]
    for k, (data, supported, reason) in enumerate(cases):
        got = c_plan(lib, data)
        assert (got.supported, got.reason, got.chroma) == (supported, reason, 0), k
        assert K.parse(data)["chroma"] == 0 and K.parse(data)["reason"] == reason, k
    cut = c_plan(lib, f444[:-2])                                  # ... as before: nothing behind the sampling test is reported
    assert (cut.width, cut.height, cut.mcu_cols, cut.mcu_rows, cut.segments, cut.scan_offset, cut.scan_bytes) == (64, 48, 0, 0, 0, 0, 0)
    assert c_plan(lib, f444).chroma == K.C444


def test_jpeg_page_takes_the_file_only_when_asked(tmp_path):
    from bb_ocr_amd.reader import jpeg_chroma, jpeg_page

    d = save(picture("gradient", 64, 48, "RGB"), quality=90, subsampling=1)
    assert jpeg_page(d) is None and jpeg_page(d, chroma=False) is None
    page = jpeg_page(d, chroma=True)
    assert page is not None and page.shape == (48, 64, 3) and page.data == d
    p = tmp_path / "f422.jpg"
    p.write_bytes(d)
    assert jpeg_page(str(p)) is None and jpeg_page(str(p), chroma=True).shape == (48, 64, 3)
    good = save(picture("gradient", 64, 48, "RGB"), quality=90)
    assert jpeg_page(good) is not None and jpeg_page(good, chroma=True) is not None
    assert jpeg_page(save(picture("gradient", 64, 48, "RGB"), quality=90, progressive=True), chroma=True) is None
    assert [jpeg_chroma(v) for v in ("chroma", " Chroma ", True, False, None, "1", 1)] == [True, True, False, False, False, False, False]


def test_read_files_routes_by_the_option(tmp_path):
    """the recording Reader of test_read_files_cpu.py: a 4:4:4 file travels as its bytes ("jpg": one decode_jpeg_batch call) with
    ``device_decode="chroma"`` and as host triples ("ycc": an upload) with ``True`` -- next to a 4:2:0 file, which both send as bytes"""
    from bb_ocr_amd.extractor_batch import _ocr_input, _plain_input_device, read_files
    from test_read_files_cpu import KW, FakeDeviceReader

    img = picture("noise", 64, 48, "RGB")
    p444, p420 = tmp_path / "a444.jpg", tmp_path / "b420.jpg"
    p444.write_bytes(save(img, quality=90, subsampling=0))
    p420.write_bytes(save(img, quality=90))
    assert _plain_input_device(p444, 0, "chroma")[0] == "jpg" and _plain_input_device(p444, 0, True)[0] == "ycc"
    assert _plain_input_device(p444)[0] == "ycc" and _plain_input_device(p420)[0] == "jpg"
    assert _ocr_input(p444, 0, True, "chroma")[0] == "jpg" and _ocr_input(p444, 0, True, True)[0] == "ycc"
    results = {}
    for opt, want in (("chroma", [("decode_jpeg_batch", (2, 48, 64, 3))]), (True, [("decode_jpeg_batch", (1, 48, 64, 3)), ("_to_dev", (1, 48, 64, 4))])):
        fd = FakeDeviceReader()
        results[opt] = read_files(fd, [p444, p420], None, 4, 2, device_decode=opt, **KW)
        assert sorted(c for c in fd.calls if c[0] in ("decode_jpeg_batch", "_to_dev")) == sorted(want), opt
    host = read_files(FakeDeviceReader(), [p444, p420], None, 4, 2, **KW)
    assert results["chroma"] == results[True] == host and all(len(v) == 2 for v in host.values())
