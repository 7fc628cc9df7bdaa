"""The baseline JPEG decoder's yardsticks, without a GPU: the restatement of tests/jpeg_entropy_ref.py (marker parser + sequential
Huffman decoder, completed to samples by tests/jpeg_ref.py) equals the installed Pillow / libjpeg-turbo bit for bit; its model of the
device's passes (speculative decode, synchronisation, scan, write) returns the sequential decoder's states and coefficients; and
``bbocr_host_jpeg_plan`` (csrc/jpegdec.cpp) equals the restatement's parse and refuses what is out of scope, each with its reason."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import jpeg_entropy_ref as J

PHOTOS = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photos", n) for n in ("IMG_9684.JPG", "IMG_9685.JPG")]
SIZES = [(56, 40), (47, 33), (19, 17), (200, 120)]                                  # width x height
SETTINGS = [dict(quality=75), dict(quality=95, optimize=True), dict(quality=90, restart_marker_rows=1),
            dict(quality=100, restart_marker_blocks=3), dict(quality=20)]
CONTENTS = ["noise", "flat", "gradient"]


def picture(content, w, h, mode, seed=0):
    from PIL import Image

    c = 3 if mode == "RGB" else 1
    if content == "noise":
        a = np.random.default_rng(seed + 7 * w + h).integers(0, 256, (h, w, c), dtype=np.uint8)
    elif content == "flat":
        a = np.zeros((h, w, c), np.uint8) + np.array([200, 90, 40][:c], np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * 3 + yy * 2 + 40 * k) % 256 for k in range(c)], 2).astype(np.uint8)
    return Image.fromarray(a if c == 3 else a[:, :, 0], mode)


def save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def matrix(size=None):
    """[(name, file bytes)]: 4 sizes x 5 settings x 3 contents x {RGB 4:2:0, L}"""
    out = []
    for (w, h) in ([size] if size else SIZES):
        for si, s in enumerate(SETTINGS):
            for content in CONTENTS:
                for mode in ("RGB", "L"):
                    out.append(("%dx%d-s%d-%s-%s" % (w, h, si, content, mode), save(picture(content, w, h, mode), **s)))
    return out


@functools.lru_cache(maxsize=None)
def sync_inputs():
    """{name: file bytes} of the four synchronisation inputs: a photograph, a rendered text page, noise, and a flat page whose periodic
    stream a lane entering out of phase never leaves"""
    from bb_ocr_amd import synth
    from PIL import Image

    return {
        "photo": open(PHOTOS[1], "rb").read(),
        "text": save(Image.fromarray(synth.page(3, width=640, height=480, lines=12, margin=24)[0]), quality=90),
        "noise": save(picture("noise", 256, 384, "RGB"), quality=95),
        "flat": save(picture("flat", 256, 384, "RGB"), quality=95),
    }


def pillow_pixels(data):
    """What libjpeg hands Pillow: YCbCr triples of a colour file (decode_file_ycc's decode), the samples of a grey one"""
    from PIL import Image

    pil = Image.open(io.BytesIO(data))
    if pil.mode == "L":
        return np.asarray(pil)
    size = pil.size
    pil.draft("YCbCr", size)
    assert pil.mode == "YCbCr" and pil.size == size
    return np.asarray(pil)


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def c_plan(lib, data):
    from bb_ocr_amd import _lib

    p = _lib.bbocr_jpeg_plan()
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    assert lib.bbocr_host_jpeg_plan(buf, len(data), C.byref(p)) == 0
    return p


@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_pillow_on_the_matrix(size):
    files = matrix(size)
    assert len(files) == 30
    for name, data in files:
        plan = J.parse(data)
        assert plan["supported"], (name, plan)
        assert np.array_equal(J.decode_pixels(data, plan), pillow_pixels(data)), name


def test_restatement_equals_pillow_on_a_photograph():
    data = open(PHOTOS[1], "rb").read()
    assert np.array_equal(J.decode_pixels(data), pillow_pixels(data))


@pytest.mark.parametrize("name,S", [("photo", 1024), ("text", 1024), ("noise", 1024), ("flat", 1024), ("flat", 32)])
def test_model_of_the_device_passes_returns_the_sequential_states(name, S):
    data = sync_inputs()[name]
    plan = J.parse(data)
    coef, states = J.decode_coefficients(data, plan, S)
    m_coef, m_states, passes = J.device_model(data, plan, S, group=64)
    assert np.array_equal(m_states, states)
    assert np.array_equal(m_coef, coef)
    assert 1 <= passes <= -(-len(states) // 64) + 1            # the bound the host gives the device


def test_the_flat_page_never_synchronises_by_itself():
    """the case that exercises the exact-prefix propagation alone: a lane decoding from the assumed state leaves its subsequence in
    another state than the exact one, everywhere"""
    data = sync_inputs()["flat"]
    plan = J.parse(data)
    st = J.Stream(data, plan)
    _, states = J.decode_coefficients(data, plan, 32)
    subs = J.subsequences(st, 32)
    wrong = 0
    for i in range(1, len(subs) - 1):
        ex, _, _ = J._run(st, subs[i][0], (subs[i][1], 0, 0), subs[i][2], 1 << 60)
        wrong += tuple(states[i + 1][:3]) != ex
    assert wrong > (len(subs) - 2) // 2


@pytest.mark.parametrize("size", SIZES)
def test_plan_equals_the_restatement(lib, size):
    for name, data in matrix(size) + ([(p, open(p, "rb").read()) for p in PHOTOS] if size == SIZES[0] else []):
        want, got = J.parse(data), c_plan(lib, data)
        assert got.supported == 1 and got.reason == J.OK, name
        assert (got.width, got.height, got.components) == (want["width"], want["height"], want["components"]), name
        assert [tuple(s) for s in got.sampling][:got.components] == want["sampling"], name
        assert (got.restart_interval, got.mcu_cols, got.mcu_rows, got.segments) == (want["restart_interval"], want["mcu_cols"], want["mcu_rows"],
                                                                                   len(want["segments"])), name
        assert (got.scan_offset, got.scan_bytes) == (want["scan_offset"], want["scan_bytes"]), name


def test_matrix_holds_restart_files_and_optimised_tables():
    plans = [J.parse(d) for _, d in matrix()]
    assert sum(p["restart_interval"] > 0 for p in plans) == 48
    assert max(len(p["segments"]) for p in plans) > 30
    assert len({str(p["huff"]) for p in plans}) > 10


def test_plan_refuses_what_is_out_of_scope(lib):
    from PIL import Image

    img = picture("gradient", 64, 48, "RGB")
    good = save(img, quality=90)
    png = io.BytesIO()
    img.save(png, "PNG")
    dht = good.index(b"\xff\xc4")
    cases = [
        (save(img, quality=90, progressive=True), J.SOF),
        (save(img, quality=90, subsampling=0), J.SAMPLING),
        (save(img, quality=90, subsampling=1), J.SAMPLING),
        (save(Image.fromarray(np.zeros((48, 64, 4), np.uint8), "CMYK"), quality=90), J.COMPONENTS),
        (png.getvalue(), J.NOT_JPEG),
        (good[:-2], J.NO_EOI),
        (good[:dht + 40], J.TRUNCATED),
    ]
    for data, reason in cases:
        assert J.parse(data) == dict(supported=False, reason=reason)
        got = c_plan(lib, data)
        assert (got.supported, got.reason) == (0, reason)
    assert c_plan(lib, good).supported == 1
