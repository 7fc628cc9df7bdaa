"""CPU: the numpy restatement of the model-input JPEG encoder (tests/jpeg_encode_ref.py) against the installed Pillow byte for byte -- the
semantics csrc/jpegenc.hip must reproduce -- and the host half of the C ABI (bbocr_host_jpeg_header, bbocr_jpeg_encode_bound) and
``preprocess.model_image_host`` against Pillow as well."""
import base64
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpeg_encode_ref as er
from test_thumbnail_cpu import page

PHOTOS = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photos", n) for n in ("IMG_9684.JPG", "IMG_9685.JPG")]
QUALITIES = [30, 50, 85, 88, 95, 100]
# no dummy blocks | a dummy Y column, a dummy Y row, both | the last Y block real | narrower than an MCU
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (40, 24), (41, 57), (100, 131), (9, 25), (16, 7)]
CONTENTS = ["smooth", "text", "noise", "black", "hf"]
HF_POSITIONS = (17, 33, 49, 63)          # zig-zag positions of the one AC term of a block: runs of 16, 32, 48 zeros, and the last position


def content(kind, h, w, seed=0):
    """uint8 [h,w,3]: smooth, rendered text, uniform noise, all black, or blocks that hold one high-frequency cosine each"""
    if kind in ("smooth", "noise"):
        return page(kind, h, w, seed)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "text":
        from PIL import Image, ImageDraw

        im = Image.new("RGB", (w, h), (236, 230, 222))
        d = ImageDraw.Draw(im)
        for k, y in enumerate(range(0, h, 11)):
            d.text((1 - 3 * k, y), "The quick brown fox 0123456789 jumps", fill=(20 + 9 * k % 60, 24, 40))
        return np.asarray(im).copy()
    yy, xx = np.mgrid[0:h, 0:w]
    which = ((yy // 8) * (-(-w // 8)) + xx // 8) % 4
    g = np.zeros((h, w))
    for k, z in enumerate(HF_POSITIONS):
        v, u = divmod(er.ZIGZAG[z], 8)
        g = np.where(which == k, 128 + 100 * np.cos((2 * (xx % 8) + 1) * u * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * v * np.pi / 16), g)
    return np.repeat(np.rint(g).astype(np.uint8)[:, :, None], 3, 2)


def pil_jpeg(a, q, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q, **kw)
    return buf.getvalue()


def as_mode(img, mode):
    return img if mode == "RGB" else img[:, :, 1].copy()


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_restatement_equals_pillow(mode, q):
    for h, w in SHAPES:
        for kind in CONTENTS:
            a = as_mode(content(kind, h, w, seed=q), mode)
            assert er.encode(a, q) == pil_jpeg(a, q), (h, w, kind)


def test_content_classes_hold_what_they_are_for():
    coef = er.coefficients(content("hf", 40, 48), 85)
    ac = [tuple(np.flatnonzero(b[1:]) + 1) for b in coef]
    for z in HF_POSITIONS:
        assert (z,) in ac, z                                               # a block whose only AC term sits at z: ZRL x (z - 1) // 16
    black = er.coefficients(content("black", 16, 16), 85)
    n = abs(int(black[0, 0])).bit_length()
    assert n > 0 and not black[:, 1:].any() and not black[4:].any()
    # the first block codes its DC term; every other block is a DC difference of category 0 (2 bits in both tables) and EOB (4 / 2 bits)
    assert np.diff(er.block_bits(black, 3)).tolist() == [er.CODES["dc"][0][n][1] + n + 4, 6, 6, 6, 4, 4]
    noise = content("noise", 100, 131)
    assert er.pack(er.coefficients(noise, 100), 3).count(b"\xFF") > 20
    assert np.diff(er.block_bits(er.coefficients(noise, 100), 3)).max() > 63 * 8
    dummy = er.dummy_blocks(17, 33)                                        # 2 x 3 MCUs hold 3 x 5 real Y blocks
    assert dummy.sum() == 24 - 15
    coef = er.coefficients(content("noise", 17, 33), 95)
    for b in np.flatnonzero(dummy):
        assert not coef[b, 1:].any() and coef[b, 0] == coef[b - 1, 0]
    assert not er.dummy_blocks(9, 25).any() and not er.dummy_blocks(16, 16).any()


@pytest.mark.parametrize("components", [1, 3])
@pytest.mark.parametrize("q", [1, 50, 100])
def test_host_header_equals_pillow(lib, components, q):
    img = content("text", 23, 9)
    a = img if components == 3 else np.ascontiguousarray(img[:, :, 0])
    for comment in (None, b"", b"c" * 300):
        want = er.split_file(pil_jpeg(a, q, **({} if comment is None else {"comment": comment})))[0]
        out = (C.c_uint8 * 1024)()
        n = C.c_size_t()
        cb = (C.c_uint8 * len(comment)).from_buffer_copy(comment) if comment else None
        assert lib.bbocr_host_jpeg_header(23, 9, components, q, cb, len(comment or b""), out, 1024, C.byref(n)) == 0
        assert bytes(out[:n.value]) == want == er.header(23, 9, components, q, comment)
        if comment:
            assert b"\xFF\xFE" + (302).to_bytes(2, "big") + comment in want
    from PIL import Image

    tabs = Image.open(io.BytesIO(pil_jpeg(a, q))).quantization
    got = er.split_file(bytes(out[:n.value]))[0]
    p = got.index(b"\xFF\xDB")
    assert [got[p + 5 + er.ZIGZAG.index(k)] for k in range(64)] == list(tabs[0])            # (Pillow lists its tables in natural order)


def test_host_header_errors(lib):
    out = (C.c_uint8 * 1024)()
    n = C.c_size_t()
    f = lib.bbocr_host_jpeg_header
    assert f(16, 16, 3, 85, None, 0, out, 1024, C.byref(n)) == 0 and n.value > 600
    assert f(16, 16, 3, 85, None, 0, out, n.value - 1, C.byref(n)) == -1
    for args in [(0, 16, 3, 85), (16, 65536, 3, 85), (16, 16, 2, 85), (16, 16, 3, 0), (16, 16, 3, 101)]:
        assert f(*args, None, 0, out, 1024, C.byref(n)) == -1, args
    assert f(16, 16, 3, 85, None, 5, out, 1024, C.byref(n)) == -1
    assert f(16, 16, 3, 85, None, 0, None, 1024, C.byref(n)) == -1


def test_bound_holds_on_noise_and_is_the_stated_formula(lib):
    for h, w in SHAPES + [(64, 48)]:
        for comps in (1, 3):
            blocks = -(-h // 8) * -(-w // 8) if comps == 1 else 6 * -(-h // 16) * -(-w // 16)
            bound = lib.bbocr_jpeg_encode_bound(h, w, comps)
            assert bound == 66160 + 2 * -(-blocks * (22 + 63 * 26) // 8) + 2
            a = as_mode(content("noise", h, w), "RGB" if comps == 3 else "L")
            assert bound >= len(pil_jpeg(a, 100, comment=b"z" * 300)) + 65533 - 300              # (room for the longest comment)
    assert lib.bbocr_jpeg_encode_bound(0, 5, 3) == 0 and lib.bbocr_jpeg_encode_bound(5, 65536, 3) == 0 and lib.bbocr_jpeg_encode_bound(5, 5, 2) == 0


def reference_encode(image_path, max_dim=1600, jpeg_quality=85):
    """the body of ``_encode_image_for_model`` (enhanced_extractor.py:399-411)"""
    from PIL import Image

    try:
        img = Image.open(image_path).convert("RGB")
        img.thumbnail((max_dim, max_dim))
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=int(max(50, min(95, jpeg_quality))))
        return base64.b64encode(buf.getvalue()).decode("utf-8")
    except Exception:
        with open(image_path, "rb") as f:
            return base64.b64encode(f.read()).decode("utf-8")


@pytest.mark.parametrize("rule", [(1600, 85), (2000, 88), (3200, 95)])
def test_model_image_host_equals_the_reference(rule, tmp_path):
    from PIL import Image

    from bb_ocr_amd.preprocess import model_image_host

    commented = str(tmp_path / "c.jpg")
    Image.open(PHOTOS[1]).save(commented, quality=90, comment=b"shelf 3, box 12")
    for path in PHOTOS + [commented]:
        got = model_image_host(path, *rule)
        assert base64.b64encode(got).decode("utf-8") == reference_encode(path, *rule)
        with open(path, "rb") as f:
            assert model_image_host(f.read(), *rule) == got
    assert b"shelf 3, box 12" in got
    assert model_image_host(PHOTOS[1], 1600, 20) == model_image_host(PHOTOS[1], 1600, 50)       # the clamp of :406
    assert model_image_host(PHOTOS[1], 1600, 100) == model_image_host(PHOTOS[1], 1600, 95)


def test_model_image_rule_is_the_extractors():
    from bb_ocr_amd.preprocess import model_image_quality, model_image_rule

    assert [model_image_rule(i) for i in (0, 1, 7)] == [(2000, 88), (3200, 95), (3200, 95)]
    assert [model_image_quality(q) for q in (10, 50, 88, 95, 100)] == [50, 50, 88, 95, 95]
