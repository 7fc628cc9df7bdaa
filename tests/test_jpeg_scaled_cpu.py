"""The trace previews' yardsticks, without a GPU: the restatement of tests/jpeg_scaled_ref.py (reduced IDCTs, plane geometry, draft rule,
boxed resize) equals the installed Pillow / libjpeg-turbo bit for bit; ``bbocr_host_resize_plan`` and ``bbocr_jpeg_scaled_dims`` equal the
restatement; ``preprocess.preview_host`` is Pillow's thumbnail of an unloaded file with the ICC profile carried, and the installed Pillow
rewrites the one preview of the reference that is committed byte for byte."""
import base64
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import jpeg_entropy_ref as J
import jpeg_ref as R
import jpeg_scaled_ref as S
from test_jpeg_decode_cpu import picture, save

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALES = (2, 4, 8)
F1_SIZES = [(1, 1), (8, 8), (17, 23), (33, 50), (48, 64), (127, 255)]                      # H x W
EDGES = (15, 16, 17, 31, 32, 33)
# (H, W, max_dim): draft scales 1 / 2 / 4, with and without the reduce step, fractional boxes
F2_CASES = [(150, 200, 10), (150, 201, 24), (97, 333, 16), (480, 640, 100), (301, 203, 33), (64, 48, 5), (1000, 37, 20), (130, 2000, 40)]


def content(kind, w, h, mode):
    from PIL import Image

    if kind == "text":
        from bb_ocr_amd import synth

        a = synth.page(3, width=max(w, 64), height=max(h, 48), lines=3, margin=4)[0][:h, :w]
        img = Image.fromarray(np.ascontiguousarray(a))
        return img if mode == "RGB" else img.convert("L")
    return picture(kind, w, h, mode)


def pillow_draft(data, s):
    """libjpeg's decode at 1 / s as Pillow's draft asks for it: YCbCr triples or grey samples"""
    from PIL import Image

    pil = Image.open(io.BytesIO(data))
    W, H = pil.size
    mode = "L" if pil.mode == "L" else "YCbCr"
    oh, ow = S.scaled_dims(H, W, s)
    if S.draft_scale(W, H, max(W // s, 1), max(H // s, 1)) == s:
        pil.draft(mode, (max(W // s, 1), max(H // s, 1)))
    else:
        # a size no request reaches at this scale (draft never scales an image below one pixel per requested pixel): what draft sets,
        # set by hand -- the decoder's scale, the image's size and the tile's extent
        pil.draft(mode, None)
        tile = pil.tile[0]
        pil.tile = [type(tile)(tile[0], (0, 0, ow, oh), tile[2], tile[3])]
        pil._size = (ow, oh)
        pil.decoderconfig = (s, 0)
    assert pil.decoderconfig == (s, 0) and pil.mode == mode and pil.size == (ow, oh), (pil.decoderconfig, pil.size, (W, H, s))
    return np.asarray(pil)


@functools.lru_cache(maxsize=None)
def f1_matrix():
    """[(name, file bytes)]: the F1 sizes x {noise, gradient} x {4:2:0, grey} x quality {30, 90, 100}"""
    out = []
    for (h, w) in F1_SIZES:
        for kind in ("noise", "gradient"):
            for mode in ("RGB", "L"):
                for q in (30, 90, 100):
                    out.append(("%dx%d-%s-%s-q%d" % (h, w, kind, mode, q), save(picture(kind, w, h, mode), quality=q)))
    return out


@functools.lru_cache(maxsize=None)
def edge_matrix():
    """widths and heights around the MCU edges, a restart-interval file among them, text and flat content"""
    out = []
    for k, h in enumerate(EDGES):
        for j, w in enumerate(EDGES):
            kind = ("text", "flat", "noise")[(k + j) % 3]
            mode = "L" if (k * 6 + j) % 4 == 3 else "RGB"
            kw = dict(quality=90, restart_marker_blocks=2) if (k + 2 * j) % 5 == 0 else dict(quality=85)
            out.append(("%dx%d-%s-%s%s" % (h, w, kind, mode, "-rst" if len(kw) == 2 else ""), save(content(kind, w, h, mode), **kw)))
    out.append(("96x160-text-RGB-rst", save(content("text", 160, 96, "RGB"), quality=92, restart_marker_rows=1)))
    return out


def small_matrix():
    """the GPU test's files: every 6th of the F1 matrix and the edge files"""
    return f1_matrix()[::6] + f1_matrix()[3::18] + edge_matrix()


@pytest.mark.parametrize("s", SCALES)
def test_restatement_equals_pillows_draft_on_the_f1_matrix(s):
    files = f1_matrix()
    assert len(files) * len(SCALES) == 216
    for name, data in files:
        assert np.array_equal(S.scaled_pixels(data, s), pillow_draft(data, s)), (name, s)


@pytest.mark.parametrize("s", SCALES)
def test_restatement_equals_pillows_draft_at_the_mcu_edges(s):
    files = edge_matrix()
    assert sum(J.parse(d)["restart_interval"] > 0 for _, d in files) >= 5
    for name, data in files:
        assert np.array_equal(S.scaled_pixels(data, s), pillow_draft(data, s)), (name, s)


def test_restatement_equals_pillows_draft_on_a_photograph():
    data = open(os.path.join(GOLDEN, "photos", "IMG_9684.JPG"), "rb").read()
    plan = J.parse(data)
    coef, _ = J.decode_coefficients(data, plan)
    for s in SCALES:
        assert np.array_equal(S.planes_to_pixels(S.scaled_planes(coef, plan, s), plan, s), pillow_draft(data, s)), s


def test_draft_rule_equals_pillow():
    from PIL import Image

    for (h, w) in [(150, 200), (97, 333), (480, 640), (1000, 37), (64, 48), (33, 50)]:
        data = save(picture("gradient", w, h, "RGB"), quality=75)
        for req in (3, 10, 24, 47, 100, 700):
            pil = Image.open(io.BytesIO(data))
            res = pil.draft(None, (req, req))
            s = S.draft_scale(w, h, req, req)
            assert pil.decoderconfig == (s, 0) and res[1] == (0, 0, w / s, h / s) and pil.size == S.scaled_dims(h, w, s)[::-1]


@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_thumbnail_of_an_unloaded_file_is_scaled_decode_plus_boxed_resize(mode):
    from PIL import Image

    scales = set()
    for (h, w, m) in F2_CASES:
        data = save(picture("noise" if (h + w) % 2 else "gradient", w, h, mode), quality=90)
        pil = Image.open(io.BytesIO(data))
        pil.thumbnail((m, m))
        scales.add(pil.decoderconfig[0])
        assert np.array_equal(S.thumbnail_of_file(data, m), np.asarray(pil)), (h, w, m)
    assert scales >= {1, 2, 4}


def test_boxed_resize_equals_pillow():
    from PIL import Image

    rng = np.random.default_rng(5)
    for (h, w, m) in F2_CASES:
        ow, oh = R.thumbnail_size(w, h, m)
        for s in (1, 2, 4):
            sh, sw = S.scaled_dims(h, w, s)
            for ch in (1, 3):
                a = rng.integers(0, 256, (sh, sw, ch), dtype=np.uint8)
                a = a[:, :, 0] if ch == 1 else a
                want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC, box=(0, 0, w / s, h / s), reducing_gap=2.0))
                assert np.array_equal(S.boxed_resize(a, ow, oh, w / s, h / s), want), (h, w, m, s, ch)


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def test_host_entry_points_equal_the_restatement(lib):
    oh, ow = C.c_int(), C.c_int()
    for (h, w) in F1_SIZES + [(4284, 5712), (65535, 65535)]:
        for s in (1, 2, 4, 8):
            assert lib.bbocr_jpeg_scaled_dims(h, w, s, C.byref(oh), C.byref(ow)) == 0
            assert (oh.value, ow.value) == S.scaled_dims(h, w, s)
    assert lib.bbocr_jpeg_scaled_dims(8, 8, 3, C.byref(oh), C.byref(ow)) != 0
    assert lib.bbocr_jpeg_scaled_dims(0, 8, 2, C.byref(oh), C.byref(ow)) != 0
    fac, box = (C.c_int * 2)(), (C.c_float * 4)()
    for (h, w, m) in F2_CASES + [(4284, 5712, 800), (4284, 5712, 200)]:
        tw, th = R.thumbnail_size(w, h, m)
        for s in (1, 2, 4, 8):
            sh, sw = S.scaled_dims(h, w, s)
            assert lib.bbocr_host_resize_plan(sh, sw, th, tw, w / s, h / s, fac, box) == 0
            fx, fy, b = S.boxed_resize_plan(tw, th, w / s, h / s)
            assert (fac[0], fac[1]) == (fx, fy) and tuple(box) == b, (h, w, m, s)
    # a box that does not end inside the last pixel, or outside the image, is refused
    assert lib.bbocr_host_resize_plan(100, 100, 10, 10, 98.5, 100.0, fac, box) != 0
    assert lib.bbocr_host_resize_plan(100, 100, 10, 10, 100.5, 100.0, fac, box) != 0
    # the whole-image plan keeps its results
    f2, rb, fb = (C.c_int * 2)(), (C.c_int * 4)(), (C.c_float * 4)()
    for (h, w, m) in F2_CASES:
        assert lib.bbocr_host_thumbnail_plan(h, w, m, C.byref(oh), C.byref(ow), f2, rb, fb) == 0
        assert lib.bbocr_host_resize_plan(h, w, oh.value, ow.value, float(w), float(h), fac, box) == 0
        assert (fac[0], fac[1]) == (f2[0], f2[1]) and tuple(box) == tuple(fb)


def stored_preview():
    """(file bytes, PIL image) of the one preview of the reference that is committed: ``original_b64`` of image 2 of its example_15.json
    (800 x 600, RGB, the photograph's 536-byte ICC profile embedded).  The 3.2-MB photograph it was made from is not in the repository,
    so nothing here or on the card reproduces this file from its source."""
    from PIL import Image

    stored = open(os.path.join(GOLDEN, "trace", "example_15_image2_original.png"), "rb").read()
    ref = Image.open(io.BytesIO(stored))
    assert ref.size == (800, 600) and ref.mode == "RGB" and len(ref.info["icc_profile"]) == 536
    return stored, ref


def test_installed_pillow_rewrites_the_stored_preview_byte_for_byte():
    """the last step of every preview -- Pillow's PNG writer on given pixels, mode and ICC profile -- yields the very file the reference
    stored: the premise under which equal pixels mean an equal string"""
    from PIL import Image

    stored, ref = stored_preview()
    buf = io.BytesIO()
    again = Image.fromarray(np.asarray(ref))
    again.info["icc_profile"] = ref.info["icc_profile"]
    again.save(buf, format="PNG")
    assert buf.getvalue() == stored


def test_preview_host_is_pillows_thumbnail_at_draft_scale_2_with_the_profile_carried():
    """``preview_host(file, 400)`` of a 2200 x 1650 4:2:0 file that carries the stored preview's ICC profile and EXIF orientation 6: the string
    decodes to Pillow's own ``thumbnail((400, 400))`` of the file (draft scale 2, un-oriented) and to the restatement's pixels, mode RGB,
    the profile embedded"""
    from PIL import Image

    from bb_ocr_amd.preprocess import preview_host

    _, ref = stored_preview()
    exif = Image.Exif()
    exif[0x0112] = 6
    data = save(ref.resize((2200, 1650), Image.BICUBIC), quality=90, icc_profile=ref.info["icc_profile"], exif=exif)
    url = preview_host(data, 400)
    assert url.startswith("data:image/png;base64,")
    got = Image.open(io.BytesIO(base64.b64decode(url.split(",", 1)[1])))
    assert got.size == (400, 300) and got.mode == "RGB" and got.info["icc_profile"] == ref.info["icc_profile"]
    pil = Image.open(io.BytesIO(data))
    pil.thumbnail((400, 400))
    assert pil.decoderconfig == (2, 0)
    assert np.array_equal(np.asarray(got), np.asarray(pil))
    assert np.array_equal(np.asarray(got), S.thumbnail_of_file(data, 400))
