"""CPU: the OCR-input thumbnail's host geometry (bbocr_thumbnail_dims, bbocr_host_thumbnail_plan, bbocr_host_resample_coeffs,
bbocr_host_jpeg_qtables) against the installed Pillow, and the numpy restatement of the JPEG round trip (tests/jpeg_ref.py) against
Pillow's encoder + decode_file to the bit -- the semantics csrc/thumb.hip must reproduce."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_ref as ref


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def _pil_thumb_size(H, W, max_dim):
    from PIL import Image

    im = Image.new("L", (W, H))
    im.thumbnail((max_dim, max_dim))
    return im.size[1], im.size[0]


def _sizes():
    out = []
    for m in (1600, 2400):
        for a in (1, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 4 * m + 3):
            for b in (1, 7, 100, 966, m + 1, 2 * m + 1):
                out.append((a, b, m))
                out.append((b, a, m))
        for r in (2, 3, 10, 37, 100):                           # aspect ratios up to 1:100
            out.append((m * 2 + 5, (m * 2 + 5) // r, m))
            out.append(((m + 1) // r + 1, m + 1, m))
    out += [(4284, 5712, 1600), (5712, 4284, 2400), (6426, 8568, 1600), (8568, 6426, 2400), (1601, 1, 1600), (16001, 7, 1600)]
    return sorted(set(out))


def _plan(lib, H, W, m):
    oh, ow = C.c_int(), C.c_int()
    f, rb, bx = (C.c_int * 2)(), (C.c_int * 4)(), (C.c_float * 4)()
    assert lib.bbocr_host_thumbnail_plan(H, W, m, C.byref(oh), C.byref(ow), f, rb, bx) == 0
    return (oh.value, ow.value), tuple(f), tuple(rb), tuple(bx)


def test_thumbnail_dims_and_plan_match_pillow(lib):
    for H, W, m in _sizes():
        oh, ow = C.c_int(), C.c_int()
        assert lib.bbocr_thumbnail_dims(H, W, m, C.byref(oh), C.byref(ow)) == 0
        want = _pil_thumb_size(H, W, m)
        assert (oh.value, ow.value) == want, (H, W, m)
        size, f, rb, bx = _plan(lib, H, W, m)
        assert size == want
        if max(H, W) > m:
            fx, fy, box = ref.resize_plan(W, H, want[1], want[0])
            assert f == (fx, fy) and rb == (0, 0, W, H) and bx == box, (H, W, m)
            # Image.resize's own rule, stated once more from the Python source
            assert f == (int(W / want[1] / 2.0) or 1, int(H / want[0] / 2.0) or 1)


def test_plan_covers_unequal_reduce_factors(lib):
    _, f, _, _ = _plan(lib, 16001, 7, 1600)
    assert f[0] != f[1] and min(f) > 1
    _, f, _, _ = _plan(lib, 6426, 8568, 1600)
    assert f == (2, 2)


def test_errors(lib):
    oh, ow = C.c_int(), C.c_int()
    assert lib.bbocr_thumbnail_dims(0, 5, 1600, C.byref(oh), C.byref(ow)) != 0
    assert lib.bbocr_thumbnail_dims(5, 5, 0, C.byref(oh), C.byref(ow)) != 0
    assert lib.bbocr_thumbnail_dims(5, 5, 16, None, C.byref(ow)) != 0
    assert lib.bbocr_host_jpeg_qtables(101, (C.c_uint16 * 128)()) != 0
    assert lib.bbocr_host_jpeg_qtables(0, (C.c_uint16 * 128)()) != 0
    ks = C.c_int()
    assert lib.bbocr_host_resample_coeffs(0, 0.0, 1.0, 1, None, None, 0, C.byref(ks)) != 0


def _coeffs(lib, n_in, in0, in1, n_out):
    ks = C.c_int()
    assert lib.bbocr_host_resample_coeffs(n_in, in0, in1, n_out, None, None, 0, C.byref(ks)) == 0
    k = ks.value
    b, c = (C.c_int * (2 * n_out))(), (C.c_int * (n_out * k))()
    assert lib.bbocr_host_resample_coeffs(n_in, in0, in1, n_out, b, c, k, C.byref(ks)) == 0
    return np.array(b, np.int64).reshape(n_out, 2), np.array(c, np.int64).reshape(n_out, k)


@pytest.mark.parametrize("H,W,m", [(1601, 1200, 1600), (3201, 100, 1600), (6403, 1000, 1600), (100, 4803, 2400), (2000, 20, 1600),
                                   (1601, 1, 1600), (4001, 130, 2400), (7001, 33, 1600), (3001, 30, 1600), (3000, 30, 1600), (6403, 3, 1600)])
def test_resample_coeffs_give_pillow_thumbnail(lib, H, W, m):
    from PIL import Image

    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pil = Image.fromarray(img)
    pil.thumbnail((m, m))
    want = np.asarray(pil)
    (oh, ow), (fx, fy), _, box = _plan(lib, H, W, m)
    a = ref.reduce(img, fx, fy) if fx > 1 or fy > 1 else img
    rh, rw = a.shape[:2]
    bh, kh = _coeffs(lib, rw, box[0], box[2], ow)
    bv, kv = _coeffs(lib, rh, box[1], box[3], oh)
    rb, rk = ref.resample_coeffs(rw, box[0], box[2], ow)
    assert np.array_equal(bh, rb) and np.array_equal(kh, rk)
    if rh > 100 * rw:                                            # Pillow's vertical-first order for very tall images
        got = ref._apply(ref._apply(a, bv, kv, 0), bh, kh, 1)
    else:
        y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        t = ref._apply(a[y0:y1], bh, kh, 1)
        bv[:, 0] -= y0
        got = ref._apply(t, bv, kv, 0)
    assert np.array_equal(got, want)
    assert np.array_equal(ref.thumbnail(img, m), want)


@pytest.mark.parametrize("q", [1, 10, 50, 75, 90, 95, 100])
def test_qtables_match_pillow(lib, q):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=q)
    tabs = Image.open(io.BytesIO(buf.getvalue())).quantization
    out = (C.c_uint16 * 128)()
    assert lib.bbocr_host_jpeg_qtables(q, out) == 0
    assert list(out[:64]) == list(tabs[0]) and list(out[64:]) == list(tabs[1])
    l, c = ref.qtables(q)
    assert list(out[:64]) == l.ravel().tolist() and list(out[64:]) == c.ravel().tolist()


def test_pillow_saves_4_2_0():
    from PIL import Image, JpegImagePlugin

    buf = io.BytesIO()
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(buf, format="JPEG", quality=90)
    assert JpegImagePlugin.get_sampling(Image.open(io.BytesIO(buf.getvalue()))) == 2


def page(kind, h, w, seed=0):
    rng = np.random.default_rng(seed + 31 * h + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        return np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), (xx + yy) * 127 // max(h + w - 2, 1) + 64], -1).astype(np.uint8)
    img = np.full((h, w, 3), (236, 230, 222), np.uint8)                 # text-like: dark strokes on paper
    for _ in range(max(1, h * w // 400)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y:y + max(1, h // 20), x:x + int(rng.integers(1, max(2, w // 3)))] = rng.integers(0, 60, 3)
    return img


def _pil_round_trip(rgb, q):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=q)
    return decode_file(buf.getvalue())


SIDES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]


@pytest.mark.parametrize("q", [50, 90, 95, 100])
@pytest.mark.parametrize("kind", ["smooth", "text", "noise"])
def test_round_trip_matches_pillow(q, kind):
    for h in SIDES:
        for w in SIDES:
            img = page(kind, h, w)
            want_rgb, want_y = _pil_round_trip(img, q)
            got_rgb, got_y = ref.round_trip(img, q)
            assert np.array_equal(got_y, want_y), (h, w)
            assert np.array_equal(got_rgb, want_rgb), (h, w)


@pytest.mark.parametrize("q", [50, 90, 95, 100])
@pytest.mark.parametrize("kind", ["smooth", "text", "noise"])
def test_round_trip_matches_pillow_thumbnail_width(q, kind):
    for h, w in ((37, 966), (966, 21), (1, 966), (17, 966)):
        img = page(kind, h, w, seed=q)
        want_rgb, want_y = _pil_round_trip(img, q)
        got_rgb, got_y = ref.round_trip(img, q)
        assert np.array_equal(got_y, want_y) and np.array_equal(got_rgb, want_rgb), (h, w)


def test_gray_page_has_neutral_chroma():
    g = page("noise", 40, 56)[..., 0]
    rgb = np.repeat(g[:, :, None], 3, 2)
    y, cb, cr = ref.round_trip_ycc(rgb, 90)
    assert (cb == 128).all() and (cr == 128).all()
    assert np.array_equal(ref.round_trip(rgb, 90)[0], np.repeat(y[:, :, None], 3, 2))


def test_ocr_input_rule_matches_extractor():
    from bb_ocr_amd.extractor_batch import _ocr_input_array
    from bb_ocr_amd.reader import decode_file_ycc

    for pg in (page("text", 1700, 300)[..., 1], page("text", 1601, 40), page("text", 90, 120), page("smooth", 2000, 999)[..., 0]):
        for idx in (None, 3):
            m, q = (1600, 90) if idx is None else (2400, 95)
            kind, a, g = _ocr_input_array(pg, idx, decode_once=False)
            assert kind == "rgb"
            rgb, gray = ref.ocr_input(pg, m, q)
            assert np.array_equal(rgb, a) and np.array_equal(gray, g)
