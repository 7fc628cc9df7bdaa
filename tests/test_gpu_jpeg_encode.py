"""-m gpu: the model-input JPEG encoder on the device (csrc/jpegenc.hip: bbocr_jpeg_encode / bbocr_op_jpeg_encode_stage) against the numpy
restatement of tests/jpeg_encode_ref.py stage by stage, against the installed Pillow byte for byte, and through
``extractor_batch.encode_images_for_model`` against the reference function run inline."""
import base64
import ctypes as C
import functools
import io
import os
import threading

import numpy as np
import pytest
import torch

import jpeg_encode_ref as er
import jpeg_ref
import orient_ref
from test_jpeg_encode_cpu import CONTENTS, PHOTOS, QUALITIES, SHAPES, as_mode, content, pil_jpeg, reference_encode

pytestmark = pytest.mark.gpu

GRAY, BGR, RGB, YCC4, YCC3 = 0, 1, 2, 3, 4
MAX_BLOCK_BITS = 22 + 63 * 26


@functools.lru_cache(maxsize=None)
def ref_stages(kind, h, w, q, mode):
    """(page, coefficients, bit offsets, unstuffed scan) of the restatement, computed once for all tests"""
    a = as_mode(content(kind, h, w, seed=q), mode)
    comps = 3 if a.ndim == 3 else 1
    coef = er.coefficients(a, q)
    return a, coef, er.block_bits(coef, comps), er.pack(coef, comps)


def stage(reader, which, dev, layout, components, q):
    H, W = int(dev.shape[0]), int(dev.shape[1])
    blocks = -(-H // 8) * -(-W // 8) if components == 1 else 6 * -(-H // 16) * -(-W // 16)
    size = [blocks * 128, (blocks + 1) * 8, -(-blocks * MAX_BLOCK_BITS // 8)][which]
    dst = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device=dev.device)
    n = C.c_size_t()
    torch.cuda.current_stream(dev.device).synchronize()
    reader._check(reader._lib.bbocr_op_jpeg_encode_stage(reader._h, which, C.c_void_p(dev.data_ptr()), H, W, int(dev.stride(0)), layout, components,
                                                         q, C.c_void_p(dst.data_ptr()), size, C.byref(n)))
    out = dst.cpu().numpy()
    assert (out[max(n.value, size):] == 0xA5).all() and n.value <= size           # nothing is written behind the destination
    raw = out[:n.value].tobytes()
    return [lambda: np.frombuffer(raw, np.int16).reshape(-1, 64), lambda: np.frombuffer(raw, np.int64), lambda: raw][which]()


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_stages_equal_the_restatement(reader, mode, q):
    for h, w in SHAPES:
        for kind in CONTENTS:
            a, coef, bits, scan = ref_stages(kind, h, w, q, mode)
            dev = reader._to_dev(a)
            layout, comps = (RGB, 3) if mode == "RGB" else (GRAY, 1)
            got = stage(reader, 0, dev, layout, comps, q)
            assert np.array_equal(got, coef), (h, w, kind)                     # (the dummy blocks' DC terms among them)
            assert np.array_equal(stage(reader, 1, dev, layout, comps, q), bits), (h, w, kind)
            assert stage(reader, 2, dev, layout, comps, q) == scan, (h, w, kind)


def test_dummy_blocks_carry_the_dc_before_them(reader):
    for h, w in [(17, 33), (40, 24), (100, 131), (16, 7)]:
        dummy = er.dummy_blocks(h, w)
        assert dummy.any()
        got = stage(reader, 0, reader._to_dev(content("noise", h, w)), RGB, 3, 95)
        for b in np.flatnonzero(dummy):
            assert not got[b, 1:].any() and got[b, 0] == got[b - 1, 0], (h, w, b)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_encode_equals_pillow(reader, mode, q):
    for h, w in SHAPES:
        for kind in CONTENTS:
            a = as_mode(content(kind, h, w, seed=q), mode)
            got = reader.encode_jpeg(reader._to_dev(a), quality=q)             # defaults: RGB -> 3 components, gray -> Pillow's "L" save
            assert got == pil_jpeg(a, q), (h, w, kind)


@pytest.mark.parametrize("h,w", [(41, 57), (17, 33), (16, 7)])
def test_every_source_layout(reader, h, w):
    rgb = content("noise", h, w, seed=3)
    want = pil_jpeg(rgb, 88)
    assert reader.encode_jpeg(reader._to_dev(rgb), RGB, 88) == want
    assert reader.encode_jpeg(reader._to_dev(np.ascontiguousarray(rgb[:, :, ::-1])), BGR, 88) == want
    g = np.ascontiguousarray(rgb[:, :, 0])
    assert reader.encode_jpeg(reader._to_dev(g), GRAY, 88, components=1) == pil_jpeg(g, 88)
    assert reader.encode_jpeg(reader._to_dev(g), GRAY, 88, components=3) == pil_jpeg(np.repeat(g[:, :, None], 3, 2), 88)    # zero chroma blocks
    want = pil_jpeg(jpeg_ref.ycc_to_rgb(rgb[..., 0], rgb[..., 1], rgb[..., 2]), 88)                 # the same bytes read as YCbCr triples
    assert reader.encode_jpeg(reader._to_dev(rgb), YCC3, 88) == want
    ycc4 = np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], 2)
    assert reader.encode_jpeg(reader._to_dev(ycc4), YCC4, 88) == want
    assert reader.encode_jpeg(reader._to_dev(ycc4), quality=88) == want                             # four bytes per pixel: YCBCR4 by default
    assert reader.encode_jpeg(reader._to_dev(rgb), quality=88, comment=b"hello") == pil_jpeg(rgb, 88, comment=b"hello")


def test_strided_crop_of_a_larger_plane(reader):
    big = content("noise", 90, 120, seed=1)
    for plane, layout in ((np.ascontiguousarray(big[:, :, ::-1]), BGR), (np.ascontiguousarray(big[:, :, 2]), GRAY)):
        dev = reader._to_dev(plane)
        before = dev.clone()
        view = dev[5:46, 7:64]                                                 # 41 x 57, guard pixels on every side
        assert not view.is_contiguous()
        crop = np.ascontiguousarray(plane[5:46, 7:64])
        want = pil_jpeg(crop[:, :, ::-1] if layout == BGR else np.repeat(crop[:, :, None], 3, 2), 85)
        assert reader.encode_jpeg(view, layout, 85, components=3) == want
        assert torch.equal(dev, before)


def test_page_that_crosses_the_scan_tiles(reader):
    """640 x 480 noise at quality 100: 7,200 blocks in 29 size / packing tiles, and enough scan bytes for several hundred stuffing tiles,
    more than the one workgroup of the tile-sum scan takes in one step"""
    a = content("noise", 480, 640, seed=5)
    want = pil_jpeg(a, 100)
    head, stuffed, _ = er.split_file(want)
    scan = stuffed.replace(b"\xFF\x00", b"\xFF")
    assert len(scan) > 256 * 2048 and stuffed.count(b"\xFF\x00") > 1000
    dev = reader._to_dev(a)
    bits = stage(reader, 1, dev, RGB, 3, 100)
    assert len(bits) == 7201 and (np.diff(bits) > 0).all() and -(-int(bits[-1]) // 8) == len(scan)
    assert stage(reader, 2, dev, RGB, 3, 100) == scan
    got = reader.encode_jpeg(dev, RGB, 100)
    assert got == want
    assert reader.encode_jpeg(dev, RGB, 100) == got                            # and again: the same bytes


def _page_with_scan_end(aligned):
    """a small gray page whose unstuffed scan ends on a byte boundary (or does not), found with the restatement"""
    for seed in range(400):
        g = np.ascontiguousarray(content("noise", 9, 25, seed=seed)[:, :, 0])
        total = int(er.block_bits(er.coefficients(g, 90), 1)[-1])
        if (total % 8 == 0) == aligned:
            return g, total
    raise AssertionError("no such page")


@pytest.mark.parametrize("aligned", [True, False])
def test_final_byte_padding(reader, aligned):
    g, total = _page_with_scan_end(aligned)
    scan = er.pack(er.coefficients(g, 90), 1)
    assert len(scan) == -(-total // 8)
    dev = reader._to_dev(g)
    assert int(stage(reader, 1, dev, GRAY, 1, 90)[-1]) == total
    assert stage(reader, 2, dev, GRAY, 1, 90) == scan
    if not aligned:
        pad = 8 - total % 8
        assert scan[-1] & ((1 << pad) - 1) == (1 << pad) - 1                 # 1-bits
    assert reader.encode_jpeg(dev, GRAY, 90, components=1) == pil_jpeg(g, 90)


def test_encode_next_to_readtext_equals_serial(reader):
    from bb_ocr_amd import synth

    pages = [content(kind, 200 + 17 * k, 300 - 9 * k, seed=k) for k, kind in enumerate(("text", "noise", "smooth"))]
    devs = [reader._to_dev(p) for p in pages]
    serial = [reader.encode_jpeg(d, RGB, 88) for d in devs]
    assert serial == [pil_jpeg(p, 88) for p in pages]
    img = synth.page(21, width=640, height=480, lines=8)[0]
    want_text = reader.readtext(img)
    out, errs = [], []

    def run():
        try:
            for _ in range(4):
                out.append([reader.encode_jpeg(d, RGB, 88) for d in devs])
        except Exception as e:                                           # reported below
            errs.append(e)

    t = threading.Thread(target=run)
    t.start()
    texts = [reader.readtext(img) for _ in range(3)]
    t.join()
    assert not errs and len(out) == 4 and all(o == serial for o in out)
    assert all(r == want_text for r in texts)


def test_errors(reader):
    pg = reader._to_dev(content("text", 64, 48))
    g = reader._to_dev(np.ascontiguousarray(content("text", 64, 48)[:, :, 0]))
    ptr, gptr = C.c_void_p(pg.data_ptr()), C.c_void_p(g.data_ptr())
    lib = reader._lib
    cap = lib.bbocr_jpeg_encode_bound(64, 48, 3)
    out = np.empty(cap, np.uint8)
    o, n = C.c_void_p(out.ctypes.data), C.c_size_t()
    com = C.cast(C.c_char_p(b"abc"), C.c_void_p)
    f = lib.bbocr_jpeg_encode
    cases = [
        (ptr, 64, 48, 144, RGB, 3, 85, None, 0, o, cap, C.byref(n)),                # valid
        (None, 64, 48, 144, RGB, 3, 85, None, 0, o, cap, C.byref(n)),
        (ptr, 64, 48, 144, RGB, 3, 85, None, 0, None, cap, C.byref(n)),
        (ptr, 64, 48, 144, RGB, 3, 85, None, 0, o, cap, None),
        (ptr, 64, 48, 144, RGB, 3, 85, None, 3, o, cap, C.byref(n)),                # a comment length without a comment
        (ptr, 0, 48, 144, RGB, 3, 85, None, 0, o, cap, C.byref(n)),
        (ptr, 64, 0, 144, RGB, 3, 85, None, 0, o, cap, C.byref(n)),
        (ptr, 65536, 1, 3, RGB, 3, 85, None, 0, o, cap, C.byref(n)),                # H outside 1 .. 65535
        (ptr, 1, 65536, 3 * 65536, RGB, 3, 85, None, 0, o, cap, C.byref(n)),
        (ptr, 64, 48, 144, 5, 3, 85, None, 0, o, cap, C.byref(n)),                  # unknown layout
        (ptr, 64, 48, 144, -1, 3, 85, None, 0, o, cap, C.byref(n)),
        (ptr, 64, 48, 143, RGB, 3, 85, None, 0, o, cap, C.byref(n)),                # pitch shorter than a row
        (ptr, 64, 48, 144, RGB, 3, 0, None, 0, o, cap, C.byref(n)),                 # quality outside 1 .. 100
        (ptr, 64, 48, 144, RGB, 3, 101, None, 0, o, cap, C.byref(n)),
        (ptr, 64, 48, 144, RGB, 2, 85, None, 0, o, cap, C.byref(n)),                # components
        (ptr, 64, 48, 144, RGB, 1, 85, None, 0, o, cap, C.byref(n)),                # one component with a colour layout
        (ptr, 64, 48, 144, RGB, 3, 85, None, 0, o, cap - 1, C.byref(n)),            # capacity below the bound
        (ptr, 64, 48, 144, RGB, 3, 85, com, 65534, o, cap, C.byref(n)),             # comment too long
    ]
    for k, args in enumerate(cases):
        assert f(reader._h, *args) == (0 if k == 0 else -1), k
    assert f(None, *cases[0]) == -1
    assert f(reader._h, gptr, 64, 48, 48, GRAY, 1, 85, com, 3, o, cap, C.byref(n)) == 0
    assert out[:n.value].tobytes() == pil_jpeg(g.cpu().numpy(), 85, comment=b"abc")
    st = lib.bbocr_op_jpeg_encode_stage
    d = torch.empty(1 << 16, dtype=torch.uint8, device=reader.device)
    dp = C.c_void_p(d.data_ptr())
    assert st(reader._h, 0, ptr, 64, 48, 144, RGB, 3, 85, dp, 1 << 16, C.byref(n)) == 0 and n.value == 72 * 128
    assert st(reader._h, 3, ptr, 64, 48, 144, RGB, 3, 85, dp, 1 << 16, C.byref(n)) == -1
    assert st(reader._h, 0, ptr, 64, 48, 144, RGB, 3, 85, dp, 72 * 128 - 1, C.byref(n)) == -1
    assert st(reader._h, 0, ptr, 64, 48, 144, RGB, 3, 85, None, 1 << 16, C.byref(n)) == -1
    for bad in (pg.float(), pg.transpose(0, 1), pg.cpu(), pg[:, :, :2], "page"):
        with pytest.raises(ValueError):
            reader.encode_jpeg(bad)
    for kw in (dict(quality=0), dict(quality=101), dict(quality=85.0), dict(components=2), dict(components=1), dict(layout=9),
               dict(layout=GRAY), dict(comment=b"x" * 65534)):
        with pytest.raises(ValueError):
            reader.encode_jpeg(pg, **kw)
    # the context still works afterwards
    assert reader.encode_jpeg(pg, RGB, 85) == pil_jpeg(pg.cpu().numpy(), 85)


# ------------------------------------------------------------------------------------------------ the extractor's function
def _inline_reference(page_bgr_or_gray, max_dim, quality):
    """``_encode_image_for_model`` of the PNG the reference writes for a processed page (gray, or BGR as cv2 holds it)"""
    from PIL import Image

    a = page_bgr_or_gray
    img = Image.fromarray(np.ascontiguousarray(a if a.ndim == 2 else a[:, :, ::-1])).convert("RGB")
    img.thumbnail((max_dim, max_dim))
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=int(max(50, min(95, quality))))
    return base64.b64encode(buf.getvalue()).decode("utf-8")


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    from PIL import Image

    d = tmp_path_factory.mktemp("model_images")
    small = Image.open(PHOTOS[1]).resize((700, 900))
    plain = io.BytesIO()
    small.save(plain, "JPEG", quality=90)
    paths = {}
    for name, data in (("oriented.jpg", orient_ref.with_orientation(plain.getvalue(), 6)),):
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    paths["comment.jpg"] = os.path.join(d, "comment.jpg")
    small.save(paths["comment.jpg"], "JPEG", quality=90, comment=b"shelf 3, box 12")
    paths["s444.jpg"] = os.path.join(d, "s444.jpg")
    small.save(paths["s444.jpg"], "JPEG", quality=90, subsampling=0)
    return paths


@pytest.mark.parametrize("device_decode", [False, True])
def test_encode_images_for_model_photographs(reader, device_decode):
    from bb_ocr_amd import extractor_batch

    for paths in (PHOTOS, PHOTOS[::-1]):
        want = [reference_encode(p, *((2000, 88) if i == 0 else (3200, 95))) for i, p in enumerate(paths)]
        assert extractor_batch.encode_images_for_model(reader, paths, device_decode=device_decode) == want
    want = [reference_encode(p, 1600, 50) for p in PHOTOS]                    # a rule of the caller's, its quality clamped
    assert extractor_batch.encode_images_for_model(reader, PHOTOS, device_decode=device_decode, rule=lambda i: (1600, 20)) == want


@pytest.mark.parametrize("device_decode", [False, True])
def test_encode_images_for_model_with_crops(reader, device_decode):
    from bb_ocr_amd import extractor_batch

    kw = dict(edge_crop_percent=5, crop_for_ocr=True)
    pages = [extractor_batch.ocr_page_crop(reader, p, **kw) for p in PHOTOS]
    want = [_inline_reference(pg, *((2000, 88) if i == 0 else (3200, 95))) for i, pg in enumerate(pages)]
    assert extractor_batch.encode_images_for_model(reader, PHOTOS, device_decode=device_decode, **kw) == want
    pages = [extractor_batch.ocr_page_crop(reader, PHOTOS[1], use_preprocessing=True, edge_crop_percent=5)]
    assert pages[0].ndim == 2                                                  # the pre-processed page is gray: zero chroma blocks
    got = extractor_batch.encode_images_for_model(reader, PHOTOS[1:], use_preprocessing=True, edge_crop_percent=5, device_decode=device_decode)
    assert got == [_inline_reference(pages[0], 2000, 88)]


@pytest.mark.parametrize("device_decode", [False, True])
def test_encode_images_for_model_orientation_comment_and_refused_file(reader, model_files, device_decode):
    from bb_ocr_amd import extractor_batch
    from bb_ocr_amd.preprocess import _imread_bgr, central_edge_crop_box
    from bb_ocr_amd.reader import jpeg_plan

    rule = lambda i: (600, 88) if i == 0 else (3200, 95)                       # image 0 is thumbnailed, the others are not
    names = ["oriented.jpg", "comment.jpg", "s444.jpg", "oriented.jpg"]
    paths = [model_files[n] for n in names]
    with open(model_files["oriented.jpg"], "rb") as f:
        plan = jpeg_plan(f.read())
    assert plan.supported and plan.orientation == 6
    with open(model_files["s444.jpg"], "rb") as f:
        assert not jpeg_plan(f.read()).supported
    # the plain branch: Image.open does not transpose, and the comment is carried
    want = [reference_encode(p, *rule(i)) for i, p in enumerate(paths)]
    got = extractor_batch.encode_images_for_model(reader, paths, device_decode=device_decode, rule=rule)
    assert got == want
    assert b"shelf 3, box 12" in base64.b64decode(got[1]) and b"shelf 3, box 12" not in base64.b64decode(got[0])
    # the crop branch reads through cv2.imread: transposed, and the PNG on the way carries no comment
    want = []
    for i, p in enumerate(paths):
        bgr = _imread_bgr(p)
        assert bgr.shape[:2] == ((700, 900) if "oriented" in p else (900, 700))
        b = central_edge_crop_box(bgr.shape[0], bgr.shape[1], 5)
        want.append(_inline_reference(bgr[b[1]:b[3], b[0]:b[2]], *rule(i)))
    got = extractor_batch.encode_images_for_model(reader, paths, edge_crop_percent=5, device_decode=device_decode, rule=rule)
    assert got == want
    assert b"shelf 3, box 12" not in base64.b64decode(got[1])
    # a chain none of whose steps applies leaves the original file: the plain branch again
    assert central_edge_crop_box(900, 700, 45) is None
    got = extractor_batch.encode_images_for_model(reader, paths[:2], edge_crop_percent=45, device_decode=device_decode, rule=rule)
    assert got == [reference_encode(p, *rule(i)) for i, p in enumerate(paths[:2])]


def test_model_image_device_equals_host(reader):
    from bb_ocr_amd.preprocess import model_image_device, model_image_host

    bgr = content("text", 700, 500, seed=2)
    for page, layout in ((bgr, BGR), (np.ascontiguousarray(bgr[:, :, 1]), GRAY)):
        for max_dim, q in ((300, 88), (700, 95), (1600, 20)):
            assert model_image_device(reader, reader._to_dev(page), layout, max_dim, q) == model_image_host(page, max_dim, q)
