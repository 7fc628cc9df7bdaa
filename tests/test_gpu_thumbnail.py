"""-m gpu: the extractor's OCR-input down-scaling on the device (csrc/thumb.hip, bbocr_ocr_thumbnail / bbocr_op_thumbnail_stage) against
the installed Pillow and the numpy restatement of tests/jpeg_ref.py, stage by stage, through ``ocr_input_device`` and through
``extract_texts(device_thumbnail=True)``."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

import jpeg_ref as ref
from test_thumbnail_cpu import SIDES, page

pytestmark = pytest.mark.gpu

PHOTO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photos", "IMG_9684.JPG")
GRAY, BGR, RGB, YCC4, YCC3 = 0, 1, 2, 3, 4


def _stage(reader, stage, src_dev, layout, max_dim=16, quality=90):
    H, W = int(src_dev.shape[0]), int(src_dev.shape[1])
    oh, ow = C.c_int(), C.c_int()
    reader._check(reader._lib.bbocr_thumbnail_dims(H, W, max_dim, C.byref(oh), C.byref(ow)))
    h, w = (oh.value, ow.value) if stage == 0 else (H, W)
    dst = torch.full((h, w, 3), 7, dtype=torch.uint8, device=src_dev.device)
    gray = torch.full((h, w), 7, dtype=torch.uint8, device=src_dev.device)
    reader._check(reader._lib.bbocr_op_thumbnail_stage(reader._h, stage, C.c_void_p(src_dev.data_ptr()), H, W, int(src_dev.stride()[0]), layout,
                                                       max_dim, quality, C.c_void_p(dst.data_ptr()), C.c_void_p(gray.data_ptr()), C.byref(oh),
                                                       C.byref(ow)))
    assert (oh.value, ow.value) == (h, w)
    return dst.cpu().numpy(), gray.cpu().numpy()


def _pil_thumb(rgb, max_dim):
    from PIL import Image

    im = Image.fromarray(rgb)
    im.thumbnail((max_dim, max_dim))
    return np.asarray(im)


@pytest.mark.parametrize("H,W,m", [(17, 9, 16), (33, 5, 16), (65, 64, 16), (16, 300, 16), (1601, 3, 16), (100, 1, 16), (37, 41, 9),
                                   (1601, 1200, 1600), (3201, 2000, 1600), (6403, 1000, 1600), (100, 4803, 2400), (2000, 20, 1600),
                                   (3001, 30, 1600), (16001, 7, 1600), (12, 12, 16)])
def test_stage0_thumbnail_equals_pillow(reader, H, W, m):
    rgb = page("noise", H, W)
    dev = reader._to_dev(rgb)
    got, _ = _stage(reader, 0, dev, RGB, m)
    assert np.array_equal(got, _pil_thumb(rgb, m))
    got, _ = _stage(reader, 0, reader._to_dev(np.ascontiguousarray(rgb[:, :, ::-1])), BGR, m)
    assert np.array_equal(got, _pil_thumb(rgb, m))
    g = np.ascontiguousarray(rgb[:, :, 1])
    got, _ = _stage(reader, 0, reader._to_dev(g), GRAY, m)
    assert np.array_equal(got, _pil_thumb(np.repeat(g[:, :, None], 3, 2), m))


@pytest.mark.parametrize("q", [50, 90, 95, 100])
@pytest.mark.parametrize("kind", ["smooth", "text", "noise"])
def test_stage1_stage2_round_trip(reader, q, kind):
    sizes = [(h, w) for h in SIDES for w in SIDES] + [(37, 966), (966, 21), (1, 966), (1600, 966)]
    for h, w in sizes:
        img = page(kind, h, w, seed=q)
        dev = reader._to_dev(img)
        want_rgb, want_y = ref.round_trip(img, q)
        got_rgb, got_y = _stage(reader, 1, dev, RGB, quality=q)
        assert np.array_equal(got_y, want_y), (h, w)
        assert np.array_equal(got_rgb, want_rgb), (h, w)
        got_ycc, _ = _stage(reader, 2, dev, RGB, quality=q)
        assert np.array_equal(got_ycc, np.stack(ref.round_trip_ycc(img, q), -1)), (h, w)
        g = np.ascontiguousarray(img[:, :, 0])                            # the gray fast path (Y blocks only)
        grgb, gy = _stage(reader, 1, reader._to_dev(g), GRAY, quality=q)
        wrgb, wy = ref.round_trip(np.repeat(g[:, :, None], 3, 2), q)
        assert np.array_equal(gy, wy) and np.array_equal(grgb, wrgb), (h, w)


def _host_ocr_input(page_host, idx):
    from bb_ocr_amd.extractor_batch import _ocr_input_array

    kind, rgb, gray = _ocr_input_array(page_host, idx, decode_once=False)
    assert kind == "rgb"
    return rgb, gray


def _check_ocr_input(reader, page_dev, page_host, idx):
    from bb_ocr_amd.preprocess import ocr_input_device

    rgb, gray = ocr_input_device(reader, page_dev, idx)
    want_rgb, want_gray = _host_ocr_input(page_host, idx)
    assert np.array_equal(rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(gray.cpu().numpy(), want_gray)


@pytest.mark.parametrize("H,W", [(1700, 1200), (1601, 40), (900, 2500), (2401, 100), (300, 200), (1600, 1600), (2400, 1000), (5000, 3001)])
@pytest.mark.parametrize("idx", [None, 0, 3])
def test_ocr_input_device_equals_host(reader, H, W, idx):
    bgr = page("text", H, W, seed=idx or 0)
    _check_ocr_input(reader, reader._to_dev(bgr), bgr, idx)
    g = np.ascontiguousarray(bgr[:, :, 1])
    _check_ocr_input(reader, reader._to_dev(g), g, idx)


def test_ocr_input_device_strided_crop(reader):
    from bb_ocr_amd.preprocess import central_edge_crop_box

    bgr = page("text", 2600, 2100, seed=5)
    dev = reader._to_dev(bgr)
    b = central_edge_crop_box(2600, 2100, 15)
    view = dev[b[1]:b[3], b[0]:b[2]]
    assert not view.is_contiguous()
    for idx in (0, 2):
        _check_ocr_input(reader, view, np.ascontiguousarray(bgr[b[1]:b[3], b[0]:b[2]]), idx)
    g = reader._to_dev(np.ascontiguousarray(bgr[:, :, 0]))
    _check_ocr_input(reader, g[b[1]:b[3], b[0]:b[2]], np.ascontiguousarray(bgr[b[1]:b[3], b[0]:b[2], 0]), 0)


def test_ocr_input_device_f2_page_reduce_2(reader):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preprocess_bgr_device

    img, _ = synth.page(3, width=1280, height=960, lines=12)
    big = np.asarray(Image.fromarray(img).resize((4400, 3300), Image.BICUBIC))
    f2 = preprocess_bgr_device(reader, reader._to_dev(np.ascontiguousarray(big[:, :, ::-1])))
    assert f2.shape == (4950, 6600)
    assert int(6600 / 1600 / 2.0) == 2                                   # the reduce step is taken
    _check_ocr_input(reader, f2, f2.cpu().numpy(), 0)


def test_ocr_input_ycc_device_photo(reader):
    from bb_ocr_amd.extractor_batch import _ocr_input
    from bb_ocr_amd.preprocess import ocr_input_ycc_device
    from bb_ocr_amd.reader import decode_file_ycc

    ycc = decode_file_ycc(PHOTO, padded=True)
    for idx in (0, 1):
        rgb, gray = ocr_input_ycc_device(reader, reader._to_dev(ycc), idx)
        kind, want_rgb, want_gray = _ocr_input(PHOTO, idx, decode_once=False)
        assert kind == "rgb"
        if idx == 0:
            assert tuple(rgb.shape) == (1600, 966, 3)
        assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(gray.cpu().numpy(), want_gray)
    tight = np.ascontiguousarray(ycc[:, :, :3])                         # the [H,W,3] decode (no zero-copy export)
    rgb, gray = ocr_input_ycc_device(reader, reader._to_dev(tight), 0)
    _, want_rgb, want_gray = _ocr_input(PHOTO, 0, decode_once=False)
    assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(gray.cpu().numpy(), want_gray)


@pytest.fixture(scope="module")
def mixed_files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("thumb_pages")
    paths = []
    for k, (w, h, scale) in enumerate([(640, 480, 1), (1280, 960, 2), (960, 1280, 2), (1280, 960, 1)]):
        img, _ = synth.page(40 + k, width=w, height=h, lines=10)
        if scale > 1:
            img = np.asarray(Image.fromarray(img).resize((w * 2 + 1, h * 2 + 3 * k), Image.BICUBIC))
        p = os.path.join(d, f"p{k}.jpg")
        Image.fromarray(img).save(p, quality=92)
        paths.append(p)
    img, _ = synth.page(50, width=1700, height=1000, lines=10)
    p = os.path.join(d, "p4.png")
    Image.fromarray(img).save(p)
    paths.append(p)
    paths.append(PHOTO)
    return paths


def test_extract_texts_device_thumbnail(reader, mixed_files):
    from bb_ocr_amd import extractor_batch

    idx = list(range(len(mixed_files)))
    want = extractor_batch.extract_texts(reader, mixed_files, idx)
    got = extractor_batch.extract_texts(reader, mixed_files, idx, device_thumbnail=True)
    assert got == want
    # the pages out of order: the cover rule follows the index
    paths = mixed_files[::-1]
    assert extractor_batch.extract_texts(reader, paths, device_thumbnail=True) == extractor_batch.extract_texts(reader, paths)


def test_extract_texts_device_thumbnail_with_crops(reader, mixed_files):
    from bb_ocr_amd import extractor_batch

    files = [mixed_files[1], mixed_files[2], mixed_files[5], mixed_files[0]]
    kw = dict(use_preprocessing=True, edge_crop_percent=10, crop_for_ocr=True)
    want = extractor_batch.extract_texts(reader, files, [0, 1, 2, 3], **kw)
    got = extractor_batch.extract_texts(reader, files, [0, 1, 2, 3], device_thumbnail=True, **kw)
    assert got == want
    kw = dict(use_preprocessing=False, crop_for_ocr=True)
    assert extractor_batch.extract_texts(reader, files, device_thumbnail=True, **kw) == extractor_batch.extract_texts(reader, files, **kw)


def test_extract_texts_device_pages_are_retried_page_by_page(reader, tmp_path):
    """A batch of pages that live on the card (kind "dev") whose device call fails is read again page by page, from slices of the same
    tensors: the texts are those of the call that did not fail."""
    from PIL import Image

    from bb_ocr_amd import extractor_batch, synth

    paths = []
    for k in range(3):
        paths.append(tmp_path / f"p{k}.png")
        Image.fromarray(synth.page(60 + k, width=400, height=300, lines=5, margin=24)[0]).save(paths[-1])

    class FailsOnce:
        """the reader, except that its first device call holding more than one page raises"""

        def __init__(self):
            self.sizes = []

        def __getattr__(self, name):
            return getattr(reader, name)

        def readtext_device(self, rgb_dev, gray_dev=None, **kw):
            self.sizes.append(int(rgb_dev.shape[0]))
            if rgb_dev.shape[0] > 1 and len(self.sizes) == 1:
                raise RuntimeError("boom")
            return reader.readtext_device(rgb_dev, gray_dev, **kw)

    kw = dict(edge_crop_percent=5, device_thumbnail=True)
    want = extractor_batch.extract_texts(reader, paths, **kw)
    proxy = FailsOnce()
    assert extractor_batch.extract_texts(proxy, paths, **kw) == want
    assert proxy.sizes == [3, 1, 1, 1]
    assert all(want[k] for k in range(3)) and len(set(want.values())) == 3        # (a retry that mixed the pages up would show)


def test_errors(reader):
    from bb_ocr_amd.preprocess import ocr_input_device

    pg = reader._to_dev(page("text", 64, 48))
    ptr = C.c_void_p(pg.data_ptr())
    rgb = torch.empty((64, 48, 3), dtype=torch.uint8, device=reader.device)
    gray = torch.empty((64, 48), dtype=torch.uint8, device=reader.device)
    pr, pgr = C.c_void_p(rgb.data_ptr()), C.c_void_p(gray.data_ptr())
    oh, ow = C.c_int(), C.c_int()
    f = reader._lib.bbocr_ocr_thumbnail
    cases = [
        (ptr, 64, 48, 144, BGR, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),           # valid
        (None, 64, 48, 144, BGR, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),
        (ptr, 64, 48, 144, BGR, 1600, 90, None, pgr, C.byref(oh), C.byref(ow)),
        (ptr, 64, 48, 144, BGR, 1600, 90, pr, None, C.byref(oh), C.byref(ow)),
        (ptr, 64, 48, 144, BGR, 1600, 90, pr, pgr, None, C.byref(ow)),
        (ptr, 64, 48, 144, 5, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),             # bad layout
        (ptr, 64, 48, 144, -1, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),
        (ptr, 64, 48, 143, BGR, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),           # pitch < a row
        (ptr, 64, 48, 144, BGR, 0, 90, pr, pgr, C.byref(oh), C.byref(ow)),              # max_dim < 1
        (ptr, 64, 48, 144, BGR, 1600, 101, pr, pgr, C.byref(oh), C.byref(ow)),          # quality > 100
        (ptr, 0, 48, 144, BGR, 1600, 90, pr, pgr, C.byref(oh), C.byref(ow)),
    ]
    for k, args in enumerate(cases):
        assert f(reader._h, *args) == (0 if k == 0 else -1), k
    assert f(None, *cases[0]) == -1
    st = reader._lib.bbocr_op_thumbnail_stage
    assert st(reader._h, 3, ptr, 64, 48, 144, BGR, 16, 90, pr, pgr, C.byref(oh), C.byref(ow)) == -1
    assert st(reader._h, 1, ptr, 64, 48, 144, BGR, 16, 90, pr, pgr, C.byref(oh), C.byref(ow)) == -1   # stages 1 / 2: gray or RGB
    assert st(reader._h, 1, ptr, 64, 48, 144, RGB, 16, 0, pr, pgr, C.byref(oh), C.byref(ow)) == -1    # and a quality
    with pytest.raises(ValueError):
        ocr_input_device(reader, pg.float())
    with pytest.raises(ValueError):
        ocr_input_device(reader, pg.transpose(0, 1))
    # the context still works afterwards
    _check_ocr_input(reader, pg, pg.cpu().numpy(), 0)


def test_concurrent_calls_equal_serial(reader):
    from bb_ocr_amd.preprocess import ocr_input_device

    pages = [page("text", 2000 + 97 * k, 1500 - 61 * k, seed=k) for k in range(4)]
    devs = [reader._to_dev(p) for p in pages]
    serial = [tuple(t.cpu().numpy() for t in ocr_input_device(reader, d, k % 2)) for k, d in enumerate(devs)]
    out = [None] * 4
    errs = []

    def run(k):
        try:
            for _ in range(3):
                out[k] = tuple(t.cpu().numpy() for t in ocr_input_device(reader, devs[k], k % 2))
        except Exception as e:                                           # reported below
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    for a, b in zip(out, serial):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
