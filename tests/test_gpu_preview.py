"""-m gpu: the processing trace's previews made on the device (preprocess.preview_device, extractor_batch.trace_previews,
bbocr_thumbnail_box) against the installed Pillow: the resize with a fractional box pixel for pixel, the previews as strings."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_ref as R
import jpeg_scaled_ref as S
from test_jpeg_decode_cpu import PHOTOS, picture, save
from test_jpeg_scaled_cpu import F2_CASES, GOLDEN

pytestmark = pytest.mark.gpu


def strided(reader, a, extra=(3, 7)):
    """the page as a view of a larger device tensor: rows further apart than their pixels"""
    h, w = a.shape[:2]
    big = torch.full((h + extra[0], w + extra[1]) + a.shape[2:], 201, dtype=torch.uint8, device=reader.device)
    big[:h, :w] = torch.from_numpy(np.ascontiguousarray(a)).to(reader.device)
    return big[:h, :w]


def test_thumbnail_box_equals_pillows_resize_with_a_box(reader):
    from PIL import Image

    from bb_ocr_amd.preprocess import PAGE_GRAY, PAGE_RGB, PAGE_YCBCR4, thumbnail_box_device

    rng = np.random.default_rng(11)
    reduced = 0
    for (h, w, m) in F2_CASES:
        ow, oh = R.thumbnail_size(w, h, m)
        for s in (1, 2, 4):
            sh, sw = S.scaled_dims(h, w, s)
            fx, fy, _ = S.boxed_resize_plan(ow, oh, w / s, h / s)
            reduced += fx > 1 or fy > 1
            for ch, layout in ((1, PAGE_GRAY), (3, PAGE_RGB)):
                a = rng.integers(0, 256, (sh, sw, ch), dtype=np.uint8)
                a = a[:, :, 0] if ch == 1 else a
                want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC, box=(0, 0, w / s, h / s), reducing_gap=2.0))
                got = thumbnail_box_device(reader, strided(reader, a), layout, oh, ow, w / s, h / s).cpu().numpy()
                assert np.array_equal(got, want), (h, w, m, s, ch)
    assert reduced >= 8
    # Pillow's padded YCbCr pixels: libjpeg's RGB first
    h, w, m, s = 301, 203, 33, 2
    ow, oh = R.thumbnail_size(w, h, m)
    sh, sw = S.scaled_dims(h, w, s)
    ycc = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
    rgb = R.ycc_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2])
    want = np.asarray(Image.fromarray(rgb).resize((ow, oh), Image.BICUBIC, box=(0, 0, w / s, h / s), reducing_gap=2.0))
    got = thumbnail_box_device(reader, strided(reader, ycc), PAGE_YCBCR4, oh, ow, w / s, h / s).cpu().numpy()
    assert np.array_equal(got, want)
    # a box that does not end inside the last pixel is refused
    with pytest.raises(Exception):
        thumbnail_box_device(reader, strided(reader, ycc), PAGE_YCBCR4, oh, ow, sw - 1.5, float(sh))


def icc_profile():
    from PIL import Image

    return Image.open(os.path.join(GOLDEN, "trace", "example_15_image2_original.png")).info["icc_profile"]


def test_preview_of_files_equals_the_host_preview(reader, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preview_device, preview_host
    from bb_ocr_amd.reader import jpeg_plan

    page = Image.fromarray(synth.page(61, width=1900, height=1300, lines=12, margin=40, colour=True)[0])
    exif = Image.Exif()
    exif[0x0112] = 6
    cases = {
        "icc+exif6": (save(page, quality=90, icc_profile=icc_profile(), exif=exif), 800),          # draft scale 1, reduce step
        "icc+exif6-draft2": (save(page, quality=90, icc_profile=icc_profile(), exif=exif), 300),    # draft scale 2: 950 x 650, box ends at 650.0
        "odd-draft4": (save(picture("gradient", 1901, 1299, "RGB"), quality=85), 150),                # draft scale 4, fractional box
        "grey": (save(page.convert("L"), quality=90), 500),
        "grey-draft2": (save(page.convert("L"), quality=90, icc_profile=icc_profile()), 301),
        "small": (save(picture("noise", 640, 480, "RGB"), quality=90), 800),                          # at most 800 px: the decode itself
        "small-grey": (save(picture("noise", 333, 222, "L"), quality=90), 800),
        "photo": (open(PHOTOS[0], "rb").read(), 200),                                                 # draft scale 2
    }
    assert jpeg_plan(cases["icc+exif6"][0]).orientation == 6
    for name, (data, m) in cases.items():
        assert jpeg_plan(data).supported, name
        want = preview_host(data, m)
        assert preview_device(reader, data, m) == want, name
        assert preview_device(reader, data, m, device_decode=False) == want, name
    pil = Image.open(io.BytesIO(cases["photo"][0]))
    pil.thumbnail((200, 200))
    assert pil.decoderconfig == (2, 0)
    path = str(tmp_path / "page.jpg")
    open(path, "wb").write(cases["icc+exif6"][0])
    assert preview_device(reader, path) == preview_host(path)
    # the host route: a PNG path, a file of a chroma class, a progressive file
    png = str(tmp_path / "page.png")
    page.save(png, "PNG")
    assert preview_device(reader, png) == preview_host(png)
    for kw in (dict(subsampling=0), dict(progressive=True)):
        data = save(page, quality=90, **kw)
        assert not jpeg_plan(data).supported and preview_device(reader, data, 300) == preview_host(data, 300)


def test_preview_of_device_pages_equals_the_host_preview(reader):
    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preprocess_bgr_device, preview_device, preview_host

    bgr = np.ascontiguousarray(synth.page(62, width=1100, height=820, lines=10, margin=32, colour=True)[0][:, :, ::-1])
    dev = reader._to_dev(bgr)
    gray = preprocess_bgr_device(reader, dev)                                  # the f2 output: 1230 x 1650, gray
    assert gray.ndim == 2 and max(gray.shape) > 800
    assert preview_device(reader, gray) == preview_host(gray.cpu().numpy())
    crop = dev[40:790, 100:1050]                                               # a strided BGR crop view above 800 px
    assert not crop.is_contiguous()
    assert preview_device(reader, crop) == preview_host(np.ascontiguousarray(bgr[40:790, 100:1050]))
    small = dev[10:500, 20:700]                                                # at most 800 px: the page itself
    assert preview_device(reader, small) == preview_host(np.ascontiguousarray(bgr[10:500, 20:700]))
    assert preview_device(reader, gray[5:605, 9:709], 800) == preview_host(gray[5:605, 9:709].cpu().numpy(), 800)


def test_trace_previews_equal_the_reference_calls(reader, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.extractor_batch import ocr_page_crop, trace_previews
    from bb_ocr_amd.preprocess import _imread_bgr, auto_crop_box_device, central_edge_crop_box, preprocess_bgr_device, preview_host

    path = str(tmp_path / "cover.jpg")
    Image.fromarray(synth.page(63, width=1280, height=960, lines=8, margin=150)[0]).save(path, "JPEG", quality=90)
    kw = dict(use_preprocessing=True, edge_crop_percent=4.0, crop_for_ocr=True, crop_margin=32)
    got = trace_previews(reader, [path], **kw)
    assert len(got) == 1
    # the four calls of the reference, restated step by step without ocr_page_crop's `pages`: the file itself, then the page each step
    # leaves (the PNG the reference writes of it) -- cv2.imread's page pre-processed, its central crop, the auto-crop of that
    pre = preprocess_bgr_device(reader, reader._to_dev(_imread_bgr(path))).cpu().numpy()
    assert pre.shape == (1440, 1920)
    b = central_edge_crop_box(pre.shape[0], pre.shape[1], 4.0)
    assert b == (77, 58, 1843, 1382)
    edge = np.ascontiguousarray(pre[b[1]:b[3], b[0]:b[2]])
    a = auto_crop_box_device(reader, reader._to_dev(edge), 32)
    assert a is not None
    auto = np.ascontiguousarray(edge[a[1]:a[3], a[0]:a[2]])
    want = {"original_b64": preview_host(path), "preprocessed_b64": preview_host(pre), "edge_cropped_b64": preview_host(edge),
            "auto_cropped_b64": preview_host(auto)}
    assert got[0] == want
    # and the pages ocr_page_crop hands out are those pages, the last one its return value
    pages = {}
    last = ocr_page_crop(reader, path, on_device=True, pages=pages, **kw)
    assert list(pages) == ["preprocess", "edge_crop", "auto_crop"]
    for step, page in zip(pages, (pre, edge, auto)):
        assert np.array_equal(pages[step].cpu().numpy(), page), step
    assert pages["auto_crop"].data_ptr() == last.data_ptr() and pages["auto_crop"].shape == last.shape
    assert trace_previews(reader, [path], device_decode=False, **kw)[0] == want
    assert trace_previews(reader, [path]) == [{"original_b64": want["original_b64"]}]
