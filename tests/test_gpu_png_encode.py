"""-m gpu: the device PNG writer (bbocr_png_encode, bbocr_op_deflate, bbocr_op_png_stage; csrc/pngenc.hip) against tests/png_ref.py byte
for byte -- the filtered stream, the per-chunk histograms, code lengths and offsets, the zlib stream, the file -- and against Pillow pixel for
pixel; then the opt-in png="device" of preprocess.preview_device and extractor_batch.trace_previews."""
import base64
import ctypes as C
import io
import zlib

import numpy as np
import pytest
import torch

import png_ref as P
from test_png_ref_cpu import icc_profile, page_cases, page_model, same_image, stream_cases, stream_model

pytestmark = pytest.mark.gpu


def strided(reader, a, extra=(3, 7)):
    """the page as a view of a larger device tensor: rows further apart than their pixels"""
    h, w = a.shape[:2]
    big = torch.full((h + extra[0], w + extra[1]) + a.shape[2:], 201, dtype=torch.uint8, device=reader.device)
    big[:h, :w] = torch.from_numpy(np.ascontiguousarray(a)).to(reader.device)
    return big[:h, :w]


def device_page(reader, name):
    """(strided device tensor, PAGE_* layout) of a page case: a BGR case holds the pixels swapped"""
    from bb_ocr_amd import _lib

    img, layout, _ = page_cases()[name]
    code = {"gray": _lib.PAGE_GRAY, "rgb": _lib.PAGE_RGB, "bgr": _lib.PAGE_BGR}[layout]
    return strided(reader, img[..., ::-1] if layout == "bgr" else img), code


def device_bytes(reader, data, shift=0):
    """the byte string on the device, `shift` bytes behind an allocation's start"""
    t = torch.zeros(len(data) + shift + 1, dtype=torch.uint8, device=reader.device)
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(reader.device)
    return t[shift:shift + len(data)]


def png_stage(reader, stage, src, layout=0, dtype=np.uint8, room=None):
    """bbocr_op_png_stage -> its output as a numpy array: stage 0 of a page tensor, stages 1 .. 3 of a 1-D byte tensor"""
    if stage == 0:
        H, W, pitch, n = src.shape[0], src.shape[1], src.stride(0), 0
        room = H * (1 + W * (1 if src.ndim == 2 else 3))
    else:
        H = W = pitch = 0
        n = src.numel()
        chunks = -(-n // P.CHUNK)
        room = {1: chunks * P.HIST_ROW * 4, 2: chunks * P.REC, 3: (chunks + 1) * 8}[stage]
    dst = torch.full((room + 16,), 0xEE, dtype=torch.uint8, device=reader.device)
    got = C.c_size_t()
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_op_png_stage(reader._h, stage, C.c_void_p(src.data_ptr()) if src.numel() else None, H, W, pitch, layout, n,
                                                 C.c_void_p(dst.data_ptr()), room, C.byref(got)))
    assert got.value == room and bool((dst[room:] == 0xEE).all())
    return dst[:room].cpu().numpy().view(dtype)


def check_stream_stages(reader, dev, chunks, data):
    hist, rec, off = P.stage_arrays(data, chunks)
    assert np.array_equal(png_stage(reader, 1, dev, dtype=np.uint32).reshape(-1, P.HIST_ROW), hist)
    assert np.array_equal(png_stage(reader, 2, dev).reshape(-1, P.REC), rec)
    assert np.array_equal(png_stage(reader, 3, dev, dtype=np.int64), off)


@pytest.mark.parametrize("name", list(page_cases()))
def test_page_stages_and_file_equal_the_model(reader, name):
    img, _, icc = page_cases()[name]
    want, chunks, stream = page_model(name)
    page, layout = device_page(reader, name)
    assert not page.is_contiguous() or page.shape[0] == 1
    assert png_stage(reader, 0, page, layout).tobytes() == stream
    check_stream_stages(reader, device_bytes(reader, stream), chunks, stream)
    got = reader.encode_png(page, layout, icc_profile=icc)
    same_image(got, img, icc)
    assert zlib.decompress(P.idat_payload(got)) == stream
    assert got == want
    assert reader.encode_png(page, layout, icc_profile=icc) == got                        # the same bytes from call to call


@pytest.mark.parametrize("name", list(stream_cases()))
def test_deflate_stages_and_stream_equal_the_model(reader, name):
    data = stream_cases()[name]
    want, chunks = stream_model(name)
    for shift in (0, 1):                                                                   # an allocation's start, and an odd address
        dev = device_bytes(reader, data, shift)
        check_stream_stages(reader, dev, chunks, data)
        got = reader.deflate_device(dev)
        assert zlib.decompress(got) == data
        assert got == want


def test_default_layouts_and_refusals(reader):
    from bb_ocr_amd import _lib

    rng = np.random.default_rng(5)
    g, rgb = rng.integers(0, 256, (5, 9), dtype=np.uint8), rng.integers(0, 256, (5, 9, 3), dtype=np.uint8)
    same_image(reader.encode_png(reader._to_dev(g)), g, None)                              # [H,W]: gray; [H,W,3]: RGB
    same_image(reader.encode_png(reader._to_dev(rgb)), rgb, None)
    same_image(reader.encode_png(reader._to_dev(rgb), _lib.PAGE_BGR), rgb[..., ::-1], None)
    four = reader._to_dev(rng.integers(0, 256, (5, 9, 4), dtype=np.uint8))
    for kw in (dict(), dict(layout=_lib.PAGE_YCBCR4)):
        with pytest.raises(ValueError):
            reader.encode_png(four, **kw)
    with pytest.raises(ValueError):
        reader.encode_png(reader._to_dev(rgb), _lib.PAGE_YCBCR3)
    # the C entry point itself: a 4-byte layout, a pitch shorter than a row, a capacity below the bound -- BBOCR_ERR_ARG, nothing written
    lib, dev = reader._lib, reader._to_dev(rgb)
    cap = int(lib.bbocr_png_encode_bound(5, 9, 3, 0))
    assert cap == P.encode_bound(5, 9, 3) and lib.bbocr_png_encode_bound(5, 9, 3, 70000) == P.encode_bound(5, 9, 3, 70000)
    assert lib.bbocr_png_encode_bound(0, 9, 3, 0) == 0 and lib.bbocr_png_encode_bound(5, 9, 4, 0) == 0
    out = np.full(cap, 0xEE, np.uint8)
    n = C.c_size_t()
    call = lambda layout, pitch, capacity: lib.bbocr_png_encode(reader._h, C.c_void_p(dev.data_ptr()), 5, 9, pitch, layout, None, 0,
                                                                C.c_void_p(out.ctypes.data), capacity, C.byref(n))
    assert call(_lib.PAGE_YCBCR4, 36, cap) == -1 and call(_lib.PAGE_YCBCR3, 27, cap) == -1
    assert call(_lib.PAGE_RGB, 26, cap) == -1 and call(_lib.PAGE_RGB, 27, cap - 1) == -1
    assert bool((out == 0xEE).all())
    assert call(_lib.PAGE_RGB, 27, cap) == 0
    same_image(out[:n.value].tobytes(), rgb, None)
    with pytest.raises(ValueError):
        reader.deflate_device(reader._to_dev(rgb))


def decoded(url):
    from PIL import Image

    assert url.startswith("data:image/png;base64,")
    im = Image.open(io.BytesIO(base64.b64decode(url.split(",", 1)[1])))
    return im.mode, im.size, np.asarray(im), im.info.get("icc_profile")


def same_preview(a, b):
    da, db = decoded(a), decoded(b)
    assert da[0] == db[0] and da[1] == db[1] and np.array_equal(da[2], db[2]) and da[3] == db[3]


def test_preview_with_the_device_png_decodes_to_the_host_preview(reader, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preview_device, preview_host
    from test_jpeg_decode_cpu import picture, save

    page = Image.fromarray(synth.page(61, width=1900, height=1300, lines=12, margin=40, colour=True)[0])
    exif = Image.Exif()
    exif[0x0112] = 6
    cases = {
        "icc+exif6": (save(page, quality=90, icc_profile=icc_profile(), exif=exif), 800),
        "grey": (save(page.convert("L"), quality=90), 500),
        "small": (save(picture("noise", 640, 480, "RGB"), quality=90), 800),
    }
    monkeypatch.delenv("BBOCR_PNG_DEVICE", raising=False)
    for name, (data, m) in cases.items():
        want = preview_host(data, m)
        info = {}
        got = preview_device(reader, data, m, png="device", info=info)
        assert info["route"] == "device-jpeg" and got != want, name
        same_preview(got, want)
        assert preview_device(reader, data, m, png="pillow") == want and preview_device(reader, data, m) == want, name
    assert decoded(preview_device(reader, cases["icc+exif6"][0], 800, png="device"))[3] == icc_profile()
    assert decoded(preview_device(reader, cases["grey"][0], 500, png="device"))[0] == "L"
    # the environment sets the default of a call made without the argument; the argument wins
    data, m = cases["small"]
    monkeypatch.setenv("BBOCR_PNG_DEVICE", "1")
    assert preview_device(reader, data, m) == preview_device(reader, data, m, png="device") != preview_host(data, m)
    assert preview_device(reader, data, m, png="pillow") == preview_host(data, m)
    with pytest.raises(ValueError):
        preview_device(reader, data, m, png="zlib")
    # a page already on the card (a strided BGR crop above 800 px), and the host route, which keeps Pillow
    monkeypatch.delenv("BBOCR_PNG_DEVICE")
    bgr = np.ascontiguousarray(synth.page(62, width=1100, height=820, lines=10, margin=32, colour=True)[0][:, :, ::-1])
    crop = reader._to_dev(bgr)[40:790, 100:1050]
    same_preview(preview_device(reader, crop, png="device"), preview_host(np.ascontiguousarray(bgr[40:790, 100:1050])))
    prog = save(page, quality=90, progressive=True)
    assert preview_device(reader, prog, 300, png="device") == preview_host(prog, 300)


def test_trace_previews_with_the_device_png(reader, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.extractor_batch import trace_previews

    path = str(tmp_path / "cover.jpg")
    Image.fromarray(synth.page(63, width=1280, height=960, lines=8, margin=150)[0]).save(path, "JPEG", quality=90)
    kw = dict(edge_crop_percent=4.0)
    want = trace_previews(reader, [path], png="pillow", **kw)
    got = trace_previews(reader, [path], png="device", **kw)
    assert len(got) == 1 and list(got[0]) == list(want[0]) == ["original_b64", "edge_cropped_b64"]
    for key in want[0]:
        assert got[0][key] != want[0][key]
        same_preview(got[0][key], want[0][key])
    assert trace_previews(reader, [path], **kw) == want
