"""-m gpu: the device side of ``cv2.imread`` -- ``page_orient`` (csrc/orient.hip: bbocr_page_orient) against the numpy restatement of
tests/orient_ref.py bit for bit, ``bbocr_jpeg_imread`` / ``preprocess.imread_bgr_device`` against ``preprocess._imread_bgr`` (Pillow) with
the path taken asserted, and the extractor's crop settings with ``device_decode=True`` against the option off.

Shapes of the kernel test: the kernel's tile edge is ``bb_ocr_amd.preprocess.ORIENT_TILE`` (= csrc/kernels.h ORIENT_TILE) pixels."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import jpeg_ref
import orient_ref as R
from test_jpeg_decode_cpu import PHOTOS, matrix, picture, save

pytestmark = pytest.mark.gpu

GRAY, BGR, RGB, YCC4, YCC3 = 0, 1, 2, 3, 4                        # bbocr.h BBOCR_PAGE_*
BYTES = {GRAY: 1, BGR: 3, RGB: 3, YCC4: 4, YCC3: 3}
ERR_ARG = -1


def tile():
    from bb_ocr_amd.preprocess import ORIENT_TILE

    return ORIENT_TILE


def shapes():
    T = tile()
    return [(1, 1), (1, 67), (67, 1), (2, 3), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (2 * T + 2, 4 * T + 1)]


def odd_pitch(row_bytes, pad):
    """a pitch larger than the row that is no multiple of 4"""
    p = row_bytes + pad
    return p if p % 4 else p + 1


def strided_page(reader, a, offset):
    """host page [H,W,c] -> a device view of the same shape whose rows are an odd pitch apart and start `offset` bytes into a buffer"""
    H, W, c = a.shape
    pitch = odd_pitch(W * c, 5)
    buf = torch.full((offset + H * pitch + 8,), 0x3C, dtype=torch.uint8, device=reader.device)
    view = buf.as_strided((H, W, c), (pitch, c, 1), offset)
    view.copy_(torch.from_numpy(a).to(reader.device))
    return view[:, :, 0] if c == 1 else view


def expected_rgb(a, layout):
    if layout == GRAY:
        return np.repeat(a, 3, axis=2)
    if layout == RGB:
        return a
    if layout == BGR:
        return a[..., ::-1]
    return jpeg_ref.ycc_to_rgb(a[..., 0], a[..., 1], a[..., 2])


def raw_orient(reader, page, layout, o, dst_layout, dst_offset=0, src_pitch=None, dst_pitch=None):
    """bbocr_page_orient into a 0xA5-filled buffer with an odd destination pitch -> (status, buffer on the host, H', W', pitch, offset)"""
    H, W = page.shape[:2]
    dc = 1 if dst_layout == GRAY else 3
    oh, ow = (W, H) if o >= 5 else (H, W)
    if dst_pitch is None:
        dst_pitch = odd_pitch(ow * dc, 7)
    dst = torch.full((dst_offset + oh * max(dst_pitch, ow * dc) + 16,), 0xA5, dtype=torch.uint8, device=reader.device)
    rh, rw = C.c_int(), C.c_int()
    torch.cuda.synchronize()
    rc = reader._lib.bbocr_page_orient(reader._h, C.c_void_p(page.data_ptr()), H, W, page.stride(0) if src_pitch is None else src_pitch, layout, o,
                                       dst_layout, C.c_void_p(dst.data_ptr() + dst_offset), dst_pitch, C.byref(rh), C.byref(rw))
    return rc, dst.cpu().numpy(), rh.value, rw.value, dst_pitch, dst_offset


def check_buffer(buf, want, pitch, offset, what):
    """`want` [H',W',c] sits in the buffer; every other byte of it is still 0xA5"""
    oh, ow, c = want.shape
    body = buf[offset:offset + oh * pitch].reshape(oh, pitch)
    assert np.array_equal(body[:, :ow * c].reshape(oh, ow, c), want), what
    assert (body[:, ow * c:] == 0xA5).all(), ("bytes behind a row", what)
    assert (buf[:offset] == 0xA5).all() and (buf[offset + oh * pitch:] == 0xA5).all(), ("bytes outside the page", what)


@pytest.mark.parametrize("shape", shapes(), ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement(reader, shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    for layout in (GRAY, BGR, RGB, YCC4, YCC3):
        a = rng.integers(0, 256, (H, W, BYTES[layout]), dtype=np.uint8)
        page = strided_page(reader, a, offset=1 + layout % 3)
        assert page.stride(0) % 4 != 0
        rgb = expected_rgb(a, layout)
        for dst_layout in (BGR, RGB) + ((GRAY,) if layout == GRAY else ()):
            px = a if dst_layout == GRAY else (rgb if dst_layout == RGB else rgb[..., ::-1])
            for o in range(1, 9):
                rc, buf, rh, rw, pitch, off = raw_orient(reader, page, layout, o, dst_layout, dst_offset=(o + layout) % 4)
                want = R.orient(px, o)
                assert rc == 0 and (rh, rw) == want.shape[:2]
                check_buffer(buf, want, pitch, off, (shape, layout, dst_layout, o))


def test_size_query_and_the_checked_wrapper(reader):
    from bb_ocr_amd.preprocess import orient_page_device

    a = np.random.default_rng(3).integers(0, 256, (5, 9, 3), dtype=np.uint8)
    page = reader._to_dev(a)
    rh, rw = C.c_int(), C.c_int()
    assert reader._lib.bbocr_page_orient(reader._h, C.c_void_p(page.data_ptr()), 5, 9, 27, BGR, 6, RGB, C.c_void_p(None), 0, C.byref(rh),
                                         C.byref(rw)) == 0
    assert (rh.value, rw.value) == (9, 5)
    got = orient_page_device(reader, page, BGR, 6, RGB)
    assert np.array_equal(got.cpu().numpy(), R.orient(a[..., ::-1], 6))
    assert np.array_equal(orient_page_device(reader, page, RGB, 8).cpu().numpy(), R.orient(a[..., ::-1], 8))      # BGR is the default
    view = reader._to_dev(np.random.default_rng(4).integers(0, 256, (12, 20, 3), dtype=np.uint8))[2:9, 3:17]       # a crop, read in place
    assert np.array_equal(orient_page_device(reader, view, BGR, 7, BGR).cpu().numpy(), R.orient(view.cpu().numpy(), 7))
    g = reader._to_dev(a[..., 0].copy())
    assert np.array_equal(orient_page_device(reader, g, GRAY, 5, GRAY).cpu().numpy(), R.orient(a[..., 0], 5))
    for bad in (torch.from_numpy(a), page.to(torch.int32), page[:, :, :2], page[:, ::2], page.permute(1, 0, 2), page[:0]):
        with pytest.raises(ValueError):
            orient_page_device(reader, bad, BGR, 6, RGB)
    for args in ((page, BGR, 0, RGB), (page, BGR, 9, RGB), (page, BGR, 6, GRAY), (page, 7, 6, RGB), (page, GRAY, 6, RGB), (g, BGR, 6, RGB),
                 (page, YCC4, 6, RGB), (page, BGR, 6, 5)):
        with pytest.raises(ValueError):
            orient_page_device(reader, *args)


def test_argument_errors_leave_the_context_usable(reader):
    a = np.random.default_rng(5).integers(0, 256, (70, 33, 3), dtype=np.uint8)
    page = reader._to_dev(a)
    bad = [dict(o=0), dict(o=9), dict(dst_layout=GRAY), dict(layout=5), dict(layout=-1), dict(dst_layout=YCC3), dict(src_pitch=33 * 3 - 1),
           dict(dst_pitch=70 * 3 - 1)]
    for kw in bad:
        args = dict(layout=BGR, o=6, dst_layout=RGB)
        args.update(kw)
        rc, buf, *_ = raw_orient(reader, page, **args)
        assert rc == ERR_ARG, kw
        assert (buf == 0xA5).all(), kw                            # nothing was queued
        rc, buf, rh, rw, pitch, off = raw_orient(reader, page, BGR, 6, RGB)       # the next valid call
        assert rc == 0
        check_buffer(buf, R.orient(a[..., ::-1], 6), pitch, off, kw)
    rh, rw = C.c_int(), C.c_int()
    dst = torch.empty((33, 70, 3), dtype=torch.uint8, device=reader.device)
    L = reader._lib
    assert L.bbocr_page_orient(reader._h, C.c_void_p(None), 70, 33, 99, BGR, 6, RGB, C.c_void_p(dst.data_ptr()), 210, C.byref(rh), C.byref(rw)) == ERR_ARG
    assert L.bbocr_page_orient(reader._h, C.c_void_p(page.data_ptr()), 0, 33, 99, BGR, 6, RGB, C.c_void_p(dst.data_ptr()), 210, C.byref(rh),
                               C.byref(rw)) == ERR_ARG
    assert L.bbocr_page_orient(reader._h, C.c_void_p(page.data_ptr()), 70, 33, 99, BGR, 6, RGB, C.c_void_p(dst.data_ptr()), 210, None, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ imread
@pytest.fixture(scope="module")
def photo():
    return R.bare(open(PHOTOS[1], "rb").read())


def host_imread(reader, data):
    from bb_ocr_amd.preprocess import _imread_bgr

    return reader._to_dev(_imread_bgr(io.BytesIO(data)))


def check_imread(reader, data, path):
    from bb_ocr_amd.preprocess import imread_bgr_device

    got = imread_bgr_device(reader, data)
    want = host_imread(reader, data)
    assert got.imread_path == path
    assert got.dtype == torch.uint8 and got.device == want.device and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got, want)
    return got


def test_imread_of_a_photograph_in_every_orientation(reader, photo, tmp_path):
    from bb_ocr_amd.preprocess import IMREAD_JPEG, imread_bgr_device

    for o in range(1, 9):
        check_imread(reader, R.with_orientation(photo, o, "II" if o % 2 else "MM"), IMREAD_JPEG)
    check_imread(reader, photo, IMREAD_JPEG)                     # no EXIF at all
    p = tmp_path / "o6.jpg"
    p.write_bytes(R.with_orientation(photo, 6))
    assert torch.equal(imread_bgr_device(reader, str(p)), host_imread(reader, p.read_bytes()))       # a path


def test_imread_restart_intervals_and_a_grey_file(reader):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import IMREAD_JPEG
    from bb_ocr_amd.reader import jpeg_plan

    img = Image.fromarray(synth.page(5, width=330, height=210)[0])
    rst = R.with_orientation(save(img, quality=90, restart_marker_rows=1), 6)
    assert jpeg_plan(rst).segments == 14 and jpeg_plan(rst).orientation == 6
    assert tuple(check_imread(reader, rst, IMREAD_JPEG).shape) == (330, 210, 3)
    grey = R.with_orientation(save(img.convert("L"), quality=90), 6, "MM")
    assert jpeg_plan(grey).components == 1
    got = check_imread(reader, grey, IMREAD_JPEG)
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])


def test_imread_of_files_the_plan_refuses(reader):
    from bb_ocr_amd.preprocess import IMREAD_RGB, IMREAD_YCC
    from bb_ocr_amd.reader import jpeg_plan

    img = picture("gradient", 200, 120, "RGB")
    f444 = R.with_orientation(save(img, quality=90, subsampling=0), 5)
    assert not jpeg_plan(f444).supported
    assert tuple(check_imread(reader, f444, IMREAD_YCC).shape) == (200, 120, 3)
    prog = R.with_orientation(save(img, quality=90, progressive=True), 8, "MM")
    assert not jpeg_plan(prog).supported
    check_imread(reader, prog, IMREAD_YCC)
    png = io.BytesIO()
    picture("noise", 131, 67, "RGB").save(png, "PNG")
    assert tuple(check_imread(reader, png.getvalue(), IMREAD_RGB).shape) == (67, 131, 3)
    prog_grey = R.with_orientation(save(img.convert("L"), quality=90, progressive=True), 6)     # not YCbCr, not planned: Pillow's RGB
    check_imread(reader, prog_grey, IMREAD_RGB)


def damaged(data):
    """64 bytes of the entropy-coded data overwritten (test_gpu_jpeg_decode.py's damaged file): the plan stays as it was"""
    from bb_ocr_amd.reader import jpeg_plan

    plan = jpeg_plan(data)
    assert plan.supported and plan.scan_bytes > 400
    bad = bytearray(data)
    a = int(plan.scan_offset) + int(plan.scan_bytes) // 2
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))
    assert jpeg_plan(bytes(bad)).supported and jpeg_plan(bytes(bad)).scan_bytes == plan.scan_bytes
    return bytes(bad)


def test_imread_of_damaged_data_and_a_mixed_batch(reader):
    from bb_ocr_amd.preprocess import IMREAD_YCC
    from bb_ocr_amd.reader import JpegPage, jpeg_plan

    files = [d for n, d in matrix((200, 120)) if "noise-RGB" in n][:3]
    bad = damaged(R.with_orientation(files[1], 6))
    check_imread(reader, bad, IMREAD_YCC)                        # status != 0 on the card: the host's decode of the same bytes, oriented there
    # three files of different orientation (and size) in ONE bbocr_jpeg_imread call
    trio = [R.with_orientation(files[0], 8), R.with_orientation(files[1], 3, "MM"), R.with_orientation(matrix((47, 33))[0][1], 5)]
    pages = [JpegPage(d, jpeg_plan(d)) for d in trio]
    assert [p.orientation for p in pages] == [8, 3, 5]
    outs, status = reader.imread_jpeg_batch(pages)
    assert status == [0, 0, 0]
    for d, t in zip(trio, outs):
        assert torch.equal(t, host_imread(reader, d))
    # a damaged middle file leaves its neighbours correct
    pages[1] = JpegPage(bad, jpeg_plan(bad))
    outs, status = reader.imread_jpeg_batch(pages)
    assert status[0] == 0 and status[2] == 0 and status[1] < 0
    assert torch.equal(outs[0], host_imread(reader, trio[0])) and torch.equal(outs[2], host_imread(reader, trio[2]))
    outs, status = reader.imread_jpeg_batch([JpegPage(trio[1], jpeg_plan(trio[1]))])          # and the context stays usable
    assert status == [0] and torch.equal(outs[0], host_imread(reader, trio[1]))


# ------------------------------------------------------------------------------------------------ the extractor's crop settings
@pytest.fixture(scope="module")
def trained(readers_trained):
    return readers_trained["fp16"]


@pytest.fixture(scope="module")
def oriented_pages(tmp_path_factory):
    """three pages built from the fixtures: a rendered page stored rotated so that orientation 6 sets it upright, a photograph at
    orientation 3, a photograph at orientation 1"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("oriented")
    upright = Image.fromarray(synth.page(61, width=900, height=640, lines=10, margin=40)[0])
    files = [R.with_orientation(save(upright.transpose(Image.Transpose.ROTATE_90), quality=92), 6),
             R.with_orientation(R.bare(open(PHOTOS[0], "rb").read()), 3, "MM"),
             R.with_orientation(R.bare(open(PHOTOS[1], "rb").read()), 1)]
    paths = []
    for k, data in enumerate(files):
        paths.append(str(d / ("page%d.jpg" % k)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    return paths


def test_extract_texts_with_the_crop_settings_equals_the_option_off(trained, oriented_pages):
    from bb_ocr_amd.extractor_batch import extract_texts, ocr_page_crop
    from bb_ocr_amd.preprocess import IMREAD_JPEG, imread_bgr_device

    kw = dict(use_preprocessing=True, edge_crop_percent=10, crop_for_ocr=True)
    want = extract_texts(trained, oriented_pages, device_decode=False, **kw)
    got = extract_texts(trained, oriented_pages, device_decode=True, **kw)
    assert got == want
    want_t = extract_texts(trained, oriented_pages, device_thumbnail=True, device_decode=False, **kw)
    got_t = extract_texts(trained, oriented_pages, device_thumbnail=True, device_decode=True, **kw)
    assert got_t == want_t
    for path in oriented_pages:                                  # and the pages behind the texts: decoded on the card, the same crops
        assert imread_bgr_device(trained, path).imread_path == IMREAD_JPEG
        a = ocr_page_crop(trained, path, crop_for_ocr=True, edge_crop_percent=10)
        b = ocr_page_crop(trained, path, crop_for_ocr=True, edge_crop_percent=10, device_decode=True)
        assert np.array_equal(a, b)


def test_drop_ins_equal_the_option_off(trained, oriented_pages):
    from bb_ocr_amd.preprocess import auto_crop_text_region, preprocess_for_book_cover

    for path in oriented_pages[:2]:
        want, _, steps = preprocess_for_book_cover(path, reader=trained)
        got, _, steps2 = preprocess_for_book_cover(path, reader=trained, device_decode=True)
        assert np.array_equal(got, want) and steps == steps2
        a, b = auto_crop_text_region(path, reader=trained), auto_crop_text_region(path, reader=trained, device_decode=True)
        assert (a is None and b is None) or np.array_equal(a, b)
