"""-m gpu: baseline JPEG files decoded on the device (csrc/jpegdec.hip: bbocr_jpeg_decode / bbocr_op_jpeg_stage) against the installed
Pillow and the restatement of tests/jpeg_entropy_ref.py, stage by stage, and through ``Reader(device_decode=True)``, ``read_files`` and
``extract_texts(device_decode=True)``."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

import jpeg_entropy_ref as J
from test_jpeg_decode_cpu import PHOTOS, matrix, pillow_pixels, save, sync_inputs

pytestmark = pytest.mark.gpu

LANES = 64                                                       # kernels.h JD_LANES: subsequences per workgroup


def decode(reader, datas, padded=False):
    """files -> [pixels or None], grouped by decoded shape as Reader.decode_jpeg_device groups them: ONE call per shape"""
    from bb_ocr_amd.reader import jpeg_page

    pages = [jpeg_page(d) for d in datas]
    out = [None] * len(pages)
    groups = {}
    for i, p in enumerate(pages):
        assert p is not None
        groups.setdefault(p.shape, []).append(i)
    for idxs in groups.values():
        t, status = reader.decode_jpeg_batch([pages[i] for i in idxs], padded=padded)
        t = t.cpu().numpy()
        for k, i in enumerate(idxs):
            out[i] = t[k] if status[k] == 0 else None
    return out


def stage(reader, stg, data, S, shape, dtype):
    dst = torch.full(shape, 77, dtype=dtype, device=reader.device)
    st = C.c_int(1)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    reader._check(reader._lib.bbocr_op_jpeg_stage(reader._h, stg, buf, len(data), S, C.c_void_p(dst.data_ptr()), dst.numel() * dst.element_size(),
                                                  C.byref(st)))
    assert st.value == 0
    return dst.cpu().numpy()


def status_word(reader, data, S=0):
    """stage 4 of bbocr_op_jpeg_stage: the JD_ERR_* bits the write pass raised for the file (jpeg_entropy_ref.ERR_*)"""
    dst = torch.full((1,), -1, dtype=torch.int32, device=reader.device)
    st = C.c_int(1)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    reader._check(reader._lib.bbocr_op_jpeg_stage(reader._h, 4, buf, len(data), S, C.c_void_p(dst.data_ptr()), 4, C.byref(st)))
    word = int(dst.cpu()[0])
    assert (st.value == 0) == (word == 0) and 0 <= word < 8
    return word


def test_matrix_in_one_call_per_shape_equals_pillow(reader):
    files = matrix()
    assert len(files) == 120
    got = decode(reader, [d for _, d in files])
    for (name, data), g in zip(files, got):
        assert g is not None, name
        assert np.array_equal(g, pillow_pixels(data)), name
    # mixed sizes and both component counts in ONE bbocr_jpeg_decode call, each file into its own buffer
    from bb_ocr_amd.reader import jpeg_page

    pages = [jpeg_page(d) for _, d in files]
    outs = [torch.full(p.shape if p.shape[2] == 3 else p.shape[:2], 9, dtype=torch.uint8, device=reader.device) for p in pages]
    n = len(pages)
    bufs = [(C.c_ubyte * len(p.data)).from_buffer_copy(p.data) for p in pages]
    fl = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sz = (C.c_size_t * n)(*[len(p.data) for p in pages])
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    pt = (C.c_longlong * n)(*[p.shape[1] * (3 if p.shape[2] == 3 else 1) for p in pages])
    status = (C.c_int * n)()
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_jpeg_decode(reader._h, fl, sz, n, 4, op, pt, status))
    assert list(status) == [0] * n
    for (name, data), o in zip(files, outs):
        assert np.array_equal(o.cpu().numpy(), pillow_pixels(data)), name


@pytest.mark.parametrize("name,S", [("photo", 0), ("text", 0), ("noise", 0), ("flat", 32), ("flat", 0)])
def test_stage_outputs_equal_the_restatement(reader, name, S):
    data = sync_inputs()[name]
    plan = J.parse(data)
    coef, states = J.decode_coefficients(data, plan, S or 1024)
    if not (name == "flat" and S == 0):
        assert len(states) > 2 * LANES                           # several workgroups of subsequences
    planes = J.component_planes(coef, plan)
    H, W, my, mx = plan["height"], plan["width"], plan["mcu_rows"], plan["mcu_cols"]
    want_px = pillow_pixels(data)
    assert np.array_equal(J.planes_to_pixels(planes, plan), want_px)
    for rep in range(2):                                         # the outputs repeat bit for bit
        got = stage(reader, 0, data, S, (len(states), 4), torch.int32)
        assert np.array_equal(got, states), rep
        got = stage(reader, 1, data, S, (coef.shape[0], 64), torch.int16)
        assert np.array_equal(got, coef), rep
        got = stage(reader, 2, data, S, (my * 16 * mx * 16 * 3 // 2,), torch.uint8)
        y = got[:my * 16 * mx * 16].reshape(my * 16, mx * 16)
        c = got[my * 16 * mx * 16:].reshape(2, my * 8, mx * 8)
        ch, cw = -(-H // 2), -(-W // 2)
        assert np.array_equal(y[:H, :W], planes[0]) and np.array_equal(c[0, :ch, :cw], planes[1]) and np.array_equal(c[1, :ch, :cw], planes[2]), rep
        got = stage(reader, 3, data, S, (H, W, 3), torch.uint8)
        assert np.array_equal(got, want_px), rep


def test_photographs_without_restart_markers_equal_decode_file_ycc(reader):
    from bb_ocr_amd.reader import decode_file_ycc, jpeg_plan

    for path in PHOTOS:
        data = open(path, "rb").read()
        assert jpeg_plan(data).restart_interval == 0
        got = decode(reader, [data])[0]
        assert got is not None and np.array_equal(got, decode_file_ycc(path))
        got4 = decode(reader, [data], padded=True)[0]
        assert np.array_equal(got4[..., :3], got)


def test_page_with_a_restart_interval_per_mcu_row_and_plain(reader):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.reader import jpeg_plan

    img = Image.fromarray(synth.page(5, width=1280, height=960)[0])
    rst, plain = save(img, quality=90, restart_marker_rows=1), save(img, quality=90)
    assert jpeg_plan(rst).segments == 60 and jpeg_plan(plain).segments == 1
    got = decode(reader, [rst, plain])
    assert np.array_equal(got[0], pillow_pixels(rst))
    assert np.array_equal(got[1], pillow_pixels(plain))


@pytest.fixture(scope="module")
def pages_dir(tmp_path_factory):
    """12 files: synthetic pages as JPEG (two sizes, one grey, one with restart markers), a photograph, one PNG, one progressive JPEG"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("jpeg_pages")
    paths = []
    for k in range(9):
        w, h = (640, 480) if k % 2 == 0 else (512, 384)
        img = Image.fromarray(synth.page(20 + k, width=w, height=h, lines=8, margin=24)[0])
        kw = dict(quality=90)
        if k == 3:
            img = img.convert("L")
        if k == 4:
            kw["restart_marker_rows"] = 1
        paths.append(str(d / ("p%02d.jpg" % k)))
        img.save(paths[-1], "JPEG", **kw)
    paths.append(str(d / "p09.png"))
    Image.fromarray(synth.page(40, width=640, height=480, lines=8, margin=24)[0]).save(paths[-1], "PNG")
    paths.append(str(d / "p10.jpg"))
    Image.fromarray(synth.page(41, width=640, height=480, lines=8, margin=24)[0]).save(paths[-1], "JPEG", quality=90, progressive=True)
    paths.append(PHOTOS[1])
    return paths


@pytest.fixture(scope="module")
def trained(readers_trained):
    return readers_trained["fp16"]


def test_readtext_of_a_path_equals_the_host_decode(trained, pages_dir):
    from bb_ocr_amd.reader import jpeg_page

    assert trained.device_decode is False
    for path in (pages_dir[0], pages_dir[1], PHOTOS[1]):
        want = trained.readtext(path)
        trained.device_decode = True
        try:
            assert jpeg_page(path) is not None
            got = trained.readtext(path)
            data = open(path, "rb").read()
            got_bytes, want_bytes = trained.readtext(data), None
        finally:
            trained.device_decode = False
        want_bytes = trained.readtext(data)
        assert len(want) > 0 and got == want
        assert got_bytes == want_bytes
    pairs = trained.decode_jpeg_device([pages_dir[3], pages_dir[9], pages_dir[10]])
    from bb_ocr_amd.reader import decode_file

    rgb, gray = decode_file(pages_dir[3])                       # the grey file
    assert pairs[1] is None and pairs[2] is None
    assert np.array_equal(pairs[0][0].cpu().numpy(), rgb) and np.array_equal(pairs[0][1].cpu().numpy(), gray)


def test_read_files_and_extract_texts_equal_the_option_off(trained, pages_dir):
    from bb_ocr_amd.extractor_batch import extract_texts, read_files

    want = read_files(trained, pages_dir)
    got = read_files(trained, pages_dir, device_decode=True)
    assert got == want and sum(len(v) > 0 for v in want.values()) >= 11
    want_t = extract_texts(trained, pages_dir)
    got_t = extract_texts(trained, pages_dir, device_decode=True)
    assert got_t == want_t and sum(len(v) > 0 for v in want_t.values()) >= 11


def test_extract_texts_with_the_device_thumbnail_on_a_page_above_the_limit(trained, pages_dir, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.extractor_batch import extract_texts

    big = str(tmp_path / "big.jpg")
    Image.fromarray(synth.page(50, width=2000, height=1500, lines=14, margin=40)[0]).save(big, "JPEG", quality=92)
    paths = [big, pages_dir[0], pages_dir[9]]
    want = extract_texts(trained, paths, device_thumbnail=True)
    got = extract_texts(trained, paths, device_thumbnail=True, device_decode=True)
    assert got == want and len(want[0]) > 0
    assert extract_texts(trained, paths, device_decode=True) == extract_texts(trained, paths)


def test_damaged_entropy_data_is_a_status_code(reader):
    """last in the file: a supported file with 64 bytes of its entropy-coded data overwritten, between two good files"""
    from bb_ocr_amd.reader import JpegPage, jpeg_plan

    files = [d for n, d in matrix((200, 120)) if "noise-RGB" in n][:3]
    plan = jpeg_plan(files[1])
    assert plan.supported and plan.scan_bytes > 400
    bad = bytearray(files[1])
    a = int(plan.scan_offset) + int(plan.scan_bytes) // 2
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))     # no FF: the markers and the plan stay as they were
    bad = bytes(bad)
    assert jpeg_plan(bad).supported and jpeg_plan(bad).scan_bytes == plan.scan_bytes
    pages = [JpegPage(d, jpeg_plan(d)) for d in (files[0], bad, files[2])]
    t, status = reader.decode_jpeg_batch(pages)
    assert status[0] == 0 and status[2] == 0 and status[1] < 0
    word = J.device_model(bad, J.parse(bad), status=True)[3]       # exactly the bits the model of the passes names
    assert word != 0 and status_word(reader, bad) == word
    t = t.cpu().numpy()
    assert np.array_equal(t[0], pillow_pixels(files[0])) and np.array_equal(t[2], pillow_pixels(files[2]))
    assert reader.decode_jpeg_device([bad]) == [None]
    again = decode(reader, [files[1]])[0]
    assert np.array_equal(again, pillow_pixels(files[1]))
