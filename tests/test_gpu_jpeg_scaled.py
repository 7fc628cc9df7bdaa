"""-m gpu: baseline JPEG files decoded at scale 1/2, 1/4 and 1/8 on the device (csrc/jpegdec.hip: bbocr_jpeg_decode_scaled /
bbocr_op_jpeg_scaled_stage) against the installed Pillow's draft decode and the restatement of tests/jpeg_scaled_ref.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_entropy_ref as J
import jpeg_scaled_ref as S
from test_gpu_jpeg_decode import status_word
from test_jpeg_decode_cpu import PHOTOS, matrix, picture, pillow_pixels, save
from test_jpeg_scaled_cpu import SCALES, pillow_draft, small_matrix

pytestmark = pytest.mark.gpu

ERR_ARG = -1                                                      # bbocr.h BBOCR_ERR_ARG
from bb_ocr_amd._lib import PAGE_YCBCR3 as YCBCR3, PAGE_YCBCR4 as YCBCR4  # noqa: E402


def decode_scaled(reader, datas, scale, layout=YCBCR3, pad=0, fill=9):
    """ONE bbocr_jpeg_decode_scaled call over all files, each into its own buffer whose rows are `pad` bytes longer than the pixels ->
    ([array or None per file], [status]); the padding must come back untouched"""
    from bb_ocr_amd.reader import jpeg_plan

    n = len(datas)
    plans = [jpeg_plan(d) for d in datas]
    px = [1 if p.components == 1 else (4 if layout == YCBCR4 else 3) for p in plans]
    dims = [S.scaled_dims(max(p.height, 1), max(p.width, 1), scale) for p in plans]
    outs = [torch.full((oh, ow * k + pad), fill, dtype=torch.uint8, device=reader.device) for (oh, ow), k in zip(dims, px)]
    bufs = [(C.c_ubyte * len(d)).from_buffer_copy(d) for d in datas]
    fl = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sz = (C.c_size_t * n)(*[len(d) for d in datas])
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    pt = (C.c_longlong * n)(*[o.shape[1] for o in outs])
    status = (C.c_int * n)(*([77] * n))
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_jpeg_decode_scaled(reader._h, fl, sz, n, layout, scale, op, pt, status))
    res = []
    for o, (oh, ow), k, st in zip(outs, dims, px, status):
        a = o.cpu().numpy()
        assert np.all(a[:, ow * k:] == fill)
        a = a[:, :ow * k]
        res.append(None if st != 0 else (a if k == 1 else a.reshape(oh, ow, k)))
    return res, list(status)


@pytest.mark.parametrize("s", SCALES)
def test_small_matrix_in_one_call_equals_pillows_draft(reader, s):
    files = small_matrix()
    assert len(files) > 50 and {J.parse(d)["components"] for _, d in files} == {1, 3}
    want = [pillow_draft(d, s) for _, d in files]
    got, status = decode_scaled(reader, [d for _, d in files], s, YCBCR3, pad=0)
    assert status == [0] * len(files)
    for (name, _), g, w in zip(files, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, s)
    for pad in (5, 8):                                            # padded pixels; rows at odd pitches and at whole words
        got4, status = decode_scaled(reader, [d for _, d in files], s, YCBCR4, pad=pad)
        assert status == [0] * len(files)
        for (name, _), g, w in zip(files, got4, want):
            if w.ndim == 3:
                assert np.array_equal(g[..., :3], w) and np.all(g[..., 3] == 255), (name, s, pad)
            else:
                assert np.array_equal(g, w), (name, s, pad)


def scaled_stage(reader, stg, data, s, shape):
    dst = torch.full(shape, 77, dtype=torch.uint8, device=reader.device)
    st = C.c_int(1)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    reader._check(reader._lib.bbocr_op_jpeg_scaled_stage(reader._h, stg, buf, len(data), s, C.c_void_p(dst.data_ptr()), dst.numel(), C.byref(st)))
    assert st.value == 0
    return dst.cpu().numpy()


@pytest.mark.parametrize("s", SCALES)
def test_stage_planes_and_pixels_equal_the_restatement(reader, s):
    files = dict(small_matrix())
    for name in ("33x50-noise-RGB-q30", "33x50-noise-L-q30", "96x160-text-RGB-rst"):
        data = files[name]
        plan = J.parse(data)
        coef, _ = J.decode_coefficients(data, plan)
        planes = S.scaled_planes(coef, plan, s)
        ph, pw, _, _ = S.plane_geometry(plan, s)
        got = scaled_stage(reader, 2, data, s, (len(planes), ph, pw))
        assert np.array_equal(got, np.stack(planes).astype(np.uint8)), (name, s)
        want = S.planes_to_pixels(planes, plan, s)
        assert np.array_equal(scaled_stage(reader, 3, data, s, want.shape), want), (name, s)


def test_scale_one_is_the_existing_decode(reader):
    files = [d for _, d in matrix((47, 33))][:12] + [d for _, d in small_matrix()[:6]]
    got, status = decode_scaled(reader, files, 1)
    assert status == [0] * len(files)
    for d, g in zip(files, got):
        assert np.array_equal(g, pillow_pixels(d))
    # a chroma class goes through at scale 1 as it does through bbocr_jpeg_decode
    d444 = save(picture("noise", 40, 24, "RGB"), quality=90, subsampling=0)
    got, status = decode_scaled(reader, [d444], 1)
    assert status == [0] and np.array_equal(got[0], pillow_pixels(d444))


def test_photograph_equals_pillows_draft(reader):
    data = open(PHOTOS[0], "rb").read()
    for s in SCALES:
        got, status = decode_scaled(reader, [data], s)
        assert status == [0] and np.array_equal(got[0], pillow_draft(data, s)), s


def test_files_outside_the_scope_are_refused_per_file(reader):
    img = picture("gradient", 64, 48, "RGB")
    good = [save(img, quality=90), save(picture("noise", 33, 17, "L"), quality=80)]
    files = [good[0], save(img, quality=90, subsampling=0), save(img, quality=90, subsampling=1), save(img, quality=90, progressive=True), good[1]]
    for s in SCALES:
        got, status = decode_scaled(reader, files, s)
        assert status == [0, ERR_ARG, ERR_ARG, ERR_ARG, 0], s
        assert np.array_equal(got[0], pillow_draft(good[0], s)) and np.array_equal(got[4], pillow_draft(good[1], s))
    assert reader.decode_jpeg_device(files[:2], chroma=True, scale=2)[1] is None
    rgb, gray = reader.decode_jpeg_device(files[:2], scale=2)[0]
    ycc = pillow_draft(good[0], 2)
    assert np.array_equal(gray.cpu().numpy(), ycc[..., 0]) and rgb.shape == (24, 32, 3)
    rc = reader._lib.bbocr_jpeg_decode_scaled(reader._h, None, None, 1, YCBCR3, 3, None, None, None)
    assert rc == ERR_ARG


def test_damaged_entropy_data_is_a_status_code(reader):
    """the existing decode test's corrupted-bytes case at scale 2: a supported file with 64 bytes of its entropy-coded data overwritten,
    between two good files"""
    from bb_ocr_amd.reader import jpeg_plan

    files = [d for n, d in matrix((200, 120)) if "noise-RGB" in n][:3]
    plan = jpeg_plan(files[1])
    bad = bytearray(files[1])
    a = int(plan.scan_offset) + int(plan.scan_bytes) // 2
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))     # no FF: the markers and the plan stay as they were
    got, status = decode_scaled(reader, [files[0], bytes(bad), files[2]], 2)
    assert status[0] == 0 and status[2] == 0 and status[1] < 0 and status[1] != ERR_ARG
    word = J.device_model(bytes(bad), J.parse(bytes(bad)), status=True)[3]      # the entropy stages are the full-scale decode's: the model's bits
    assert word != 0 and status_word(reader, bytes(bad)) == word
    assert np.array_equal(got[0], pillow_draft(files[0], 2)) and np.array_equal(got[2], pillow_draft(files[2], 2))
    again, status = decode_scaled(reader, [files[1]], 2)
    assert status == [0] and np.array_equal(again[0], pillow_draft(files[1], 2))
