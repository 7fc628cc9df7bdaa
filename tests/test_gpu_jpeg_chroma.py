"""-m gpu: 4:4:4, 4:2:2 and 4:4:0 JPEG files decoded on the device (csrc/jpegdec.hip) against the installed Pillow and the restatement of
tests/jpeg_chroma_ref.py, stage by stage; through ``bbocr_jpeg_imread`` with an EXIF orientation against the host's ``imread``; and through
``Reader(device_decode="chroma").readtext(path)`` against the host decode.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_chroma_ref as K
import jpeg_entropy_ref as J
import orient_ref as R
from test_gpu_jpeg_decode import stage, status_word
from test_gpu_orient import host_imread
from test_jpeg_chroma_cpu import matrix, stage_input
from test_jpeg_decode_cpu import picture, pillow_pixels, save

pytestmark = pytest.mark.gpu

LANES = 64                                                       # kernels.h JD_LANES: subsequences per workgroup
YCBCR4, YCBCR3 = 3, 4                                             # bbocr.h BBOCR_PAGE_*


def pages_of(datas):
    from bb_ocr_amd.reader import jpeg_page

    pages = [jpeg_page(d, chroma=True) for d in datas]
    assert all(p is not None for p in pages) and all(jpeg_page(d) is None for d in datas[:3])
    return pages


def test_matrix_in_one_call_per_shape_and_in_one_call_equals_pillow(reader):
    files = matrix()
    assert len(files) == 198
    want = [pillow_pixels(d) for _, _, d in files]
    pages = pages_of([d for _, _, d in files])
    groups = {}
    for i, p in enumerate(pages):
        groups.setdefault(p.shape, []).append(i)
    assert len(groups) == 11
    for padded in (False, True):                                 # ONE bbocr_jpeg_decode call per shape, 3 and 4 bytes per pixel
        for idxs in groups.values():
            t, status = reader.decode_jpeg_batch([pages[i] for i in idxs], padded=padded)
            assert status == [0] * len(idxs)
            t = t.cpu().numpy()
            for k, i in enumerate(idxs):
                assert np.array_equal(t[k][..., :3], want[i]), (files[i][0], padded)
                assert not padded or (t[k][..., 3] == 255).all(), files[i][0]
    n = len(pages)                                               # every size and class in ONE call, each file into its own buffer
    files_c, sizes_c = reader._jpeg_files(pages)
    for layout, px in ((YCBCR3, 3), (YCBCR4, 4)):
        outs = [torch.full(p.shape[:2] + (px,), 9, dtype=torch.uint8, device=reader.device) for p in pages]
        op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        pt = (C.c_longlong * n)(*[p.shape[1] * px for p in pages])
        status = (C.c_int * n)(*([1] * n))
        torch.cuda.synchronize()
        reader._check(reader._lib.bbocr_jpeg_decode(reader._h, files_c, sizes_c, n, layout, op, pt, status))
        assert list(status) == [0] * n
        for (name, _, _), o, w in zip(files, outs, want):
            assert np.array_equal(o.cpu().numpy()[..., :3], w), (name, px)


@pytest.mark.parametrize("name", ["noise444", "noise422", "noise440", "flat422"])
def test_stage_outputs_equal_the_restatement(reader, name):
    data, S = stage_input(name)
    plan = K.parse(data)
    assert plan["chroma"] == {"noise444": K.C444, "noise422": K.C422, "noise440": K.C440, "flat422": K.C422}[name]
    coef, states = K.decode_coefficients(data, plan, S or 1024)
    assert len(states) > 2 * LANES                               # several workgroups of subsequences
    planes = K.component_planes(coef, plan)
    want_padded = K.padded_planes(coef, plan)
    H, W, my, mx = plan["height"], plan["width"], plan["mcu_rows"], plan["mcu_cols"]
    assert (H, W) == (384, 256)
    h, v = K.luma(plan)
    want_px = pillow_pixels(data)
    assert np.array_equal(K.planes_to_pixels(planes, plan), want_px)
    ysz, csz = my * 8 * v * mx * 8 * h, my * 8 * mx * 8
    for rep in range(2):                                         # the outputs repeat bit for bit
        got = stage(reader, 0, data, S, (len(states), 4), torch.int32)
        assert np.array_equal(got, states), rep
        got = stage(reader, 1, data, S, (coef.shape[0], 64), torch.int16)
        assert np.array_equal(got, coef), rep
        got = stage(reader, 2, data, S, (ysz + 2 * csz,), torch.uint8)
        assert np.array_equal(got[:ysz].reshape(my * 8 * v, mx * 8 * h), want_padded[0]), rep
        assert np.array_equal(got[ysz:ysz + csz].reshape(my * 8, mx * 8), want_padded[1]), rep
        assert np.array_equal(got[ysz + csz:].reshape(my * 8, mx * 8), want_padded[2]), rep
        got = stage(reader, 3, data, S, (H, W, 3), torch.uint8)
        assert np.array_equal(got, want_px), rep


def test_imread_with_an_orientation_equals_the_host(reader):
    from bb_ocr_amd.preprocess import IMREAD_JPEG, IMREAD_YCC, imread_bgr_device
    from bb_ocr_amd.reader import JpegPage, jpeg_plan

    f422 = save(picture("noise", 131, 67, "RGB"), quality=90, subsampling=1, restart_marker_rows=1)
    f440 = K.make_440(save(picture("gradient", 67, 131, "RGB"), quality=90, subsampling=1))
    cases = [R.with_orientation(f422, 6), R.with_orientation(f422, 5, "MM"), R.with_orientation(f440, 6, "MM"), R.with_orientation(f440, 5)]
    plans = [jpeg_plan(d) for d in cases]
    assert [(p.chroma, p.orientation, p.supported) for p in plans] == [(K.C422, 6, 0), (K.C422, 5, 0), (K.C440, 6, 0), (K.C440, 5, 0)]
    want = [host_imread(reader, d) for d in cases]
    outs, status = reader.imread_jpeg_batch([JpegPage(d, p) for d, p in zip(cases, plans)])      # ONE bbocr_jpeg_imread call
    assert status == [0, 0, 0, 0]
    for o, w in zip(outs, want):
        assert tuple(o.shape) == (131, 67, 3) and torch.equal(o, w)
    for d, w in zip(cases, want):
        got = imread_bgr_device(reader, d, device_decode="chroma")
        assert got.imread_path == IMREAD_JPEG and got.is_contiguous() and torch.equal(got, w)
        for option in (True, None):                              # the host's decode, oriented on the card: as before
            got = imread_bgr_device(reader, d, option)
            assert got.imread_path == IMREAD_YCC and torch.equal(got, w)


@pytest.fixture(scope="module")
def chroma_reader(states_trained):
    import bb_ocr_amd

    r = bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, precision="fp16", device_decode="chroma")
    yield r
    r.close()


def test_readtext_of_a_path_equals_the_host_decode(chroma_reader, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth

    r = chroma_reader
    assert r.device_decode is True and r.jpeg_chroma is True and r.decode_option == "chroma"
    img = Image.fromarray(synth.page(3, width=640, height=480, lines=12, margin=24)[0])
    for sub in (0, 1):
        path = str(tmp_path / ("page%d.jpg" % sub))
        img.save(path, "JPEG", quality=90, subsampling=sub)
        assert r.decode_jpeg_device([path])[0] is not None and r.decode_jpeg_device([path], chroma=False) == [None]
        got = r.readtext(path)
        got_files = r.readtext_files([path])
        r.device_decode = False
        try:
            want = r.readtext(path)
            want_files = r.readtext_files([path], device_decode=False)
        finally:
            r.device_decode = True
        assert len(want) > 0 and got == want and got_files == want_files and len(want_files[0]) > 0       # boxes, texts, confidences


def test_damaged_entropy_data_is_a_status_code(reader):
    """a 4:2:2 file with 64 bytes of its entropy-coded data overwritten (test_gpu_jpeg_decode.py's recipe), between two good files"""
    from bb_ocr_amd.reader import JpegPage, jpeg_plan

    files = [d for n, c, d in matrix((200, 120)) if "noise" in n and c == K.C422][:3]
    plan = jpeg_plan(files[1])
    assert plan.chroma == K.C422 and plan.scan_bytes > 400
    bad = bytearray(files[1])
    a = int(plan.scan_offset) + int(plan.scan_bytes) // 2
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))     # no FF: the markers and the plan stay as they were
    bad = bytes(bad)
    assert jpeg_plan(bad).chroma == K.C422 and jpeg_plan(bad).scan_bytes == plan.scan_bytes
    t, status = reader.decode_jpeg_batch([JpegPage(d, jpeg_plan(d)) for d in (files[0], bad, files[2])])
    assert status[0] == 0 and status[2] == 0 and status[1] < 0
    word = J.device_model(bad, K.parse(bad), status=True, stream=K.Stream(bad, K.parse(bad)))[3]      # exactly the model's bits
    assert word != 0 and status_word(reader, bad) == word
    t = t.cpu().numpy()
    assert np.array_equal(t[0], pillow_pixels(files[0])) and np.array_equal(t[2], pillow_pixels(files[2]))
    assert reader.decode_jpeg_device([bad], chroma=True) == [None]
    t, status = reader.decode_jpeg_batch([JpegPage(files[1], plan)])  # and the context stays usable
    assert status == [0] and np.array_equal(t.cpu().numpy()[0], pillow_pixels(files[1]))
