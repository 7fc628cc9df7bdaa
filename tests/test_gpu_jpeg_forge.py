"""-m gpu: the files of test_jpeg_forge_cpu.py -- baseline JPEG files no libjpeg encoder writes -- on the device (csrc/jpegdec.hip through
bbocr_jpeg_decode, bbocr_op_jpeg_stage, bbocr_jpeg_decode_scales and the Reader).  List A decodes to the source's pixels with status 0,
list B never reaches the device, list C ends in exactly the status word the model of tests/jpeg_entropy_ref.py names.  Every comparison
is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_chroma_ref as K
import jpeg_entropy_ref as J
from test_gpu_jpeg_decode import stage, status_word
from test_jpeg_decode_cpu import pillow_pixels
from test_jpeg_forge_cpu import BIG, KINDS, big, list_a, list_b, list_c, model, pixels_of, source, sources_a
from test_jpeg_scaled_cpu import pillow_draft

pytestmark = pytest.mark.gpu

YCBCR3 = 4                                                        # bbocr.h BBOCR_PAGE_YCBCR3
GUARD = 64                                                        # bytes behind every output of the mixed call
ERR_DATA = -7                                                     # bbocr.h BBOCR_ERR_DATA


def all_of_list_a():
    """[(name, file, Pillow's pixels of its source)]: every source's variants, then the long scans"""
    out = [(n, d, pixels_of(n, k, s)) for k, s in sources_a() for n, d in list_a(k, s)]
    return out + [(n, d, pillow_pixels(source(k, BIG, 95))) for n, k, d in big()]


def pages_of(datas):
    from bb_ocr_amd.reader import jpeg_page

    pages = [jpeg_page(d, chroma=True) for d in datas]                # the opt-in path: chroma classes are taken
    assert all(p is not None for p in pages)
    return pages


def test_list_a_in_one_call_per_shape_and_in_one_call_equals_pillow(reader):
    from bb_ocr_amd.reader import jpeg_page

    files = all_of_list_a()
    assert len(files) == 3 * (33 + 36) + 3 * 24 + 4
    pages = pages_of([d for _, d, _ in files])
    for (name, d, _), p in zip(files, pages):
        assert (jpeg_page(d) is None) == (name.split("-")[0] not in KINDS), name      # a chroma class only when asked
    groups = {}
    for i, p in enumerate(pages):
        groups.setdefault(p.shape, []).append(i)
    assert len(groups) == 8                                      # 3 sizes and the long scans, grey and colour
    for idxs in groups.values():                                 # ONE bbocr_jpeg_decode call per shape
        t, status = reader.decode_jpeg_batch([pages[i] for i in idxs])
        assert status == [0] * len(idxs), [files[i][0] for k, i in enumerate(idxs) if status[k]]
        t = t.cpu().numpy()
        for k, i in enumerate(idxs):
            assert np.array_equal(t[k], files[i][2]), files[i][0]
    n = len(pages)                                               # every file in ONE call, each into its own buffer with guard bytes behind it
    size = [p.shape[0] * p.shape[1] * p.shape[2] for p in pages]
    outs = [torch.full((sz + GUARD,), 9, dtype=torch.uint8, device=reader.device) for sz in size]
    files_c, sizes_c = reader._jpeg_files(pages)
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    pt = (C.c_longlong * n)(*[p.shape[1] * p.shape[2] for p in pages])
    status = (C.c_int * n)(*([1] * n))
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_jpeg_decode(reader._h, files_c, sizes_c, n, YCBCR3, op, pt, status))
    assert list(status) == [0] * n, [f[0] for f, s in zip(files, status) if s]
    for (name, _, want), o, sz in zip(files, outs, size):
        got = o.cpu().numpy()
        assert np.array_equal(got[:sz].reshape(want.shape), want), name
        assert (got[sz:] == 9).all(), name


def stage_cases():
    """the tables that miss the look-ahead, the swapped ids, a restart marker behind every MCU and fill bytes: grey, 4:2:0 and one chroma
    class at 56 x 40 / 47 x 33, and the long scans"""
    want = ("flat-10", "flat-16", "skewed", "ids-swapped", "ri-1", "fill-rst-eoi", "fill-rst-ri-1")
    out = [(n, d) for k, s in (("L", (56, 40)), ("420", (56, 40)), ("422", (47, 33))) for n, d in list_a(k, s) if n.split("x", 1)[1].split("-", 1)[1] in want]
    assert len(out) == 3 * len(want)
    return out + [(n, d) for n, _, d in big()]


@pytest.mark.parametrize("S", [32, 0])
def test_stage_states_and_coefficients_equal_the_restatement(reader, S):
    """the sequential decoder's states and coefficients, which the model of the device passes returns for these files
    (test_jpeg_forge_cpu.py), from two runs that agree bit for bit"""
    groups = 0
    for name, data in stage_cases():
        plan = K.parse(data)
        coef, states = K.decode_coefficients(data, plan, S or 1024)
        groups = max(groups, -(-len(states) // 64))
        for rep in range(2):
            got = stage(reader, 0, data, S, (len(states), 4), torch.int32)
            assert np.array_equal(got, states), (name, rep)
            got = stage(reader, 1, data, S, (coef.shape[0], 64), torch.int16)
            assert np.array_equal(got, coef), (name, rep)
            assert status_word(reader, data, S) == 0, (name, rep)
    assert groups > (2 if S else 1)                               # several workgroups of subsequences


def test_scales_equal_pillows_draft(reader):
    by = {n: d for k, s in (("L", (56, 40)), ("420", (56, 40)), ("422", (47, 33))) for n, d in list_a(k, s)}
    names = ["L-56x40-unary", "420-56x40-flat-16", "422-47x33-ids-swapped", "420-56x40-ri-1"]
    datas = [by[n] for n in names]
    decodes, status = reader.decode_jpeg_scales_batch(pages_of(datas), (1, 2, 4, 8))           # ONE call: the entropy stages run once per file
    assert status == [0] * 4
    for name, data, dec in zip(names, datas, decodes):
        for s in (1, 2, 4, 8):
            got = dec[s].cpu().numpy()
            want = pillow_pixels(data) if s == 1 else pillow_draft(data, s)
            assert np.array_equal(got[..., :3] if got.ndim == 3 else got, want), (name, s)
            if got.ndim == 3:
                assert (got[..., 3] == 255).all(), (name, s)


def test_list_c_status_words_are_the_models(reader, readers_trained):
    from bb_ocr_amd.reader import JpegPage, jpeg_plan

    cases = list_c()
    words = {name: model(data, K.parse(data))[3] for name, _, _, data in cases}
    assert 0 in words.values() and J.ERR_COUNT in words.values()
    for name, kind, size, data in cases:                          # exactly the model's bits
        assert status_word(reader, data) == words[name], name
    trained = readers_trained["fp16"]
    for kind, size in sorted({(k, s) for _, k, s, _ in cases}):   # ONE call per source: its files between two good ones
        mine = [(n, d) for n, k, s, d in cases if (k, s) == (kind, size)]
        good = source(kind, size)
        want = pillow_pixels(good)
        datas = [good] + [d for _, d in mine] + [good]
        t, status = reader.decode_jpeg_batch([JpegPage(d, jpeg_plan(d)) for d in datas])
        t = t.cpu().numpy()
        assert status[0] == 0 and status[-1] == 0 and np.array_equal(t[0], want) and np.array_equal(t[-1], want), kind
        for k, (name, data) in enumerate(mine, 1):
            assert status[k] == (ERR_DATA if words[name] else 0), name
            if words[name] == 0:
                assert np.array_equal(t[k], want), name
            else:
                assert reader.decode_jpeg_device([data], chroma=True) == [None], name
        if kind in KINDS:                                         # readtext of the bytes: the device decode, or the host's where it ends in a status
            for name, data in [m for m in mine if m[0].endswith(("last-1-zero", "last-64-zeros", "middle-64-pattern"))]:
                want_text = trained.readtext(data)
                trained.device_decode = True
                try:
                    got_text = trained.readtext(data)
                finally:
                    trained.device_decode = False
                assert got_text == want_text, name


def test_list_b_never_reaches_the_device(reader):
    before = reader.jpeg_counters()
    for name, data, reason, _ in list_b():
        assert reader.decode_jpeg_device([data], chroma=True) == [None], name
    assert reader.jpeg_counters() == before
    good = source("420", (47, 33))                                # and the counters do count
    assert reader.decode_jpeg_device([good])[0] is not None and reader.jpeg_counters()["files"] == before["files"] + 1
