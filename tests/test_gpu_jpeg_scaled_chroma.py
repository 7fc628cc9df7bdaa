"""-m gpu: the scaled decode of the chroma classes and the shared entropy pass on the device (csrc/jpegdec.hip's jd_idct / jd_output on
the host's geometry table, bbocr_jpeg_decode_scales, bbocr_op_jpeg_scaled_class_stage, bbocr_jpeg_counters) against the restatement of
tests/jpeg_scaled_chroma_ref.py, the installed Pillow's draft and the single-purpose entry points, bit for bit; then the previews that
ride on them (preprocess.preview_device(device_decode="chroma"), extractor_batch.trace_previews) against preprocess.preview_host."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import jpeg_chroma_ref as K
import jpeg_scaled_chroma_ref as SC
import jpeg_scaled_ref as S
from test_gpu_jpeg_scaled import decode_scaled
from test_gpu_preview import icc_profile
from test_jpeg_decode_cpu import picture, pillow_pixels, save
from test_jpeg_scaled_chroma_cpu import CLASSES, class_file
from test_jpeg_scaled_cpu import SCALES, pillow_draft

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_DATA = -1, -7                                        # bbocr.h BBOCR_ERR_*
from bb_ocr_amd._lib import JPEG_FORM_IMREAD as IMREAD, JPEG_FORM_YCBCR as YCBCR, PAGE_YCBCR3 as YCBCR3, PAGE_YCBCR4 as YCBCR4  # noqa: E402

# 130x257 noise at quality 95 spans several jd_sync workgroups; the narrow sizes reach the replication branch inside the fancy helpers
STAGE_SIZES = [(1, 1), (3, 2), (8, 9), (17, 15), (2, 37), (37, 2), (33, 50), (130, 257)]
FILL = 93


@functools.lru_cache(maxsize=None)
def stage_files(size):
    """[(name, file bytes, plan, coefficients)] of one size: classes x {noise q95, gradient q30}; one reference decode serves every test"""
    out = []
    for cls in CLASSES:
        for kind, q in (("noise", 95), ("gradient", 30)):
            data = class_file(cls, kind, size[0], size[1], quality=q)
            plan = K.parse(data)
            out.append(("%dx%d-%s-q%d-c%d" % (size + (kind, q, cls)), data, plan, K.decode_coefficients(data, plan)[0]))
    return out


def class_stage(reader, stg, data, s, nbytes):
    dst = torch.full((nbytes + 16,), FILL, dtype=torch.uint8, device=reader.device)
    st = C.c_int(1)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_op_jpeg_scaled_class_stage(reader._h, stg, buf, len(data), s, C.c_void_p(dst.data_ptr()), nbytes, C.byref(st)))
    assert st.value == 0
    a = dst.cpu().numpy()
    assert np.all(a[nbytes:] == FILL)
    return a[:nbytes]


@pytest.mark.parametrize("size", STAGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_stage_planes_and_pixels_equal_the_restatement_and_pillow(reader, size):
    from bb_ocr_amd.reader import jpeg_plan

    for name, data, plan, coef in stage_files(size):
        if size == (130, 257) and "noise" in name:
            assert -(-int(jpeg_plan(data).scan_bytes) * 8 // 1024) > 64, name           # more than one workgroup of subsequences
        for s in SCALES:
            planes = [p.astype(np.uint8) for p in SC.scaled_planes(coef, plan, s)]
            geo = SC.geometry(plan, s)
            assert [p.shape for p in planes] == [(g[1], g[2]) for g in geo]
            got = class_stage(reader, 2, data, s, sum(p.size for p in planes))
            assert np.array_equal(got, np.concatenate([p.ravel() for p in planes])), (name, s)
            want = SC.planes_to_pixels(planes, plan, s)
            assert np.array_equal(want, pillow_draft(data, s)), (name, s)
            assert np.array_equal(class_stage(reader, 3, data, s, want.size).reshape(want.shape), want), (name, s)


def test_class_stage_refuses_everything_else(reader):
    dst = torch.zeros(1 << 16, dtype=torch.uint8, device=reader.device)
    for data in (save(picture("noise", 40, 24, "RGB"), quality=80), save(picture("noise", 40, 24, "L"), quality=80),
                 save(picture("noise", 40, 24, "RGB"), quality=80, subsampling=0, progressive=True)):
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        assert reader._lib.bbocr_op_jpeg_scaled_class_stage(reader._h, 3, buf, len(data), 2, C.c_void_p(dst.data_ptr()), dst.numel(), None) == ERR_ARG
    data = class_file(K.C422, "noise", 24, 40, quality=80)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    for stg, s, nbytes in ((1, 2, dst.numel()), (3, 1, dst.numel()), (3, 3, dst.numel()), (3, 2, 10), (2, 2, 10)):
        assert reader._lib.bbocr_op_jpeg_scaled_class_stage(reader._h, stg, buf, len(data), s, C.c_void_p(dst.data_ptr()), nbytes, None) == ERR_ARG
    # and the existing stage entry point keeps refusing the classes
    assert reader._lib.bbocr_op_jpeg_scaled_stage(reader._h, 3, buf, len(data), 2, C.c_void_p(dst.data_ptr()), dst.numel(), None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ bbocr_jpeg_decode_scales
def decode_scales(reader, datas, outputs, layout=YCBCR4, pad=0, offset=0, guard=32, expect_rc=0):
    """ONE bbocr_jpeg_decode_scales call.  ``outputs``: [(scale, form)].  Every destination lies `offset` bytes into a buffer of its own
    with rows `pad` bytes longer than the pixels and `guard` bytes behind the last row; everything but the pixels must come back
    untouched -> ([{scale: array or None} per file], [status])"""
    from bb_ocr_amd import _lib
    from bb_ocr_amd.reader import jpeg_plan

    n = len(datas)
    plans = [jpeg_plan(d) for d in datas]
    outs = (_lib.bbocr_jpeg_output * len(outputs))()
    keep, shapes = [], []
    for o, (s, form) in enumerate(outputs):
        bufs, geo = [], []
        for p in plans:
            H, W = max(p.height, 1), max(p.width, 1)
            if form == IMREAD:
                rows, cols, px = (W, H, 3) if p.orientation >= 5 else (H, W, 3)
            else:
                rows, cols = S.scaled_dims(H, W, s)
                px = 1 if p.components == 1 else (4 if layout == YCBCR4 else 3)
            pitch = cols * px + pad
            bufs.append(torch.full((offset + rows * pitch + guard,), FILL, dtype=torch.uint8, device=reader.device))
            geo.append((rows, cols, px, pitch))
        ptrs = (C.c_void_p * n)(*[b.data_ptr() + offset for b in bufs])
        pitches = (C.c_longlong * n)(*[g[3] for g in geo])
        outs[o].scale, outs[o].form, outs[o].dev_out, outs[o].pitches = s, form, ptrs, pitches
        keep.append((bufs, ptrs, pitches))
        shapes.append(geo)
    fb = [(C.c_ubyte * len(d)).from_buffer_copy(d) for d in datas]
    fl = (C.c_void_p * n)(*[C.addressof(b) for b in fb])
    sz = (C.c_size_t * n)(*[len(d) for d in datas])
    status = (C.c_int * n)(*([77] * n))
    torch.cuda.synchronize()
    rc = reader._lib.bbocr_jpeg_decode_scales(reader._h, fl, sz, n, layout, outs, len(outputs), status)
    assert rc == expect_rc, (rc, reader._lib.bbocr_last_error(reader._h))
    res = [{} for _ in datas]
    for o, (s, form) in enumerate(outputs):
        for k, (buf, (rows, cols, px, pitch)) in enumerate(zip(keep[o][0], shapes[o])):
            a = buf.cpu().numpy()
            assert np.all(a[:offset] == FILL) and np.all(a[offset + rows * pitch:] == FILL), (k, s)
            a = a[offset:offset + rows * pitch].reshape(rows, pitch)
            assert np.all(a[:, cols * px:] == FILL), (k, s)
            if rc != 0 or status[k] != 0:
                if rc != 0 or status[k] == ERR_ARG:
                    assert np.all(a == FILL), (k, s)                        # a refused file's destinations are never written
                res[k][s] = None
                continue
            a = a[:, :cols * px]
            res[k][s] = a if px == 1 else a.reshape(rows, cols, px)
    return res, list(status)


def strip(a):
    """the padded pixels' fourth byte is 255"""
    if a.ndim == 3 and a.shape[2] == 4:
        assert np.all(a[..., 3] == 255)
        return a[..., :3]
    return a


def want_at(data, s):
    return pillow_pixels(data) if s == 1 else pillow_draft(data, s)


@functools.lru_cache(maxsize=None)
def batch_files():
    """{name: bytes}: 4:2:0, grey, the three classes (one with a restart interval), a progressive file and a file with 64 damaged bytes"""
    from bb_ocr_amd.reader import jpeg_plan

    good = {
        "420": save(picture("noise", 200, 120, "RGB"), quality=90),
        "grey": save(picture("gradient", 67, 33, "L"), quality=80),
        "444": class_file(K.C444, "noise", 33, 50, quality=90),
        "422-rst": class_file(K.C422, "noise", 130, 257, quality=95, restart_marker_rows=1),
        "440": class_file(K.C440, "gradient", 37, 18, quality=75),
        "420-small": save(picture("gradient", 5, 3, "RGB"), quality=75),
    }
    bad = bytearray(class_file(K.C422, "noise", 130, 257, quality=95))
    plan = jpeg_plan(bytes(bad))
    a = int(plan.scan_offset) + int(plan.scan_bytes) // 2
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))     # no FF: the markers and the plan stay as they were
    files = dict(good)
    files["progressive"] = save(picture("noise", 64, 48, "RGB"), quality=90, progressive=True)
    files["damaged"] = bytes(bad)
    order = ["420", "444", "progressive", "grey", "422-rst", "damaged", "440", "420-small"]
    return {k: files[k] for k in order}


def test_decode_scales_equals_the_single_purpose_calls_and_pillow(reader):
    from bb_ocr_amd.reader import jpeg_page

    files = batch_files()
    names, datas = list(files), list(files.values())
    ok = [k for k, nm in enumerate(names) if nm not in ("progressive", "damaged")]
    want_status = [0 if k in ok else (ERR_ARG if names[k] == "progressive" else ERR_DATA) for k in range(len(names))]
    before = reader.jpeg_counters()
    # {1, 2}
    got, status = decode_scales(reader, datas, [(1, YCBCR), (2, YCBCR)])
    assert status == want_status
    after = reader.jpeg_counters()
    taken = len(names) - 1                                            # every file but the progressive one runs
    assert {k: after[k] - before[k] for k in after} == dict(files=taken, entropy_runs=taken, idct_passes=2 * taken, output_passes=2 * taken)
    for k in ok:
        for s in (1, 2):
            assert np.array_equal(strip(got[k][s]), want_at(datas[k], s)), (names[k], s)
    # the files bbocr_jpeg_decode_scaled takes come out as it writes them, all of them as bbocr_jpeg_decode writes them
    plain = [k for k in ok if names[k] in ("420", "grey", "420-small")]
    single, st = decode_scaled(reader, [datas[k] for k in plain], 2, YCBCR4)
    assert st == [0] * len(plain) and all(np.array_equal(single[i], got[k][2]) for i, k in enumerate(plain))
    pages = [jpeg_page(datas[k], chroma=True) for k in ok]
    for k, p in zip(ok, pages):
        t, st = reader.decode_jpeg_batch([p], padded=True)
        assert st == [0] and np.array_equal(t[0].cpu().numpy(), got[k][1]), names[k]
    # {1 imread, 4}
    got, status = decode_scales(reader, datas, [(4, YCBCR), (1, IMREAD)], layout=YCBCR3)
    assert status == want_status
    single, st = reader.imread_jpeg_batch(pages)
    assert st == [0] * len(ok)
    for i, k in enumerate(ok):
        assert np.array_equal(got[k][1], single[i].cpu().numpy()), names[k]
        assert np.array_equal(got[k][4], want_at(datas[k], 4)), names[k]
    # {8}
    got, status = decode_scales(reader, datas, [(8, YCBCR)], layout=YCBCR3)
    assert status == want_status
    for k in ok:
        assert np.array_equal(got[k][8], want_at(datas[k], 8)), names[k]
    # all four scales at once; the context is still usable and the damaged file's neighbours were decoded
    got, status = decode_scales(reader, datas, [(8, YCBCR), (1, YCBCR), (4, YCBCR), (2, YCBCR)])
    assert status == want_status
    for k in ok:
        for s in (1, 2, 4, 8):
            assert np.array_equal(strip(got[k][s]), want_at(datas[k], s)), (names[k], s)


@pytest.mark.parametrize("layout,pad,offset", [(YCBCR3, 0, 0), (YCBCR3, 5, 1), (YCBCR4, 0, 0), (YCBCR4, 8, 4), (YCBCR4, 3, 0), (YCBCR4, 0, 3)])
def test_destination_layouts_and_guard_bytes(reader, layout, pad, offset):
    """3 and 4 bytes per pixel, odd pitches and destinations at odd byte offsets (the output kernel's byte path), whole words (its dword
    path), at scale 1 and the draft scales, every class: the pixels are Pillow's and no byte outside them is written.  The 1 x 1 and
    3 x 2 files (H x W) reach the narrow-plane branch of the h2v2 fancy upsampling"""
    datas = [d for size in ((17, 15), (2, 37), (33, 50)) for _, d, _, _ in stage_files(size)]
    datas += [save(picture("noise", 50, 33, "RGB"), quality=85), save(picture("noise", 50, 33, "L"), quality=85)]
    datas += [save(picture("noise", w, h, mode), quality=85) for mode in ("RGB", "L") for h, w in ((1, 1), (3, 2))]
    got, status = decode_scales(reader, datas, [(1, YCBCR), (2, YCBCR), (4, YCBCR), (8, YCBCR)], layout=layout, pad=pad, offset=offset)
    assert status == [0] * len(datas)
    for k, d in enumerate(datas):
        for s in (1,) + tuple(SCALES):
            assert np.array_equal(strip(got[k][s]), want_at(d, s)), (k, s)


def test_argument_errors_are_returned_before_any_work(reader):
    datas = [class_file(K.C422, "gradient", 24, 40, quality=80)]
    before = reader.jpeg_counters()
    for outputs in ([(2, YCBCR), (2, YCBCR)], [(1, YCBCR), (1, IMREAD)], [(2, IMREAD)], [(3, YCBCR)], [(2, 7)], []):
        decode_scales(reader, datas, outputs, expect_rc=ERR_ARG)          # and every destination byte is untouched
    decode_scales(reader, datas, [(2, YCBCR)], layout=1, expect_rc=ERR_ARG)
    lib, h = reader._lib, reader._h
    assert lib.bbocr_jpeg_decode_scales(h, None, None, 1, YCBCR3, None, 1, None) == ERR_ARG
    assert lib.bbocr_jpeg_counters(h, None) == ERR_ARG
    assert reader.jpeg_counters() == before
    # a destination that is too narrow, or missing, refuses that file alone
    got, status = decode_scales(reader, datas * 2, [(2, YCBCR)], pad=-1)
    assert status == [ERR_ARG, ERR_ARG] and reader.jpeg_counters() == before
    got, status = decode_scales(reader, datas, [(2, YCBCR)])
    assert status == [0] and np.array_equal(strip(got[0][2]), pillow_draft(datas[0], 2))
    # the calls that are pinned: a chroma class at a draft scale is refused by bbocr_jpeg_decode_scaled and decode_jpeg_device
    assert decode_scaled(reader, datas, 2)[1] == [ERR_ARG]
    assert reader.decode_jpeg_device(datas, chroma=True, scale=2) == [None]


def test_reader_decode_jpeg_scales(reader):
    files = batch_files()
    names, datas = list(files), list(files.values())
    out = reader.decode_jpeg_scales(datas, scales=(1, 4), chroma=True)
    assert [o is None for o in out] == [nm in ("progressive", "damaged") for nm in names]
    one = reader.decode_jpeg_device(datas, chroma=True)
    for nm, d, o, w in zip(names, datas, out, one):
        if o is None:
            continue
        assert sorted(o) == [1, 4]
        assert torch.equal(o[1][0], w[0]) and torch.equal(o[1][1], w[1]), nm
        ycc = pillow_draft(d, 4)
        assert np.array_equal(o[4][1].cpu().numpy(), ycc if ycc.ndim == 2 else ycc[..., 0]) and o[4][0].shape == ycc.shape[:2] + (3,), nm
    # without the option the classes stay with the host; with imread the scale-1 entry is cv2.imread's page
    out = reader.decode_jpeg_scales(datas, scales=(2,), chroma=False)
    assert [o is None for o in out] == [nm not in ("420", "grey", "420-small") for nm in names]
    out = reader.decode_jpeg_scales([files["440"]], scales=(2, 1), chroma=True, imread=True)
    from bb_ocr_amd.reader import jpeg_page

    assert torch.equal(out[0][1], reader.imread_jpeg_batch([jpeg_page(files["440"], True)])[0][0])
    with pytest.raises(ValueError):
        reader.decode_jpeg_scales(datas, scales=(2, 2))
    with pytest.raises(ValueError):
        reader.decode_jpeg_scales(datas, scales=(2,), imread=True)


# ------------------------------------------------------------------------------------------------ the previews
def test_preview_of_chroma_class_files_equals_the_host_preview(reader):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preview_device, preview_host
    from bb_ocr_amd.reader import jpeg_plan

    page = Image.fromarray(synth.page(64, width=1900, height=1300, lines=12, margin=40, colour=True)[0])
    exif = Image.Exif()
    exif[0x0112] = 6
    tagged = save(page, quality=90, subsampling=1, icc_profile=icc_profile(), exif=exif)
    assert jpeg_plan(tagged).orientation == 6 and jpeg_plan(tagged).chroma == K.C422
    tall = K.make_440(save(picture("gradient", 900, 40, "RGB"), quality=85, subsampling=1))          # 40 wide, 900 high
    cases = [
        ("422-icc-exif6", tagged, 800), ("422-icc-exif6-draft2", tagged, 300), ("422-draft4", tagged, 150), ("422-draft8", tagged, 75),
        ("444", save(page, quality=90, subsampling=0), 800), ("444-draft2", save(page, quality=90, subsampling=0), 301),
        ("444-odd-draft4", save(picture("gradient", 1901, 1299, "RGB"), quality=85, subsampling=0), 150),
        ("440-tall", tall, 800), ("440-tall-draft2", tall, 10), ("440-small", class_file(K.C440, "noise", 97, 333, quality=90), 800),
        ("422-small", class_file(K.C422, "noise", 480, 640, quality=90), 800), ("444-small", class_file(K.C444, "noise", 222, 333, quality=90), 800),
    ]
    seen = set()
    for name, data, m in cases:
        plan = jpeg_plan(data)
        assert plan.chroma and not plan.supported, name
        seen.add((plan.chroma, max(plan.height, plan.width) > m))
        want = preview_host(data, m)
        info = {}
        assert preview_device(reader, data, m, device_decode="chroma", info=info) == want, name
        assert info == {"route": "device-jpeg"}, name
        assert preview_device(reader, data, m, device_decode=True, info=info) == want and info == {"route": "host"}, name
        assert preview_device(reader, data, m, device_decode=False, info=info) == want and info == {"route": "host"}, name
    assert seen == {(c, big) for c in CLASSES for big in (False, True)}
    # a file inside the plan's own scope takes the card either way; a page on the card is "device-page"
    info = {}
    data = save(page, quality=90)
    assert preview_device(reader, data, 300, device_decode=True, info=info) == preview_host(data, 300) and info == {"route": "device-jpeg"}
    assert preview_device(reader, data, 300, device_decode="chroma", info=info) == preview_host(data, 300) and info == {"route": "device-jpeg"}
    dev = reader._to_dev(np.ascontiguousarray(np.asarray(page)[:, :, ::-1]))
    assert preview_device(reader, dev, info=info) == preview_host(np.ascontiguousarray(np.asarray(page)[:, :, ::-1])) and info == {"route": "device-page"}


@pytest.mark.parametrize("subsampling,option", [(2, True), (1, "chroma")], ids=["420", "422"])
def test_trace_previews_decode_the_cover_once(reader, tmp_path, subsampling, option):
    """test_gpu_preview's construction on a 4:2:0 and a 4:2:2 cover: the four strings are those of four preview_host calls, and the file
    went through the entropy stages once"""
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.extractor_batch import trace_previews
    from bb_ocr_amd.preprocess import _imread_bgr, auto_crop_box_device, central_edge_crop_box, preprocess_bgr_device, preview_host

    path = str(tmp_path / "cover.jpg")
    exif = Image.Exif()
    exif[0x0112] = 3 if subsampling == 1 else 1
    Image.fromarray(synth.page(63, width=1280, height=960, lines=8, margin=150)[0]).save(path, "JPEG", quality=90, subsampling=subsampling, exif=exif)
    kw = dict(use_preprocessing=True, edge_crop_percent=4.0, crop_for_ocr=True, crop_margin=32)
    before = reader.jpeg_counters()
    got = trace_previews(reader, [path], device_decode=option, **kw)
    after = reader.jpeg_counters()
    assert (after["files"] - before["files"], after["entropy_runs"] - before["entropy_runs"]) == (1, 1)
    pre = preprocess_bgr_device(reader, reader._to_dev(_imread_bgr(path))).cpu().numpy()
    b = central_edge_crop_box(pre.shape[0], pre.shape[1], 4.0)
    edge = np.ascontiguousarray(pre[b[1]:b[3], b[0]:b[2]])
    a = auto_crop_box_device(reader, reader._to_dev(edge), 32)
    assert a is not None
    auto = np.ascontiguousarray(edge[a[1]:a[3], a[0]:a[2]])
    want = {"original_b64": preview_host(path), "preprocessed_b64": preview_host(pre), "edge_cropped_b64": preview_host(edge),
            "auto_cropped_b64": preview_host(auto)}
    assert got == [want]
    if option == "chroma":                                              # without the option the file is the host's, as before
        before = reader.jpeg_counters()
        assert trace_previews(reader, [path], device_decode=True, **kw) == [want]
        assert reader.jpeg_counters() == before


def test_trace_previews_share_the_pass_between_the_draft_scale_and_the_full_page(reader, tmp_path):
    """a 4:2:2 page large enough for draft scale 2 (and orientation 6): the original's preview comes from the 1/2 output and the crop chain
    from the scale-1 imread output of ONE call -- 1 entropy run, 2 IDCT passes -- and the strings are those of the host-decoded trace"""
    from PIL import Image

    from bb_ocr_amd.extractor_batch import trace_previews
    from bb_ocr_amd.preprocess import preview_draft_scale, preview_host
    from bb_ocr_amd.reader import jpeg_plan

    path = str(tmp_path / "page.jpg")
    exif = Image.Exif()
    exif[0x0112] = 6
    picture("gradient", 3300, 3210, "RGB").save(path, "JPEG", quality=80, subsampling=1, exif=exif, icc_profile=icc_profile())
    plan = jpeg_plan(open(path, "rb").read())
    assert plan.chroma == K.C422 and preview_draft_scale(plan) == 2
    kw = dict(use_preprocessing=True, edge_crop_percent=4.0)
    before = reader.jpeg_counters()
    got = trace_previews(reader, [path], device_decode="chroma", **kw)
    after = reader.jpeg_counters()
    assert {k: after[k] - before[k] for k in after} == dict(files=1, entropy_runs=1, idct_passes=2, output_passes=2)
    assert got == trace_previews(reader, [path], device_decode=False, **kw) and reader.jpeg_counters() == after
    assert got[0]["original_b64"] == preview_host(path) and sorted(got[0]) == ["edge_cropped_b64", "original_b64", "preprocessed_b64"]
