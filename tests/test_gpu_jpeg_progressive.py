"""-m gpu: progressive JPEG files decoded on the device (csrc/jpegprog.hip) -- the coefficients after every scan against the restatement
of tests/jpeg_progressive_ref.py, so that a failure names the scan kind; the pixels at scale 1, 2, 4 and 8 against the installed Pillow's
full and draft decodes; the ``imread`` form against the host's ``cv2.imread`` page; a mixed batch with a damaged file; and the Python
routes that ride on ``device_decode="progressive"``.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_progressive_ref as P
from test_gpu_orient import host_imread
from test_jpeg_decode_cpu import picture, pillow_pixels, save
from test_jpeg_progressive_cpu import flat_eob_file, matrix, written
from test_jpeg_scaled_cpu import pillow_draft

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_DATA = -1, -7                                       # bbocr.h BBOCR_ERR_*
YCBCR4, YCBCR3 = 3, 4                                             # bbocr.h BBOCR_PAGE_*


def pick(size, mode, quality=75, restart=None, kind="noise"):
    name = "%dx%d-%s-q%d-r%s-%s" % (size[0], size[1], mode, quality, restart, kind)
    return next(d for n, _, d in matrix(size) if n == name)


STAGE_FILES = {
    "8x8-L": lambda: pick((8, 8), "L"),
    "17x9-420": lambda: pick((17, 9), "420"),                    # 3 luma blocks a row in its AC scans, 4 in the buffer
    "47x33-420": lambda: pick((47, 33), "420"),
    "47x33-444": lambda: pick((47, 33), "444"),
    "47x33-422": lambda: pick((47, 33), "422"),
    "47x33-440": lambda: pick((47, 33), "440"),
    "47x33-L": lambda: pick((47, 33), "L"),
    "64x48-r1": lambda: pick((64, 48), "420", restart=1),
    "64x48-r3": lambda: pick((64, 48), "420", restart=3),        # 12 MCUs, 48 luma blocks, 12 chroma blocks: four or sixteen whole segments
    "17x9-r3": lambda: pick((17, 9), "420", restart=3),          # 2 MCUs, 6 luma blocks, 2 chroma blocks: a short (last) segment
    "spectral": lambda: written("spectral"),
    "approx3": lambda: written("approx3"),
    "dc_apart": lambda: written("dc_apart"),
    "200x120": lambda: save(picture("noise", 200, 120, "RGB"), quality=90, progressive=True),   # first scans of several workgroups of subsequences
}
LANES = 64                                                       # subsequences per workgroup of the first scans' passes


def prog_stage(reader, stg, data, n_scans, S, shape, dtype, want_status=0):
    dst = torch.full(shape, 77, dtype=dtype, device=reader.device)
    st = C.c_int(1)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    reader._check(reader._lib.bbocr_op_jpeg_progressive_stage(reader._h, stg, buf, len(data), n_scans, S, C.c_void_p(dst.data_ptr()),
                                                              dst.numel() * dst.element_size(), C.byref(st)))
    assert st.value == want_status
    return dst.cpu().numpy()


def scan_kind(s):
    return ("DC" if s["ss"] == 0 else "AC") + (" first" if s["ah"] == 0 else " refinement")


@pytest.mark.parametrize("S", [0, 32])
@pytest.mark.parametrize("name", list(STAGE_FILES))
def test_coefficients_after_every_scan_equal_the_restatement(reader, name, S):
    data = STAGE_FILES[name]()
    plan = P.parse(data)
    assert plan["supported"]
    after = []
    final = P.decode_coefficients(data, plan, each=lambda k, c: after.append(c.copy()))
    assert len(after) == len(plan["scans"])
    if name in ("17x9-r3", "dc_apart"):                           # a last segment shorter than the interval
        assert any(P.scan_units(plan, s) % s["restart_interval"] for s in plan["scans"] if s["restart_interval"])
    if name == "200x120":                                         # states carried across workgroups, in DC first and AC first scans
        cut, subs = S or 1024, {}
        for sc in plan["scans"]:
            if sc["ah"] == 0:
                n = sum(max(-(-P.Bits(data[a:b]).n // cut), 1) for a, b in sc["segments"])
                subs[scan_kind(sc)] = max(subs.get(scan_kind(sc), 0), n)
        assert S != 32 or (subs["DC first"] > LANES and subs["AC first"] > 2 * LANES), subs      # 104 and 1528: 2 and 24 workgroups
    for k, want in enumerate(after):
        got = prog_stage(reader, 1, data, k + 1, S, want.shape, torch.int16)
        assert np.array_equal(got, want), (name, k, scan_kind(plan["scans"][k]))
    assert np.array_equal(prog_stage(reader, 1, data, 0, S, final.shape, torch.int16), final), name
    want_px = pillow_pixels(data)
    assert np.array_equal(prog_stage(reader, 3, data, 0, S, want_px.shape, torch.uint8), want_px), name


@pytest.mark.parametrize("S", [0, 32])
def test_end_of_band_runs_at_the_cap(reader, S):
    """the blocks of a run are counted at its symbol: with S = 32 a subsequence of four bytes completes 32,767 blocks"""
    data = flat_eob_file()
    plan = P.parse(data)
    want = P.decode_coefficients(data, plan)
    assert want.shape == (32768, 64)
    assert np.array_equal(prog_stage(reader, 1, data, 0, S, want.shape, torch.int16), want)
    assert np.array_equal(prog_stage(reader, 3, data, 0, 0, (1024, 2048), torch.uint8), pillow_pixels(data))


def progressive_pages(datas):
    from bb_ocr_amd.reader import jpeg_page

    pages = [jpeg_page(d, chroma=True, progressive=True) for d in datas]
    assert all(p is not None and p.progressive for p in pages) and all(jpeg_page(d, chroma=True) is None for d in datas)
    return pages


def test_every_scale_in_one_call_equals_pillows_full_and_draft_decodes(reader):
    names = ["17x9-420", "47x33-420", "47x33-444", "47x33-422", "47x33-440", "47x33-L", "64x48-r3", "approx3", "dc_apart"]
    datas = [STAGE_FILES[n]() for n in names] + [save(picture("gradient", 200, 120, "RGB"), quality=85, progressive=True)]
    decodes, status = reader.decode_jpeg_scales_batch(progressive_pages(datas), (1, 2, 4, 8))    # ONE bbocr_jpeg_decode_progressive call
    assert status == [0] * len(datas)
    for name, data, dec in zip(names + ["200x120"], datas, decodes):
        for s in (1, 2, 4, 8):
            want = pillow_pixels(data) if s == 1 else pillow_draft(data, s)
            got = dec[s].cpu().numpy()
            assert np.array_equal(got[..., :3] if got.ndim == 3 else got, want), (name, s)
            assert got.ndim == 2 or (got[..., 3] == 255).all(), (name, s)
    for s in (1, 4):                                              # the one-output form behind decode_jpeg_batch
        t, status = reader.decode_jpeg_batch(progressive_pages(datas[1:3]), scale=s)
        assert status == [0, 0]
        for k in range(2):
            assert np.array_equal(t[k].cpu().numpy(), pillow_pixels(datas[1 + k]) if s == 1 else pillow_draft(datas[1 + k], s)), (k, s)


def test_imread_with_orientation_6_equals_the_host(reader):
    from bb_ocr_amd.preprocess import IMREAD_JPEG, IMREAD_YCC, imread_bgr_device

    data = written("exif6")
    want = host_imread(reader, data)
    assert tuple(want.shape) == (47, 33, 3)
    outs, status = reader.imread_jpeg_batch(progressive_pages([data]))
    assert status == [0] and torch.equal(outs[0], want)
    decodes, status = reader.decode_jpeg_scales_batch(progressive_pages([data]), (1, 2), imread=True)
    assert status == [0] and torch.equal(decodes[0][1], want)
    assert np.array_equal(decodes[0][2].cpu().numpy()[..., :3], pillow_draft(data, 2))
    got = imread_bgr_device(reader, data, device_decode="progressive")
    assert got.imread_path == IMREAD_JPEG and torch.equal(got, want)
    for option in ("chroma", True, None):                         # the host's decode, oriented on the card: as before
        got = imread_bgr_device(reader, data, option)
        assert got.imread_path == IMREAD_YCC and torch.equal(got, want)


def damaged_refinement():
    """A 200 x 120 progressive 4:2:0 file with 64 bytes inside its first AC refinement scan overwritten (no byte becomes FF: the markers
    and the plan stay as they were), which the restatement cannot decode"""
    data = save(picture("noise", 200, 120, "RGB"), quality=90, progressive=True)
    plan = P.parse(data)
    s = next(s for s in plan["scans"] if s["ss"] > 0 and s["ah"] > 0)
    assert s["bytes"] > 400
    a = s["offset"] + s["bytes"] // 2
    bad = bytearray(data)
    bad[a:a + 64] = bytes((37 * k + 11) % 251 for k in range(64))
    bad = bytes(bad)
    damaged = P.parse(bad)
    assert damaged["supported"] and [x["bytes"] for x in damaged["scans"]] == [x["bytes"] for x in plan["scans"]]
    with pytest.raises(ValueError):
        P.decode_coefficients(bad, damaged)
    return data, bad


def test_mixed_batch_with_a_png_and_a_damaged_file(reader):
    import io

    from PIL import Image

    from bb_ocr_amd import _lib

    good, bad = damaged_refinement()
    png = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(png, "PNG")
    datas = [STAGE_FILES["47x33-420"](), STAGE_FILES["47x33-444"](), STAGE_FILES["47x33-L"](), save(picture("noise", 56, 40, "RGB"), quality=75),
             png.getvalue(), bad]
    shapes = [(33, 47, 3), (33, 47, 3), (33, 47), (40, 56, 3), (8, 8, 3), (120, 200, 3)]
    n = len(datas)
    bufs = [(C.c_ubyte * len(d)).from_buffer_copy(d) for d in datas]
    files = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_size_t * n)(*[len(d) for d in datas])
    for rep in range(2):                                          # the second call: the context stays usable behind a damaged file
        outs = [torch.full(s, 9, dtype=torch.uint8, device=reader.device) for s in shapes]
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        pitches = (C.c_longlong * n)(*[s[1] * (3 if len(s) == 3 else 1) for s in shapes])
        out = _lib.bbocr_jpeg_output(1, _lib.JPEG_FORM_YCBCR, ptrs, pitches)
        status = (C.c_int * n)(*([1] * n))
        torch.cuda.synchronize()
        reader._check(reader._lib.bbocr_jpeg_decode_progressive(reader._h, files, sizes, n, YCBCR3, C.byref(out), 1, status))
        assert list(status) == [0, 0, 0, 0, ERR_ARG, ERR_DATA], rep
        for k in range(4):
            assert np.array_equal(outs[k].cpu().numpy(), pillow_pixels(datas[k])), (rep, k)
        assert (outs[4] == 9).all()                               # a refused file's destination is never written
    t, status = reader.decode_jpeg_batch(progressive_pages([good]))
    assert status == [0] and np.array_equal(t[0].cpu().numpy(), pillow_pixels(good))
    assert reader.decode_jpeg_device([bad], progressive=True) == [None] and reader.decode_jpeg_device([good]) == [None]
    assert reader.decode_jpeg_device([good], progressive=True)[0] is not None


def test_existing_calls_keep_refusing_a_progressive_file(reader):
    from bb_ocr_amd import _lib

    data = STAGE_FILES["47x33-420"]()
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    files, sizes = (C.c_void_p * 1)(C.addressof(buf)), (C.c_size_t * 1)(len(data))
    o = torch.zeros((33, 47, 3), dtype=torch.uint8, device=reader.device)
    ptrs, pitches = (C.c_void_p * 1)(o.data_ptr()), (C.c_longlong * 1)(47 * 3)
    out = _lib.bbocr_jpeg_output(1, _lib.JPEG_FORM_YCBCR, ptrs, pitches)
    for call in (lambda st: reader._lib.bbocr_jpeg_decode(reader._h, files, sizes, 1, YCBCR3, ptrs, pitches, st),
                 lambda st: reader._lib.bbocr_jpeg_imread(reader._h, files, sizes, 1, ptrs, pitches, st),
                 lambda st: reader._lib.bbocr_jpeg_decode_scaled(reader._h, files, sizes, 1, YCBCR3, 2, ptrs, pitches, st),
                 lambda st: reader._lib.bbocr_jpeg_decode_scales(reader._h, files, sizes, 1, YCBCR3, C.byref(out), 1, st)):
        status = (C.c_int * 1)(1)
        reader._check(call(status))
        assert list(status) == [ERR_ARG]
    before = reader.jpeg_counters()
    reader.decode_jpeg_batch(progressive_pages([data]))
    after = reader.jpeg_counters()
    assert [after[k] - before[k] for k in ("files", "entropy_runs", "idct_passes", "output_passes")] == [1, 1, 1, 1]


def test_preview_takes_the_device_route_only_when_asked(reader):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import preview_device, preview_host

    page = Image.fromarray(synth.page(41, width=640, height=480, lines=10, margin=24)[0])
    for kw in (dict(subsampling=2), dict(subsampling=0, restart_marker_blocks=7)):
        data = save(page, quality=90, progressive=True, **kw)
        for max_dim in (800, 150):                                # as decoded, and through a draft scale
            want = preview_host(data, max_dim)
            info = {}
            assert preview_device(reader, data, max_dim, device_decode="progressive", info=info) == want and info == {"route": "device-jpeg"}
            for option in ("chroma", True):
                assert preview_device(reader, data, max_dim, device_decode=option, info=info) == want and info == {"route": "host"}


@pytest.fixture(scope="module")
def progressive_reader(states_trained):
    import bb_ocr_amd

    r = bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, precision="fp16", device_decode="progressive")
    yield r
    r.close()


def test_read_files_over_baseline_and_progressive_pages_returns_the_texts_of_the_option_off(progressive_reader, tmp_path):
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.extractor_batch import read_files

    r = progressive_reader
    assert r.device_decode is True and r.jpeg_chroma is True and r.jpeg_progressive is True and r.decode_option == "progressive"
    paths = []
    for i, kw in enumerate([dict(), dict(progressive=True), dict(progressive=True, subsampling=0), dict(subsampling=1), dict(progressive=True)]):
        paths.append(str(tmp_path / ("page%d.jpg" % i)))
        Image.fromarray(synth.page(3 + i, width=640, height=480, lines=12, margin=24)[0]).save(paths[-1], "JPEG", quality=90, **kw)
    assert r.jpeg_progressive_plan(paths[1]).supported == 1 and r.jpeg_progressive_plan(paths[0]).supported == 0
    got = read_files(r, paths, device_decode="progressive")
    want = read_files(r, paths)
    assert got == want and all(len(want[i]) > 0 for i in range(len(paths)))
    assert r.readtext_files(paths) == r.readtext_files(paths, device_decode=False)
