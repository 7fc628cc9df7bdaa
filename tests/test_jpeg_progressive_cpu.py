"""Progressive JPEG files without a GPU: the restatement of tests/jpeg_progressive_ref.py equals the installed Pillow / libjpeg-turbo bit
for bit -- on files Pillow writes (every sampling, restart intervals, an end-of-band run at the format's cap) and on scripts it never
writes (``jpeg_progressive_ref.write``); ``bbocr_host_jpeg_progressive_plan`` (csrc/jpeg_parse.h) equals its plan field by field and
refuses what is out of scope, each with its reason, while ``bbocr_host_jpeg_plan`` answers as before; and ``device_decode="progressive"``
-- nothing else -- routes such a file to the device decoder."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_chroma_ref as K
import jpeg_progressive_ref as P
import test_read_files_cpu as R
from test_jpeg_decode_cpu import c_plan, lib, picture, pillow_pixels, save  # noqa: F401  (lib: a fixture)
from test_read_files_cpu import files  # noqa: F401  (a fixture)

SIZES = [(8, 8), (16, 16), (17, 9), (47, 33), (64, 48)]                              # width x height
MODES = ["420", "444", "422", "L", "440"]
QUALITIES = [30, 75, 95]
RESTARTS = [None, 1, 3]
KINDS = ["noise", "gradient", "flat", "page"]
SUBSAMPLING = {"420": 2, "444": 0, "422": 1}
# libjpeg's default progression (jcparam.c jpeg_simple_progression), which Pillow writes: 10 scans for colour, 6 for grey
SCRIPT_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                 ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
SCRIPT_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


@functools.lru_cache(maxsize=None)
def _page():
    from bb_ocr_amd import synth

    return synth.page(41, width=320, height=192, lines=4, margin=16, colour=True)[0]


def image(kind, w, h, mode):
    from PIL import Image

    if kind != "page":
        return picture(kind, w, h, mode)
    crop = Image.fromarray(_page()[40:40 + h, 24:24 + w])
    return crop if mode == "RGB" else crop.convert("L")


def baseline_coefficients(data):
    """(coefficients, frame) of a baseline file jpeg_chroma_ref decodes: what ``P.write`` codes again"""
    plan = K.parse(data)
    return K.decode_coefficients(data, plan)[0], plan


def progressive_file(kind, w, h, mode, quality, restart):
    """One file of the matrix.  4:4:0 is made the way the chroma tests make it -- jpeg_chroma_ref.make_440 of the transposed 4:2:2 file --
    and coded again with libjpeg's default progression by the scan writer; every other file is Pillow's own."""
    if mode == "440":
        coef, plan = baseline_coefficients(K.make_440(save(image(kind, h, w, "RGB"), quality=quality, subsampling=1)))
        return P.write(coef, plan, SCRIPT_COLOUR, restart)
    kw = dict(quality=quality, progressive=True)
    if restart:
        kw["restart_marker_blocks"] = restart
    if mode != "L":
        kw["subsampling"] = SUBSAMPLING[mode]
    return save(image(kind, w, h, "L" if mode == "L" else "RGB"), **kw)


@functools.lru_cache(maxsize=None)
def matrix(size):
    """[(name, mode, file bytes)] of one size: 5 modes x 3 qualities x 3 restart settings x 4 picture kinds = 180 files"""
    w, h = size
    return [("%dx%d-%s-q%d-r%s-%s" % (w, h, mode, q, r, kind), mode, progressive_file(kind, w, h, mode, q, r))
            for mode in MODES for q in QUALITIES for r in RESTARTS for kind in KINDS]


@functools.lru_cache(maxsize=None)
def written(name):
    """The files of scripts Pillow never writes, coded by ``P.write`` from the coefficients of a baseline file:
    spectral     4:2:0 47 x 33: spectral selection only, no successive approximation
    approx3      grey 64 x 48: Al = 3 and three refinement steps, for DC and for AC
    dc_apart     4:2:0 40 x 24 (5 luma blocks a row in a scan of its own, 6 in the MCU raster): every DC scan non-interleaved, restart
                 intervals of 2 and 3 blocks in the luma scans, the default progression's approximation behind them
    exif6        4:2:0 47 x 33 behind an EXIF block of orientation 6, libjpeg's default progression"""
    if name == "spectral":
        coef, plan = baseline_coefficients(save(picture("noise", 47, 33, "RGB"), quality=85))
        return P.write(coef, plan, [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 6, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)])
    if name == "approx3":
        coef, plan = baseline_coefficients(save(picture("noise", 64, 48, "L"), quality=95))
        script = [((0,), 0, 0, 0, 3), ((0,), 1, 63, 0, 3)]
        for a in (3, 2, 1):
            script += [((0,), 0, 0, a, a - 1), ((0,), 1, 20, a, a - 1), ((0,), 21, 63, a, a - 1)]
        return P.write(coef, plan, script, [None, 5, None, None, 7, None, None, None, 1, None, None])
    if name == "dc_apart":
        coef, plan = baseline_coefficients(save(picture("noise", 40, 24, "RGB"), quality=90))
        script = [((0,), 0, 0, 0, 1), ((1,), 0, 0, 0, 1), ((2,), 0, 0, 0, 1)] + SCRIPT_COLOUR[1:6]
        script += [((0,), 0, 0, 1, 0), ((1,), 0, 0, 1, 0), ((2,), 0, 0, 1, 0)] + SCRIPT_COLOUR[7:]
        restart = [2, None, None, 3, None, None, None, 3, 2, None, None, None, None, 4]
        return P.write(coef, plan, script, restart)
    if name == "exif6":
        coef, plan = baseline_coefficients(save(picture("gradient", 47, 33, "RGB"), quality=80))
        tiff = b"MM\x00\x2A\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01\x00\x06\x00\x00\x00\x00\x00\x00"
        return P.write(coef, plan, SCRIPT_COLOUR, head=P._segment(0xE1, b"Exif\x00\x00" + tiff))
    raise KeyError(name)


WRITTEN = ["spectral", "approx3", "dc_apart", "exif6"]


@functools.lru_cache(maxsize=None)
def flat_eob_file():
    """Flat grey 2048 x 1024: 32,768 blocks without an AC coefficient, so every AC scan is end-of-band runs at the format's cap of 32,767"""
    return save(picture("flat", 2048, 1024, "L"), quality=75, progressive=True)


def c_prog_plan(lib, data):
    from bb_ocr_amd import _lib

    p = _lib.bbocr_jpeg_progressive_plan()
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    assert lib.bbocr_host_jpeg_progressive_plan(buf, len(data), C.byref(p)) == 0
    return p


def assert_plan_equal(cp, plan, name=""):
    """The C plan field by field against the restatement's, the script included"""
    assert (cp.supported, cp.reason) == (int(plan["supported"]), plan["reason"]), name
    assert cp.n_scans == len(plan["scans"]), name
    if cp.n_scans:
        nc = plan["components"]
        assert (cp.width, cp.height, cp.components, cp.mcu_cols, cp.mcu_rows, cp.chroma) == (
            plan["width"], plan["height"], nc, plan["mcu_cols"], plan["mcu_rows"], plan["chroma"]), name
        assert [tuple(cp.sampling[i]) for i in range(min(nc, 3))] == [tuple(s) for s in plan["sampling"]], name
    for k, s in enumerate(plan["scans"]):
        c = cp.scans[k]
        ns = len(s["comps"])
        assert (c.components, list(c.component)[:ns], list(c.dc_table)[:ns], list(c.ac_table)[:ns]) == (ns, s["comps"], s["dc_table"], s["ac_table"]), (name, k)
        assert (c.ss, c.se, c.ah, c.al, c.restart_interval, c.segments, c.offset, c.bytes) == (
            s["ss"], s["se"], s["ah"], s["al"], s["restart_interval"], len(s["segments"]), s["offset"], s["bytes"]), (name, k)


def script_of(plan):
    return [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in plan["scans"]]


@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_pillow_and_the_c_plan_on_the_matrix(lib, size):
    files = matrix(size)
    assert len(files) == 180
    for name, mode, data in files:
        plan = P.parse(data)
        cp = c_prog_plan(lib, data)
        assert plan["supported"] and cp.supported == 1, name                 # a plan that refuses everything cannot pass
        assert_plan_equal(cp, plan, name)
        assert (plan["width"], plan["height"]) == size, name
        assert script_of(plan) == (SCRIPT_GREY if mode == "L" else SCRIPT_COLOUR), name
        want = pillow_pixels(data)
        assert want.shape == ((size[1], size[0]) if mode == "L" else (size[1], size[0], 3)), name
        assert np.array_equal(P.decode_pixels(data, plan), want), name
        old = c_plan(lib, data)                                              # the existing plan keeps refusing the file
        assert (old.supported, old.reason, old.chroma) == (0, P.SOF, 0), name


def test_matrix_holds_restart_segments_short_last_segments_and_the_block_raster_trap():
    plans = [(mode, P.parse(d)) for size in SIZES for _, mode, d in matrix(size)]
    assert {p["chroma"] for _, p in plans} == {0, K.C444, K.C422, K.C440}
    assert sum(any(s["restart_interval"] for s in p["scans"]) for _, p in plans) == 600
    assert any(P.scan_units(p, s) % s["restart_interval"] for _, p in plans for s in p["scans"] if s["restart_interval"])   # a short last segment
    narrower = [p for m, p in plans if m == "420" and P.comp_raster(p, 0)[0] < 2 * p["mcu_cols"]]
    assert narrower and any(P.comp_raster(p, 0)[1] < 2 * p["mcu_rows"] for m, p in plans if m == "420")


def test_end_of_band_run_at_the_cap():
    data = flat_eob_file()
    plan = P.parse(data)
    assert plan["supported"] and P.n_blocks(plan) == 32768
    stats = {}
    coef = P.decode_coefficients(data, plan, stats=stats)
    assert stats["eobrun"] >= 16384
    assert not coef[:, 1:].any()
    assert np.array_equal(K.planes_to_pixels(K.component_planes(coef, plan), plan), pillow_pixels(data))


@pytest.mark.parametrize("name", WRITTEN)
def test_scripts_pillow_never_writes(lib, name):
    data = written(name)
    plan = P.parse(data)
    assert plan["supported"], plan["reason"]
    assert_plan_equal(c_prog_plan(lib, data), plan, name)
    assert np.array_equal(P.decode_pixels(data, plan), pillow_pixels(data))
    script = script_of(plan)
    if name == "spectral":
        assert all(ah == 0 and al == 0 for _, _, _, ah, al in script)
    if name == "approx3":
        assert [(ah, al) for _, ss, _, ah, al in script if ss == 0] == [(0, 3), (3, 2), (2, 1), (1, 0)]
        assert [(ah, al) for _, ss, _, ah, al in script if ss == 1] == [(0, 3), (3, 2), (2, 1), (1, 0)]
        assert {s["restart_interval"] for s in plan["scans"]} == {0, 1, 5, 7}            # a DRI between scans is in force from there on
    if name == "dc_apart":
        assert plan["width"] % 16 and [c for c, ss, _, ah, _ in script if ss == 0 and ah == 0] == [(0,), (1,), (2,)]
        assert P.comp_raster(plan, 0)[0] == 5 and 2 * plan["mcu_cols"] == 6
        assert len(plan["scans"][0]["segments"]) == -(-15 // 2)                           # the interval counts blocks, not MCUs
    if name == "exif6":
        assert c_prog_plan(lib, data).orientation == 6 == c_plan(lib, data).orientation


def test_orientation_follows_the_existing_plan(lib):
    for size in SIZES[:2]:
        for name, _, data in matrix(size)[:8]:
            assert c_prog_plan(lib, data).orientation == c_plan(lib, data).orientation == 1, name


def _sos_offsets(data, plan):
    """offset of the FF of every SOS marker"""
    return [s["offset"] - (2 + 2 + 1 + 2 * len(s["comps"]) + 3) for s in plan["scans"]]


def test_refusals(lib):
    from PIL import Image

    data = matrix((47, 33))[0][2]                                             # 4:2:0, no restart interval
    plan = P.parse(data)
    sos = _sos_offsets(data, plan)
    assert all(data[o:o + 2] == b"\xFF\xDA" for o in sos)
    cases = {}
    cases["last scan cut out"] = (data[:sos[-1]] + b"\xFF\xD9", P.SCRIPT)
    k = next(i for i, s in enumerate(plan["scans"]) if s["ah"] == 2)          # a refinement with the wrong Ah
    wrong = bytearray(data)
    wrong[plan["scans"][k]["offset"] - 1] = 0x10
    cases["wrong Ah"] = (bytes(wrong), P.SCRIPT)
    coef, frame = baseline_coefficients(save(picture("noise", 16, 16, "L"), quality=90))
    bands = [((0,), k, k, 0, 0) for k in range(1, 64)]
    ok64 = P.write(coef, frame, [((0,), 0, 0, 0, 0)] + bands)
    cases["65 scans"] = (P.write(coef, frame, [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0)] + bands), P.SCANS)
    dqt = P._segment(0xDB, bytes([0]) + bytes([9] * 64))
    cases["DQT behind the first SOS"] = (data[:sos[1]] + dqt + data[sos[1]:], P.MULTISCAN)
    cases["CMYK"] = (save(Image.fromarray(np.zeros((16, 16, 4), np.uint8) + 90, "CMYK"), progressive=True), P.COMPONENTS)
    cases["truncated before EOI"] = (data[:-2], P.NO_EOI)
    cases["baseline"] = (save(picture("noise", 47, 33, "RGB"), quality=90), P.SOF)          # it has bbocr_host_jpeg_plan
    cases["12 bit"] = (data.replace(b"\xFF\xC2\x00\x11\x08", b"\xFF\xC2\x00\x11\x0C"), P.PRECISION)
    cases["arithmetic"] = (data.replace(b"\xFF\xC2\x00\x11\x08", b"\xFF\xCA\x00\x11\x08"), P.SOF)
    cases["AC before DC"] = (P.write(coef, frame, [((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)]), P.SCRIPT)
    cases["not a JPEG"] = (b"\x89PNG\r\n\x1a\n" + bytes(32), P.NOT_JPEG)
    flat_dc = bytes([0x00]) + bytes(P.FLAT_DC[0]) + bytes(P.FLAT_DC[1])       # a table whose counts are no prefix code: three codes of one bit
    spectral = written("spectral")
    assert spectral.count(flat_dc) == 1
    cases["no prefix code"] = (spectral.replace(flat_dc, bytes([0x00, 3, 0, 0, 0, 13]) + flat_dc[6:]), P.TABLES)
    for name, (bad, reason) in cases.items():
        assert bad != data, name
        ref = P.parse(bad)
        assert (ref["supported"], ref["reason"]) == (False, reason), name
        assert_plan_equal(c_prog_plan(lib, bad), ref, name)
    full = P.parse(ok64)
    assert full["supported"] and len(full["scans"]) == 64                      # the cap itself is taken
    assert_plan_equal(c_prog_plan(lib, ok64), full, "64 scans")
    assert np.array_equal(P.decode_pixels(ok64, full), pillow_pixels(ok64))


def test_a_file_the_baseline_walk_leaves_before_its_frame_header_is_routed_by_its_own_plan(lib):
    """a DHT with table id 2 in front of SOF2: ``bbocr_host_jpeg_plan`` stops there (BBOCR_JPEG_TABLES), the progressive plan takes the file"""
    from bb_ocr_amd.reader import jpeg_page

    data = matrix((47, 33))[0][2]
    sof = data.index(b"\xFF\xC2")
    data = data[:sof] + P._segment(0xC4, bytes([0x02]) + bytes(P.FLAT_DC[0]) + bytes(P.FLAT_DC[1])) + data[sof:]
    assert c_plan(lib, data).reason == P.TABLES and c_prog_plan(lib, data).supported == 1
    assert_plan_equal(c_prog_plan(lib, data), P.parse(data))
    assert np.array_equal(P.decode_pixels(data), pillow_pixels(data))
    page = jpeg_page(data, chroma=True, progressive=True)
    assert page is not None and page.progressive and jpeg_page(data, chroma=True) is None


def test_existing_entry_points_keep_refusing(lib):
    from bb_ocr_amd import _lib
    from bb_ocr_amd.reader import jpeg_page

    data = matrix((47, 33))[0][2]
    assert C.sizeof(_lib.bbocr_jpeg_plan) == 96
    assert jpeg_page(data, chroma=True) is None and jpeg_page(data) is None
    page = jpeg_page(data, chroma=True, progressive=True)
    assert page is not None and page.shape == (33, 47, 3) and page.orientation == 1
    assert jpeg_page(matrix((47, 33))[-1][2][:-2], chroma=True, progressive=True) is None      # a file the new plan refuses


def test_routing_with_the_recording_reader(files):
    """``device_decode="progressive"`` sends the progressive file of test_read_files_cpu.py's directory to the device decoder as a ``"jpg"``
    page, in a group with the baseline files of its shape; ``True`` and ``"chroma"`` leave it to the host pool as ``"ycc"``"""
    paths, spec, want = files
    assert sum(kind == "prog" for kind, _ in spec) == 1
    fd = R.FakeDeviceReader()
    assert R.run(fd, paths, device_decode="progressive") == want
    groups = R.batches(spec, {**R.DEVICE_KIND, "prog": "jpg"})
    assert sorted(len(idx) for k, idx in groups if k == "jpg") == [1, 2, 4, 4, 4, 4]
    assert R.made(fd) == collections.Counter(c for k, idx in groups for c in R.uploaded_calls(k, len(idx)))
    for option in (True, "chroma"):
        fd = R.FakeDeviceReader()
        assert R.run(fd, paths, device_decode=option) == want
        groups = R.batches(spec, R.DEVICE_KIND)
        assert sorted(len(idx) for k, idx in groups if k == "jpg") == [1, 1, 4, 4, 4, 4]
        assert R.made(fd) == collections.Counter(c for k, idx in groups for c in R.uploaded_calls(k, len(idx)))
