"""The scaled decode of the chroma classes, without a GPU: the restatement of tests/jpeg_scaled_chroma_ref.py (n x n blocks for every
component, fancy upsampling at the reduced size, replication at 1/8) equals the installed Pillow's draft bit for bit on the issue's
864-case matrix and on restart-interval files; fancy upsampling at 1/8 -- the one tempting mistake -- does not;
``bbocr_host_jpeg_scaled_geometry`` equals the restatement's geometry; the library exports the entry points of the shared-pass decode."""
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_chroma_ref as K
import jpeg_scaled_chroma_ref as SC
from test_jpeg_decode_cpu import c_plan, lib, picture, save  # noqa: F401  (lib: a fixture)
from test_jpeg_scaled_cpu import SCALES, pillow_draft

SIZES = [(1, 1), (3, 2), (5, 4), (8, 9), (9, 3), (16, 16), (17, 15), (2, 37), (37, 2), (24, 40), (31, 17), (33, 50), (64, 48), (97, 333),
         (130, 257), (150, 200)]                                   # H x W
KINDS = ("noise", "gradient")
QUALITIES = (30, 75, 95)
CLASSES = (K.C444, K.C422, K.C440)
NEW_SYMBOLS = ("bbocr_jpeg_decode_scales", "bbocr_jpeg_counters", "bbocr_host_jpeg_scaled_geometry", "bbocr_op_jpeg_scaled_class_stage")


def class_file(cls, kind, h, w, **kw):
    """a baseline file of `h` x `w` pixels of the chroma class; a 4:4:0 file is the lossless transposition of the w x h 4:2:2 file"""
    if cls == K.C440:
        return K.make_440(save(picture(kind, h, w, "RGB"), subsampling=1, **kw))
    return save(picture(kind, w, h, "RGB"), subsampling={K.C444: 0, K.C422: 1}[cls], **kw)


@functools.lru_cache(maxsize=None)
def class_matrix(size):
    """[(name, class, file bytes)] of one size: {noise, gradient} x qualities x classes"""
    h, w = size
    return [("%dx%d-%s-q%d-c%d" % (h, w, kind, q, cls), cls, class_file(cls, kind, h, w, quality=q))
            for kind in KINDS for q in QUALITIES for cls in CLASSES]


def decoded(data):
    """(plan, coefficients): one entropy decode serves the three scales"""
    plan = K.parse(data)
    return plan, K.decode_coefficients(data, plan)[0]


def test_matrix_is_the_issues():
    assert len(SIZES) * len(KINDS) * len(QUALITIES) * len(CLASSES) * len(SCALES) == 864


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pillows_draft_on_the_matrix(size):
    files = class_matrix(size)
    assert len(files) == 18
    for name, cls, data in files:
        plan, coef = decoded(data)
        assert plan["chroma"] == cls and (plan["height"], plan["width"]) == size, name
        for s in SCALES:
            got = SC.planes_to_pixels(SC.scaled_planes(coef, plan, s), plan, s)
            want = pillow_draft(data, s)
            assert got.shape == want.shape and np.array_equal(got, want), (name, s)


def test_restatement_equals_pillows_draft_on_restart_interval_files():
    files = []
    for (h, w), kw in (((33, 50), dict(restart_marker_blocks=2)), ((64, 48), dict(restart_marker_rows=1)), ((17, 15), dict(restart_marker_blocks=2))):
        for cls in (K.C444, K.C422):                               # make_440 writes no restart interval
            files.append(("%dx%d-c%d" % (h, w, cls), class_file(cls, "noise", h, w, quality=90, **kw)))
    for name, data in files:
        plan = K.parse(data)
        assert plan["restart_interval"] > 0 and len(plan["segments"]) > 1, name
        for s in SCALES:
            assert np.array_equal(SC.scaled_pixels(data, s, plan), pillow_draft(data, s)), (name, s)


def test_fancy_upsampling_at_scale_8_differs_from_pillow():
    """the negative control: the matrix reaches the branch that tells replication from fancy upsampling at 1/8"""
    differ = total = 0
    for size in ((33, 50), (97, 333), (130, 257)):
        for name, cls, data in class_matrix(size):
            if cls == K.C444:
                continue
            plan, coef = decoded(data)
            wrong = SC.planes_to_pixels(SC.scaled_planes(coef, plan, 8), plan, 8, fancy_at_8=True)
            total += 1
            differ += not np.array_equal(wrong, pillow_draft(data, 8))
    assert total == 36 and differ >= 1


def test_files_inside_the_scaled_decodes_scope_are_the_existing_restatement():
    import jpeg_scaled_ref as S

    for mode in ("RGB", "L"):
        data = save(picture("noise", 50, 33, mode), quality=80)
        for s in SCALES:
            assert np.array_equal(SC.scaled_pixels(data, s), S.scaled_pixels(data, s))


def c_geometry(lib, plan_c, s):
    from bb_ocr_amd import _lib

    comps = (_lib.bbocr_jpeg_scaled_comp * 3)()
    rc = lib.bbocr_host_jpeg_scaled_geometry(C.byref(plan_c), s, comps)
    return rc, [(g.block, g.plane_rows, g.plane_cols, g.valid_rows, g.valid_cols, g.upsample) for g in comps]


def test_host_geometry_equals_the_restatement(lib):
    from bb_ocr_amd import _lib

    for size in SIZES:
        files = [(cls, d) for _, cls, d in class_matrix(size)[:3]]
        files += [(0, save(picture("gradient", size[1], size[0], "RGB"), quality=75)), (0, save(picture("gradient", size[1], size[0], "L"), quality=75))]
        for cls, data in files:
            plan = K.parse(data)
            pc = c_plan(lib, data)
            assert pc.chroma == cls
            for s in SCALES:
                rc, got = c_geometry(lib, pc, s)
                want = SC.geometry(plan, s)
                assert rc == 0 and got[:len(want)] == want and got[len(want):] == [(0,) * 6] * (3 - len(want)), (size, cls, s)
    # a 24-megapixel page, planned by hand: 4284 x 5712 in every sampling the decoder takes
    H, W = 4284, 5712
    for comps, (h, v), cls in ((3, (2, 2), 0), (3, (1, 1), K.C444), (3, (2, 1), K.C422), (3, (1, 2), K.C440), (1, (1, 1), 0)):
        plan = dict(height=H, width=W, components=comps, sampling=[(h, v), (1, 1), (1, 1)], mcu_cols=-(-W // (8 * h)), mcu_rows=-(-H // (8 * v)))
        pc = _lib.bbocr_jpeg_plan()
        pc.width, pc.height, pc.components, pc.mcu_cols, pc.mcu_rows = W, H, comps, plan["mcu_cols"], plan["mcu_rows"]
        pc.supported, pc.chroma = int(cls == 0), cls
        for i, (a, b) in enumerate(plan["sampling"]):
            pc.sampling[i][0], pc.sampling[i][1] = a, b
        for s in SCALES:
            rc, got = c_geometry(lib, pc, s)
            assert rc == 0 and got[:comps] == SC.geometry(plan, s), (comps, h, v, s)
    assert SC.geometry(dict(plan, components=3, sampling=[(2, 1)] + [(1, 1)] * 2, mcu_cols=357, mcu_rows=536), 8)[1] == (1, 536, 357, 536, 357, SC.UP_REPLICATE)
    # refused: scale 1 and 3, a plan the decoder does not take, null pointers
    pc = c_plan(lib, save(picture("gradient", 40, 24, "RGB"), quality=75, subsampling=1))
    assert c_geometry(lib, pc, 1)[0] != 0 and c_geometry(lib, pc, 3)[0] != 0
    assert c_geometry(lib, c_plan(lib, save(picture("gradient", 40, 24, "RGB"), quality=75, progressive=True)), 2)[0] != 0
    assert lib.bbocr_host_jpeg_scaled_geometry(None, 2, None) != 0


def test_the_new_entry_points_are_exported(lib):
    from bb_ocr_amd import _lib

    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "bbocr.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    from bb_ocr_amd import Reader

    assert callable(Reader.decode_jpeg_scales) and callable(Reader.jpeg_counters)
