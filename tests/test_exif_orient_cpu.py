"""EXIF orientation in the JPEG plan (csrc/jpegdec.cpp: bbocr_host_jpeg_plan, no GPU) against the installed Pillow, and the numpy
restatement of the eight orientations (tests/orient_ref.py) against ``ImageOps.exif_transpose``.  Needs the built library."""
import ctypes as C
import io

import numpy as np
import pytest

import orient_ref as R
from test_jpeg_decode_cpu import PHOTOS, picture, save

PLAN_FIELDS = ("width", "height", "components", "restart_interval", "mcu_cols", "mcu_rows", "segments", "scan_bytes", "supported", "reason")


@pytest.fixture(scope="module")
def photo():
    """IMG_9685.JPG without the APP segments it came with: JFIF is put back so that it stays a YCbCr file"""
    from PIL import Image

    data = R.bare(open(PHOTOS[1], "rb").read())
    assert Image.open(io.BytesIO(data)).getexif().get(0x0112) is None
    return data


def plan(data):
    from bb_ocr_amd.reader import jpeg_plan

    return jpeg_plan(data)


def pillow_orientation(data):
    from PIL import Image

    return Image.open(io.BytesIO(data)).getexif().get(0x0112)


def same_plan(a, b, shift):
    """every field but the orientation; the scan starts `shift` bytes later"""
    for f in PLAN_FIELDS:
        assert getattr(a, f) == getattr(b, f), f
    assert [list(r) for r in a.sampling] == [list(r) for r in b.sampling]
    assert a.scan_offset == b.scan_offset + shift


def test_plan_struct_keeps_its_size_and_offsets():
    from bb_ocr_amd import _lib

    P = _lib.bbocr_jpeg_plan
    assert C.sizeof(P) == 96                                     # 3 + 6 + 4 ints, 2 long long, supported, reason, 4 ints
    assert P.supported.offset == 72 and P.reason.offset == 76 and P.orientation.offset == 80 and P.reserved.offset == 84
    assert P.scan_offset.offset == 56 and P.scan_bytes.offset == 64


@pytest.mark.parametrize("order", ["II", "MM"])
@pytest.mark.parametrize("behind_jfif", [True, False])
def test_orientation_equals_pillow(photo, order, behind_jfif):
    from PIL import Image

    base = plan(photo)
    assert base.supported and base.orientation == 1
    for o in range(1, 9):
        d = R.with_orientation(photo, o, order, behind_jfif)
        p = plan(d)
        assert pillow_orientation(d) == o
        assert p.orientation == o, (o, order, behind_jfif)
        same_plan(p, base, len(d) - len(photo))
        assert Image.open(io.BytesIO(d)).size == (base.width, base.height)      # still the file it was


def test_restatement_accepts_and_the_host_decodes_the_spliced_file(photo):
    import jpeg_entropy_ref as J
    from bb_ocr_amd.reader import decode_file_ycc

    d = R.with_orientation(photo, 6, "MM")
    assert J.parse(d)["width"] == plan(photo).width
    assert np.array_equal(decode_file_ycc(d), decode_file_ycc(photo))          # decode_file_ycc applies no orientation


MALFORMED = {
    "no tag": dict(with_tag=False),
    "tag only in IFD1": dict(where="ifd1"),
    "value 0": dict(value=0),
    "value 9": dict(value=9),
    "value 65535": dict(value=65535),
    "count 2": dict(count=2),
    "type ASCII": dict(typ=2),
    "IFD offset beyond the segment": dict(ifd_offset=4000),
    "IFD offset at the last byte": dict(ifd_offset=8 + 2 + 24 + 4 - 1),
    "entry count runs off the segment": dict(entry_count=40),
    "another tag": dict(tag=0x0113),
}


@pytest.mark.parametrize("order", ["II", "MM"])
@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_everything_else_is_orientation_1(photo, case, order):
    kw = dict(value=6)
    kw.update(MALFORMED[case])
    d = R.splice(photo, R.exif_segment(order=order, **kw))
    p = plan(d)
    assert p.orientation == 1, case
    same_plan(p, plan(photo), len(d) - len(photo))               # malformed EXIF changes nothing else


def test_pillow_reports_out_of_range_values_and_does_not_transpose(photo):
    from PIL import Image, ImageOps

    for v in (0, 9, 65535):
        d = R.with_orientation(photo, v)
        assert pillow_orientation(d) == v
        pil = Image.open(io.BytesIO(d))
        assert ImageOps.exif_transpose(pil).size == pil.size


def test_no_exif_truncated_exif_and_other_containers(photo):
    assert plan(photo).orientation == 1
    seg = R.exif_segment(6)
    for cut in (6, 8, 10, 13, 15, 17, 20, 29):                   # the segment ends inside the TIFF header, the IFD, the entry
        short = seg[:4 + cut]
        short = short[:2] + bytes([(len(short) - 2) >> 8, (len(short) - 2) & 255]) + short[4:]
        d = R.splice(photo, short)
        p = plan(d)
        assert p.orientation == 1, cut
        same_plan(p, plan(photo), len(d) - len(photo))
    d = R.splice(photo, b"\xFF\xE1\x00\x0Ahttp://a") + b""      # an APP1 that is not EXIF (XMP's place), then the real one
    d = R.splice(d, R.exif_segment(3))
    assert plan(d).orientation == 3
    two = R.splice(R.splice(photo, R.exif_segment(8)), R.exif_segment(6))       # the FIRST EXIF segment counts
    assert plan(two).orientation == 6
    png = io.BytesIO()
    picture("noise", 8, 8, "RGB").save(png, "PNG")
    p = plan(png.getvalue())
    assert not p.supported and p.orientation in (0, 1)


def test_long_typed_tag_is_honoured(photo):
    for order in ("II", "MM"):
        d = R.with_orientation(photo, 8, order, typ=4)
        assert pillow_orientation(d) == 8 and plan(d).orientation == 8


def test_refused_files_report_their_orientation():
    """a 4:4:4 file, a progressive one and a grey one: the host-YCbCr path of imread_bgr_device reads the plan's orientation"""
    from bb_ocr_amd.reader import JpegPage

    img = picture("gradient", 40, 24, "RGB")
    for kw, ok in ((dict(subsampling=0), False), (dict(progressive=True), False), (dict(), True)):
        d = R.with_orientation(save(img, quality=90, **kw), 5, "MM")
        p = plan(d)
        assert bool(p.supported) == ok and p.orientation == 5, kw
    d = R.with_orientation(save(picture("gradient", 40, 24, "L"), quality=90), 7)
    p = plan(d)
    assert p.supported and p.orientation == 7
    page = JpegPage(d, p)
    assert page.orientation == 7 and page.shape == (24, 40, 1)    # the shape stays the un-oriented decode's


@pytest.mark.parametrize("order", ["II", "MM"])
def test_restatement_equals_exif_transpose(photo, order):
    from PIL import Image, ImageOps

    small = save(Image.open(io.BytesIO(photo)).resize((37, 23)), quality=90)
    a = np.asarray(Image.open(io.BytesIO(small)).convert("RGB"))
    for o in range(1, 9):
        d = R.with_orientation(small, o, order)
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(d))).convert("RGB"))
        got = R.orient(a, o)
        assert got.shape == ((37, 23, 3) if o >= 5 else (23, 37, 3))
        assert np.array_equal(got, want), o
        assert np.array_equal(R.orient(a[..., 0], o), want[..., 0])


def test_imread_restatement_on_the_host(photo):
    """_imread_bgr (the host path the device one must equal) is orient() of the un-oriented RGB decode, channels reversed"""
    from PIL import Image

    from bb_ocr_amd.preprocess import _imread_bgr, exif_orientation

    rgb = np.asarray(Image.open(io.BytesIO(photo)).convert("RGB"))
    for o in (1, 3, 6, 8):
        d = R.with_orientation(photo, o)
        assert np.array_equal(_imread_bgr(io.BytesIO(d)), R.orient(rgb, o)[..., ::-1])
    assert [exif_orientation(v) for v in (None, 0, 1, 8, 9, 65535, "6")] == [1, 1, 1, 8, 1, 1, 1]
