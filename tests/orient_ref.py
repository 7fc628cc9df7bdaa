"""Restatement of the EXIF orientation step of ``cv2.imread`` (``PIL.ImageOps.exif_transpose`` = OpenCV's ``ExifTransform``) in numpy
slices, and a builder of EXIF APP1 segments, well-formed and malformed, that splices one into a JPEG file's bytes.  Test infrastructure:
test_exif_orient_cpu.py pins ``orient`` against the installed Pillow; test_gpu_orient.py holds the device kernel against it."""
import struct

import numpy as np


def orient(a, o):
    """``a`` [H,W] or [H,W,C] in EXIF orientation ``o`` (1 .. 8): [H,W,...] for 1-4, [W,H,...] for 5-8"""
    t = np.swapaxes(a, 0, 1)
    return np.ascontiguousarray({1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: t, 6: t[:, ::-1], 7: t[::-1, ::-1], 8: t[::-1]}[o])


def exif_segment(value=6, order="II", typ=3, count=1, tag=0x0112, where="ifd0", ifd_offset=None, entry_count=None, with_tag=True):
    """One APP1 segment (marker and length included).  ``order``: "II" / "MM"; ``typ``: 3 SHORT, 4 LONG, 2 ASCII; ``where``: "ifd0", or
    "ifd1" (IFD0 then holds only an XResolution-free Make entry and links to an IFD1 with the tag); ``ifd_offset``: written instead of
    the true IFD0 offset; ``entry_count``: written instead of IFD0's true entry count; ``with_tag=False``: IFD0 without tag 0x0112."""
    e = "<" if order == "II" else ">"

    def entry(tg, ty, cnt, val):
        if ty == 3:
            body = struct.pack(e + "HH", val & 0xFFFF, 0)
        elif ty == 4:
            body = struct.pack(e + "I", val)
        else:
            body = bytes([0x30 + val % 10, 0, 0, 0])
        return struct.pack(e + "HHI", tg, ty, cnt) + body

    make = entry(0x010F, 2, 2, 7)                                  # Make = "7\0", inline
    ori = entry(tag, typ, count, value)
    if where == "ifd1":
        ifd0 = [make]
        ifd1 = [ori]
    else:
        ifd0 = [ori, make] if with_tag else [make]
        ifd1 = []
    off0 = 8
    off1 = off0 + 2 + 12 * len(ifd0) + 4 if ifd1 else 0
    tiff = (b"II*\0" if order == "II" else b"MM\0*") + struct.pack(e + "I", off0 if ifd_offset is None else ifd_offset)
    tiff += struct.pack(e + "H", len(ifd0) if entry_count is None else entry_count) + b"".join(ifd0) + struct.pack(e + "I", off1)
    if ifd1:
        tiff += struct.pack(e + "H", len(ifd1)) + b"".join(ifd1) + struct.pack(e + "I", 0)
    body = b"Exif\0\0" + tiff
    return b"\xFF\xE1" + struct.pack(">H", len(body) + 2) + body


def strip_app(data, drop=(0xE0, 0xE1, 0xE2)):
    """The JPEG file without its leading APP0 / APP1 / APP2 segments (JFIF, EXIF, MPF ...)"""
    assert data[:2] == b"\xFF\xD8"
    p, keep = 2, []
    while data[p] == 0xFF and data[p + 1] != 0xDA:
        L = struct.unpack(">H", data[p + 2:p + 4])[0]
        if data[p + 1] not in drop:
            keep.append(data[p:p + 2 + L])
        p += 2 + L
    return data[:2] + b"".join(keep) + data[p:]


def bare(data):
    """A photograph's file without the APP0 / APP1 / APP2 segments it came with (EXIF, XMP, MPF), behind a fresh JFIF segment: it stays a
    YCbCr file and carries no orientation of its own"""
    data = strip_app(data)
    return data[:2] + b"\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00" + data[2:]


def splice(data, segment, behind_jfif=True):
    """``segment`` behind SOI and the APP0 segments that follow it (``behind_jfif=False``: those APP0 segments are dropped and an Adobe
    APP14 with transform 1 keeps a 3-component file YCbCr: an EXIF-only file as cameras write it)"""
    assert data[:2] == b"\xFF\xD8"
    p = 2
    while data[p] == 0xFF and data[p + 1] == 0xE0:
        p += 2 + struct.unpack(">H", data[p + 2:p + 4])[0]
    if behind_jfif:
        return data[:p] + segment + data[p:]
    adobe = b"\xFF\xEE" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 1)
    return data[:2] + segment + adobe + data[p:]


def with_orientation(data, value, order="II", behind_jfif=True, **kw):
    """``data`` (a JPEG file without EXIF) carrying EXIF orientation ``value``"""
    return splice(data, exif_segment(value, order, **kw), behind_jfif)
