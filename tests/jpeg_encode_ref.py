"""Restatement of a baseline JPEG encoder as Pillow 12 / libjpeg-turbo run it for ``Image.save(buf, "JPEG", quality=q)`` of an RGB or
"L" image, in numpy and plain Python: the yardstick of csrc/jpegenc.* (test_jpeg_encode_cpu.py pins it to the installed Pillow byte for
byte; test_gpu_jpeg_encode.py holds the device stages against it).

  * ``coefficients``  stage 0: per MCU colour conversion, edge replication, h2v2 downsampling, ISLOW FDCT and quantisation (the steps of
                      tests/jpeg_ref.py), kept as int16 [blocks][64] in zig-zag order, blocks in MCU order (Y00 Y01 Y10 Y11 Cb Cr; one
                      component: the blocks in raster order).  Y blocks wholly beyond ceil(W/8) x ceil(H/8) are libjpeg's DUMMY blocks
                      (jccoefct.c): AC terms zero, DC that of the block before them in MCU order;
  * ``block_bits``    stage 1: the bit length of every block (jchuff.c::encode_one_block: DC difference against the previous block of
                      the component, run/size symbols, ZRL for runs of 16 and more, EOB unless position 63 is non-zero) and their
                      exclusive prefix sum, the total last;
  * ``pack``          stage 2: the bits MSB first, the last byte padded with 1-bits;
  * ``stuff``         a zero byte behind every 0xFF;
  * ``header``        SOI, APP0 JFIF 1.01, [COM], DQT per table, SOF0, DHT per table, SOS -- what Pillow writes in front of the scan.
``encode`` is the whole file.
"""
from __future__ import annotations

import struct

import numpy as np

import jpeg_ref
from jpeg_entropy_ref import ZIGZAG

# ITU T.81 Annex K.3: (BITS, HUFFVAL) of the typical Huffman tables
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROM = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROM = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


def _codes(spec):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table (Annex C)"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = {"dc": [_codes(DC_LUM), _codes(DC_CHROM)], "ac": [_codes(AC_LUM), _codes(AC_CHROM)]}


# ----------------------------------------------------------------------------------------------------------------- stage 0
def _fdct_quant(plane, qt):
    """[by, bx, 64] quantised coefficients in zig-zag order of a sample plane whose sides are multiples of 8"""
    h, w = plane.shape
    b = (plane.astype(np.int64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    d = jpeg_ref._fdct_1d(jpeg_ref._fdct_1d(b, 3, True), 2, False)
    qv = qt * 8
    coef = np.sign(d) * ((np.abs(d) + qv // 2) // qv)
    return coef.reshape(h // 8, w // 8, 64)[:, :, ZIGZAG]


def coefficients(img: np.ndarray, quality: int) -> np.ndarray:
    """int16 [blocks][64]: ``img`` uint8 [H,W,3] RGB (three components, 4:2:0) or [H,W] (one component)"""
    H, W = img.shape[:2]
    ql, qc = jpeg_ref.qtables(quality)
    bh, bw = -(-H // 8), -(-W // 8)
    if img.ndim == 2:
        y = _fdct_quant(jpeg_ref._pad_edge(img.astype(np.int64), bh * 8, bw * 8), ql)
        return y.reshape(-1, 64).astype(np.int16)
    my, mx = -(-H // 16), -(-W // 16)
    y, cb, cr = jpeg_ref.rgb_to_ycc(img)
    yq = np.zeros((my * 2, mx * 2, 64), np.int64)
    yq[:bh, :bw] = _fdct_quant(jpeg_ref._pad_edge(y, bh * 8, bw * 8), ql)
    ch = -(-H // 2)
    chroma = []
    for c in (cb, cr):
        full = jpeg_ref._pad_edge(c, 2 * ch, 16 * mx)        # expand_right_edge of the input rows, the odd last row replicated
        s = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
        ds = (s + np.tile(np.array([1, 2], np.int64), 4 * mx)[None, :]) >> 2
        chroma.append(_fdct_quant(jpeg_ref._pad_edge(ds, my * 8, mx * 8), qc))   # expand_bottom_edge of the downsampled plane
    out = np.zeros((my, mx, 6, 64), np.int64)
    for j in range(my):
        for i in range(mx):
            for k in range(4):
                by, bx = 2 * j + (k >> 1), 2 * i + (k & 1)
                if by < bh and bx < bw:
                    out[j, i, k] = yq[by, bx]
                else:
                    out[j, i, k, 0] = out[j, i, k - 1, 0]       # a dummy block: the DC before it, no AC (Y00 is never one)
            out[j, i, 4], out[j, i, 5] = chroma[0][j, i], chroma[1][j, i]
    return out.reshape(-1, 64).astype(np.int16)


def dummy_blocks(H: int, W: int) -> np.ndarray:
    """bool [blocks] of a three-component page: True where the block is a dummy Y block"""
    bh, bw = -(-H // 8), -(-W // 8)
    my, mx = -(-H // 16), -(-W // 16)
    out = np.zeros((my, mx, 6), bool)
    for j in range(my):
        for i in range(mx):
            for k in range(4):
                out[j, i, k] = not (2 * j + (k >> 1) < bh and 2 * i + (k & 1) < bw)
    return out.reshape(-1)


# ----------------------------------------------------------------------------------------------------------------- stages 1, 2
def _nbits(v: int) -> int:
    return abs(v).bit_length()


def _symbols(coef, components):
    """per block the list of (code, length) pairs jchuff.c emits"""
    last = [0, 0, 0]
    blocks = []
    for b in range(coef.shape[0]):
        comp = 0 if components == 1 else (0, 0, 0, 0, 1, 2)[b % 6]
        tab = 0 if comp == 0 else 1
        zz = [int(v) for v in coef[b]]
        out = []
        diff = zz[0] - last[comp]
        last[comp] = zz[0]
        n = _nbits(diff)
        out.append(CODES["dc"][tab][n])
        if n:
            out.append(((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
        r = 0
        for k in range(1, 64):
            v = zz[k]
            if v == 0:
                r += 1
                continue
            while r > 15:
                out.append(CODES["ac"][tab][0xF0])
                r -= 16
            n = _nbits(v)
            out.append(CODES["ac"][tab][(r << 4) + n])
            out.append(((v if v >= 0 else v - 1) & ((1 << n) - 1), n))
            r = 0
        if r:
            out.append(CODES["ac"][tab][0x00])
        blocks.append(out)
    return blocks


def block_bits(coef: np.ndarray, components: int) -> np.ndarray:
    """int64 [blocks + 1]: the bit offset of every block in the unstuffed scan, then the total"""
    sizes = [sum(n for _, n in blk) for blk in _symbols(coef, components)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def pack(coef: np.ndarray, components: int) -> bytes:
    """the unstuffed scan: every block's bits MSB first, the last byte filled with 1-bits"""
    out = bytearray()
    acc = n = 0
    for blk in _symbols(coef, components):
        for code, length in blk:
            acc = (acc << length) | code
            n += length
            while n >= 8:
                out.append((acc >> (n - 8)) & 0xFF)
                n -= 8
            acc &= (1 << n) - 1
    if n:
        out.append(((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 0xFF)
    return bytes(out)


def stuff(scan: bytes) -> bytes:
    return scan.replace(b"\xFF", b"\xFF\x00")


# ----------------------------------------------------------------------------------------------------------------- the file
def _segment(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def header(H: int, W: int, components: int, quality: int, comment: bytes = None) -> bytes:
    ql, qc = jpeg_ref.qtables(quality)
    out = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if comment:
        out += _segment(0xFE, bytes(comment))
    for k, q in enumerate((ql, qc)[:1 if components == 1 else 2]):
        out += _segment(0xDB, bytes([k]) + bytes(int(q.ravel()[z]) for z in ZIGZAG))
    comps = [(1, 0x22 if components == 3 else 0x11, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if components == 3 else [])
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, components) + b"".join(bytes(c) for c in comps))
    for cls_id, spec in ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHROM), (0x11, AC_CHROM))[:2 if components == 1 else 4]:
        out += _segment(0xC4, bytes([cls_id]) + bytes(spec[0]) + bytes(spec[1]))
    sel = [(1, 0x00)] + ([(2, 0x11), (3, 0x11)] if components == 3 else [])
    return out + _segment(0xDA, bytes([components]) + b"".join(bytes(s) for s in sel) + b"\x00\x3F\x00")


def encode(img: np.ndarray, quality: int, comment: bytes = None) -> bytes:
    """``Image.fromarray(img).save(buf, "JPEG", quality=quality)`` (``comment``: the image's ``info["comment"]``)"""
    components = 1 if img.ndim == 2 else 3
    coef = coefficients(img, quality)
    return header(img.shape[0], img.shape[1], components, quality, comment) + stuff(pack(coef, components)) + b"\xFF\xD9"


def split_file(data: bytes):
    """(header up to and including SOS, stuffed scan, trailer) of a single-scan JPEG file"""
    p = 2
    while True:
        assert data[p] == 0xFF
        L = struct.unpack(">H", data[p + 2:p + 4])[0]
        m = data[p + 1]
        p += 2 + L
        if m == 0xDA:
            break
    return data[:p], data[p:-2], data[-2:]
