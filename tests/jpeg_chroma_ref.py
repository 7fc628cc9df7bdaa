"""Restatement of the baseline JPEG decoder for the chroma layouts beside 4:2:0 -- 4:4:4 (luma sampled 1x1), 4:2:2 (2x1) and 4:4:0 (1x2),
both chroma components 1x1 -- on top of tests/jpeg_entropy_ref.py and tests/jpeg_ref.py, which stay the yardstick of everything inside
that scope and are imported, not edited.  The yardstick of ``bbocr_jpeg_plan::chroma`` and of what csrc/jpegdec.* decodes for such a file.

  * ``parse``       jpeg_entropy_ref's plan; for a file it refuses with SAMPLING that is of one of the three classes and passes every check
                    behind the sampling test, the full plan -- MCUs of 8 h x 8 v pixels -- with ``chroma`` = 1 / 2 / 3, ``supported`` False
                    and ``reason`` SAMPLING; every other refused file: ``chroma`` 0;
  * ``Stream``      the entropy-coded segments with h * v luma blocks, then Cb and Cr, per MCU;
  * ``decode_coefficients`` / ``component_planes`` / ``decode_pixels``  as in jpeg_entropy_ref, for any of the plans above;
  * ``upsample_h2v1`` / ``upsample_h1v2``  jdsample.c's h2v1_fancy_upsample (h2v1_upsample when the plane is at most 2 wide) and
                    h1v2_fancy_upsample;
  * ``make_440``    a 4:4:0 file, which Pillow cannot write: the lossless transposition of a 4:2:2 file.
"""
from __future__ import annotations

import struct

import numpy as np

import jpeg_encode_ref as E
import jpeg_entropy_ref as J
import jpeg_ref

C444, C422, C440 = 1, 2, 3                                        # bbocr_jpeg_plan::chroma (include/bbocr.h)
LUMA = {C444: (1, 1), C422: (2, 1), C440: (1, 2)}                 # (h, v) of component 0


# ------------------------------------------------------------------------------------------------ the plan
def _sof0(data: bytes):
    """Offset of the first SOF0 segment's body (the precision byte), found as jpeg_entropy_ref walks the headers; None: none before SOS"""
    p, n = 2, len(data)
    while p + 4 <= n and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            p += 2
            continue
        if m == 0xC0:
            return p + 4
        if m in (0xDA, 0xD9):
            return None
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    return None


def parse(data: bytes) -> dict:
    """The plan of a file.  Inside jpeg_entropy_ref's scope: its plan and ``chroma`` 0.  Of a chroma class: see the module text.  The checks
    behind the sampling test are jpeg_entropy_ref's own: they run on the same bytes with the frame header rewritten as the 4:2:0 file of
    the same MCU grid (sampling 2x2, 1x1, 1x1 and 2 / h, 2 / v times the size), which moves no byte and changes no other check."""
    data = bytes(data)
    plan = J.parse(data)
    plan["chroma"] = 0
    if plan["supported"] or plan["reason"] != J.SAMPLING:
        return plan
    s = _sof0(data)
    H, W = (data[s + 1] << 8) | data[s + 2], (data[s + 3] << 8) | data[s + 4]
    samp = [(data[s + 7 + 3 * i] >> 4, data[s + 7 + 3 * i] & 15) for i in range(3)]
    cls = next((c for c, hv in LUMA.items() if samp == [hv, (1, 1), (1, 1)]), 0)
    if not cls:
        return plan
    h, v = LUMA[cls]
    if W * 2 // h > 65535 or H * 2 // v > 65535:
        raise NotImplementedError("the rewritten frame header holds at most 65535 pixels a side")
    as420 = bytearray(data)
    as420[s + 1:s + 5] = struct.pack(">HH", H * 2 // v, W * 2 // h)
    as420[s + 7] = 0x22
    full = J.parse(bytes(as420))
    if not full["supported"]:
        return plan                                              # fails a later check: refused as before, nothing more reported
    assert (full["mcu_cols"], full["mcu_rows"]) == (-(-W // (8 * h)), -(-H // (8 * v)))
    full.update(width=W, height=H, sampling=samp, supported=False, reason=J.SAMPLING, chroma=cls)
    return full


def luma(plan):
    """(h, v): luma blocks of an MCU across and down"""
    return tuple(plan["sampling"][0]) if plan["components"] == 3 else (1, 1)


# ------------------------------------------------------------------------------------------------ entropy decoding
class Stream(J.Stream):
    """jpeg_entropy_ref.Stream with the MCU of the plan's sampling: h * v luma blocks, row after row, then Cb, then Cr"""

    def __init__(self, data: bytes, plan: dict):
        super().__init__(data, plan)
        if plan["components"] == 3:
            h, v = luma(plan)
            self.bpm = h * v + 2
            self.comp = [0] * (h * v) + [1, 2]


def decode_coefficients(data: bytes, plan: dict, S: int = 1024):
    """jpeg_entropy_ref.decode_coefficients on ``Stream``: (coef int32 [blocks][64] natural order, DC absolute; entry states int64
    [subsequences][4] = (bit in the unstuffed stream, block in MCU, zig-zag position, first output block))"""
    st = Stream(data, plan)
    coef = np.zeros((st.nmcu * st.bpm, 64), np.int32)
    entries = []
    blk0 = 0
    for s in range(len(st.seg_byte) - 1):
        nbits = (st.seg_byte[s + 1] - st.seg_byte[s]) * 8
        want = st.seg_blocks(s)
        state, done = (0, 0, 0), 0
        for a in range(0, max(nbits, 1), S):
            entries.append((st.seg_byte[s] * 8 + state[0], state[1], state[2], blk0 + done))
            state, n, ok = J._run(st, s, state, min(a + S, nbits), want - done, coef, blk0 + done)
            done += n
        if done != want:
            raise ValueError("segment %d holds %d blocks, expected %d" % (s, done, want))
        blk0 += want
    J._dc_sums(coef, st)
    return coef, np.array(entries, np.int64)


# ------------------------------------------------------------------------------------------------ coefficients -> samples
def _idct(blocks, q):
    """[by, bx, 8, 8] quantised blocks -> the sample plane [by * 8, bx * 8] (dequantise, ISLOW IDCT, range limit)"""
    d = blocks * np.array(q, np.int64).reshape(8, 8)
    r = jpeg_ref._idct_1d(d, 2, True)
    r = jpeg_ref.range_limit(jpeg_ref._idct_1d(r, 3, False))
    return r.transpose(0, 2, 1, 3).reshape(r.shape[0] * 8, r.shape[1] * 8)


def padded_planes(coef: np.ndarray, plan: dict):
    """The component planes in whole MCUs: Y [mcu_rows * 8 v, mcu_cols * 8 h], Cb and Cr [mcu_rows * 8, mcu_cols * 8] (one component: Y)"""
    mx, my = plan["mcu_cols"], plan["mcu_rows"]
    if plan["components"] == 1:
        return [_idct(coef.astype(np.int64).reshape(my, mx, 8, 8), plan["quant"][0])]
    h, v = luma(plan)
    c = coef.astype(np.int64).reshape(my, mx, h * v + 2, 8, 8)
    y = c[:, :, :h * v].reshape(my, mx, v, h, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * v, mx * h, 8, 8)
    return [_idct(y, plan["quant"][0]), _idct(c[:, :, h * v], plan["quant"][1]), _idct(c[:, :, h * v + 1], plan["quant"][2])]


def component_planes(coef: np.ndarray, plan: dict):
    """... cropped to each component's size: Y [H, W], Cb and Cr [ceil(H / v), ceil(W / h)]"""
    H, W = plan["height"], plan["width"]
    planes = padded_planes(coef, plan)
    if plan["components"] == 1:
        return [planes[0][:H, :W]]
    h, v = luma(plan)
    ch, cw = -(-H // v), -(-W // h)
    return [planes[0][:H, :W], planes[1][:ch, :cw], planes[2][:ch, :cw]]


def upsample_h2v1(c: np.ndarray, W: int) -> np.ndarray:
    """jdsample.c h2v1_fancy_upsample of a plane [H, ceil(W / 2)], cropped to W columns; h2v1_upsample when it is at most 2 wide"""
    c = c.astype(np.int64)
    if c.shape[1] <= 2:
        return np.repeat(c, 2, 1)[:, :W]
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)               # the end samples' missing neighbours are themselves: they come out copied
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :W]


def upsample_h1v2(c: np.ndarray, H: int) -> np.ndarray:
    """jdsample.c h1v2_fancy_upsample of a plane [ceil(H / 2), W], cropped to H rows (the rows above the first and below the last are
    those rows again); whatever the width"""
    c = c.astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]])
    dn = np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    out[0::2] = (3 * c + up + 1) >> 2
    out[1::2] = (3 * c + dn + 2) >> 2
    return out[:H]


def planes_to_pixels(planes, plan):
    H, W = plan["height"], plan["width"]
    if plan["components"] == 1 or luma(plan) == (2, 2):
        return J.planes_to_pixels(planes, plan)
    up = {(1, 1): lambda c: c, (2, 1): lambda c: upsample_h2v1(c, W), (1, 2): lambda c: upsample_h1v2(c, H)}[luma(plan)]
    return np.stack([planes[0], up(planes[1]), up(planes[2])], axis=2).astype(np.uint8)


def decode_pixels(data: bytes, plan: dict = None) -> np.ndarray:
    """uint8 [H,W,3] YCbCr triples (colour files) or [H,W] samples (grey files): what libjpeg hands Pillow"""
    plan = plan or parse(data)
    coef, _ = decode_coefficients(data, plan)
    return planes_to_pixels(component_planes(coef, plan), plan)


# ------------------------------------------------------------------------------------------------ a 4:4:0 file
def _symbols(zz, comp):
    """jpeg_encode_ref._symbols for blocks of any MCU layout: ``comp[b]`` is block b's component (typical tables: 0 for luma, 1 for chroma)"""
    last = [0, 0, 0]
    blocks = []
    for b in range(zz.shape[0]):
        tab = 0 if comp[b] == 0 else 1
        v = [int(x) for x in zz[b]]
        diff = v[0] - last[comp[b]]
        last[comp[b]] = v[0]
        n = E._nbits(diff)
        out = [E.CODES["dc"][tab][n]]
        if n:
            out.append(((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
        r = 0
        for k in range(1, 64):
            if v[k] == 0:
                r += 1
                continue
            while r > 15:
                out.append(E.CODES["ac"][tab][0xF0])
                r -= 16
            n = E._nbits(v[k])
            out.append(E.CODES["ac"][tab][(r << 4) + n])
            out.append(((v[k] if v[k] >= 0 else v[k] - 1) & ((1 << n) - 1), n))
            r = 0
        if r:
            out.append(E.CODES["ac"][tab][0x00])
        blocks.append(out)
    return blocks


def _pack(blocks) -> bytes:
    """jpeg_encode_ref.pack of ``_symbols``' output"""
    acc = n = 0
    out = bytearray()
    for blk in blocks:
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


def make_440(data_422: bytes) -> bytes:
    """The 4:4:0 file a lossless transposition of the 4:2:2 file ``data_422`` yields: its coefficients with the MCU grid and every 8x8
    block transposed (an MCU's two luma blocks, side by side before, are now one above the other: the same order), the quantisation
    tables transposed, coded again with the typical Huffman tables and no restart interval, behind a JFIF header of sampling 1x2, 1x1,
    1x1 and swapped width and height."""
    plan = parse(data_422)
    assert plan["chroma"] == C422
    coef, _ = decode_coefficients(data_422, plan)
    my, mx = plan["mcu_rows"], plan["mcu_cols"]
    t = coef.reshape(my, mx, 4, 8, 8).transpose(1, 0, 2, 4, 3).reshape(-1, 64)
    scan = E.stuff(_pack(_symbols(t[:, J.ZIGZAG], [0, 0, 1, 2] * (mx * my))))
    out = b"\xFF\xD8" + E._segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k in range(3):
        q = np.array(plan["quant"][k]).reshape(8, 8).T.ravel()
        out += E._segment(0xDB, bytes([k]) + bytes(int(q[z]) for z in J.ZIGZAG))
    out += E._segment(0xC0, struct.pack(">BHHB", 8, plan["width"], plan["height"], 3) + bytes([1, 0x12, 0, 2, 0x11, 1, 3, 0x11, 2]))
    for cls_id, spec in ((0x00, E.DC_LUM), (0x10, E.AC_LUM), (0x01, E.DC_CHROM), (0x11, E.AC_CHROM)):
        out += E._segment(0xC4, bytes([cls_id]) + bytes(spec[0]) + bytes(spec[1]))
    out += E._segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11]) + b"\x00\x3F\x00")
    return out + scan + b"\xFF\xD9"
