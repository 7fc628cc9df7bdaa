"""CPU restatement of the decode at scale 1/2, 1/4 and 1/8 (Pillow's ``draft``, ``decoderconfig == (s, 0)``) of the files of a chroma class --
4:4:4, 4:2:2 and 4:4:0 -- in numpy, on top of tests/jpeg_chroma_ref.py (plan, entropy decoding, the two fancy upsamplers) and
tests/jpeg_scaled_ref.py (the reduced IDCTs), which are imported, not edited.  The yardstick of ``bbocr_host_jpeg_scaled_geometry``, of
``bbocr_op_jpeg_scaled_class_stage`` and of what ``bbocr_jpeg_decode_scales`` writes for such a file.

With n = 8 / s, OH = ceil(H / s), OW = ceil(W / s) and luma sampling (h, v):

- every component's blocks go through the n x n reduced IDCT.  jdmaster.c doubles a component's ``DCT_scaled_size`` only when both
  directions allow it; for 4:2:2 and 4:4:0 one does not, so -- unlike 4:2:0 -- the chroma blocks stay n x n and the chroma keeps the file's
  sampling: Y ``[mcu_rows n v][mcu_cols n h]``, Cb and Cr ``[mcu_rows n][mcu_cols n]``;
- the valid chroma extent is ceil(OH / v) rows of ceil(OW / h) samples (libjpeg's ``downsampled_height`` / ``downsampled_width``);
- at s = 2 and 4 the chroma is upsampled at the reduced size by ``h2v1_fancy_upsample`` (4:2:2; ``h2v1_upsample`` when the plane is at most
  2 samples wide) or ``h1v2_fancy_upsample`` (4:4:0);
- at s = 8 it is replicated, ``out[y][x] = c[y // v][x // h]``: jdsample.c turns fancy upsampling off when ``min_DCT_scaled_size`` is 1;
- 4:4:4: the three planes have the output's size, nothing is upsampled.
"""
from __future__ import annotations

import numpy as np

import jpeg_chroma_ref as K
import jpeg_scaled_ref as S

UP_NONE, UP_H2V1_FANCY, UP_H1V2_FANCY, UP_H2V2_NOT_NEEDED, UP_REPLICATE = range(5)      # bbocr.h BBOCR_JPEG_UP_*


def geometry(plan: dict, s: int):
    """Per component ``(block, plane_rows, plane_cols, valid_rows, valid_cols, upsample)`` of the decode at 1 / s of any file the decoder
    takes: a grey file, a 4:2:0 file (jpeg_scaled_ref's geometry: chroma blocks of twice the edge) or a file of a chroma class"""
    n = 8 // s
    oh, ow = S.scaled_dims(plan["height"], plan["width"], s)
    my, mx = plan["mcu_rows"], plan["mcu_cols"]
    if plan["components"] == 1:
        return [(n, my * n, mx * n, oh, ow, UP_NONE)]
    h, v = K.luma(plan)
    if (h, v) == (2, 2):
        return [(n, my * 2 * n, mx * 2 * n, oh, ow, UP_NONE)] + [(2 * n, my * 2 * n, mx * 2 * n, oh, ow, UP_H2V2_NOT_NEEDED)] * 2
    up = UP_NONE if h * v == 1 else (UP_REPLICATE if s == 8 else (UP_H2V1_FANCY if h == 2 else UP_H1V2_FANCY))
    chroma = (n, my * n, mx * n, -(-oh // v), -(-ow // h), up)
    return [(n, my * n * v, mx * n * h, oh, ow, UP_NONE), chroma, chroma]


def scaled_planes(coef: np.ndarray, plan: dict, s: int):
    """The component planes of a chroma-class file's decode at 1 / s in whole MCUs (what the device keeps): [Y, Cb, Cr] int64"""
    n = 8 // s
    h, v = K.luma(plan)
    mx, my = plan["mcu_cols"], plan["mcu_rows"]
    c = coef.astype(np.int64).reshape(my, mx, h * v + 2, 8, 8)

    def idct(blocks, q):                                        # [by, bx, 8, 8] -> [by * n, bx * n]
        r = S.idct_reduced(blocks * np.array(q, np.int64).reshape(8, 8), n)
        return r.transpose(0, 2, 1, 3).reshape(r.shape[0] * n, r.shape[1] * n)

    y = c[:, :, :h * v].reshape(my, mx, v, h, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * v, mx * h, 8, 8)
    return [idct(y, plan["quant"][0]), idct(c[:, :, h * v], plan["quant"][1]), idct(c[:, :, h * v + 1], plan["quant"][2])]


def planes_to_pixels(planes, plan: dict, s: int, fancy_at_8: bool = False) -> np.ndarray:
    """uint8 [OH,OW,3].  ``fancy_at_8``: the WRONG rule -- fancy upsampling at s = 8 as well -- which the tests use as a negative control"""
    geo = geometry(plan, s)
    oh, ow = geo[0][3], geo[0][4]
    h, v = K.luma(plan)
    out = [planes[0][:oh, :ow]]
    for p, g in zip(planes[1:], geo[1:]):
        c, up = p[:g[3], :g[4]], g[5]
        if up == UP_REPLICATE and fancy_at_8:
            up = UP_H2V1_FANCY if h == 2 else UP_H1V2_FANCY
        if up == UP_H2V1_FANCY:
            c = K.upsample_h2v1(c, ow)
        elif up == UP_H1V2_FANCY:
            c = K.upsample_h1v2(c, oh)
        elif up == UP_REPLICATE:
            c = np.repeat(np.repeat(c, v, 0), h, 1)[:oh, :ow]
        out.append(c)
    return np.stack(out, axis=2).astype(np.uint8)


def scaled_pixels(data: bytes, s: int, plan: dict = None, fancy_at_8: bool = False) -> np.ndarray:
    """What ``draft`` with ``decoderconfig == (s, 0)`` decodes: YCbCr triples [OH,OW,3], or a grey file's samples [OH,OW].  Files inside
    jpeg_scaled_ref's scope (4:2:0, grey) are its own"""
    plan = plan or K.parse(data)
    if not plan["chroma"]:
        return S.scaled_pixels(data, s, plan)
    coef, _ = K.decode_coefficients(data, plan)
    return planes_to_pixels(scaled_planes(coef, plan, s), plan, s, fancy_at_8)
