"""CPU restatement of the trace previews' two device pieces (``enhanced_extractor.py:184-199``: ``Image.open(path)``,
``thumbnail((800, 800))``, ``save(format="PNG")``), in numpy, on the Pillow 12 / libjpeg-turbo semantics of each step.  The device path
(csrc/jpegdec.hip's scaled forms, ``bbocr_thumbnail_box``) is compared against it; the installed Pillow is compared against both.

- ``draft_scale``: ``JpegImageFile.draft``'s scale for a requested size: ``min(W // rw, H // rh)`` rounded down to 8 / 4 / 2 / 1.
- ``scaled_dims``: the decode's size at scale 1/s, ``ceil(W / s) x ceil(H / s)``.
- ``idct_reduced``: jidctred.c's 4x4, 2x2 and 1x1 inverse DCTs (CONST_BITS 13, PASS1_BITS 2) and jidctint.c's 8x8 one, on dequantised
  blocks.
- ``scaled_planes`` / ``scaled_pixels``: jdmaster.c's per-component ``DCT_scaled_size``: luma blocks come out n x n with n = 8 / s, the
  chroma blocks of a 4:2:0 file 2n x 2n, so every plane already has the output's size and nothing is upsampled.
- ``boxed_resize_plan`` / ``boxed_resize``: ``Image.resize((ow, oh), BICUBIC, box=(0, 0, bw, bh), reducing_gap=2.0)`` for a float box that
  ends inside the last pixel: reduce by ``int(bw / ow / 2) or 1`` over the whole image, then resample from the box ``(0, 0, bw / fx,
  bh / fy)`` (C floats).
- ``thumbnail_of_file``: ``Image.thumbnail`` of an unloaded JPEG: draft scale from twice the requested size, scaled decode, libjpeg's
  YCbCr -> RGB, boxed resize to the size ``preserve_aspect_ratio`` gives for the ORIGINAL size.
"""
from __future__ import annotations

import numpy as np

import jpeg_entropy_ref as J
import jpeg_ref as R

CONST_BITS, PASS1_BITS = 13, 2


def draft_scale(w: int, h: int, rw, rh) -> int:
    s = min(w // rw, h // rh)
    for k in (8, 4, 2):
        if s >= k:
            return k
    return 1


def scaled_dims(h: int, w: int, s: int):
    """(oh, ow)"""
    return -(-h // s), -(-w // s)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct4_1d(c, axis, first):
    """one jpeg_idct_4x4 pass along `axis` (8 inputs, of which 4 is never read; 4 outputs)"""
    c = np.moveaxis(c, axis, 0)
    t0 = c[0] << (CONST_BITS + 1)
    t2 = c[2] * 15137 - c[6] * 6270
    t10, t12 = t0 + t2, t0 - t2
    o0 = -c[7] * 1730 + c[5] * 11893 - c[3] * 17799 + c[1] * 8697
    o2 = -c[7] * 4176 - c[5] * 4926 + c[3] * 7373 + c[1] * 20995
    sh = CONST_BITS - PASS1_BITS + 1 if first else CONST_BITS + PASS1_BITS + 3 + 1
    o = [_descale(t10 + o2, sh), _descale(t12 + o0, sh), _descale(t12 - o0, sh), _descale(t10 - o2, sh)]
    return np.moveaxis(np.stack(o), 0, axis)


def _idct2_1d(c, axis, first):
    c = np.moveaxis(c, axis, 0)
    t10 = c[0] << (CONST_BITS + 2)
    t0 = -c[7] * 5906 + c[5] * 6967 - c[3] * 10426 + c[1] * 29692
    sh = CONST_BITS - PASS1_BITS + 2 if first else CONST_BITS + PASS1_BITS + 3 + 2
    return np.moveaxis(np.stack([_descale(t10 + t0, sh), _descale(t10 - t0, sh)]), 0, axis)


def idct_reduced(blocks: np.ndarray, n: int) -> np.ndarray:
    """dequantised int64 blocks [..., 8 (row), 8 (column)] -> samples [..., n, n]; n = 8: jidctint.c"""
    if n == 8:
        return R.range_limit(R._idct_1d(R._idct_1d(blocks, -2, True), -1, False))
    if n == 4:
        return R.range_limit(_idct4_1d(_idct4_1d(blocks, -2, True), -1, False))
    if n == 2:
        return R.range_limit(_idct2_1d(_idct2_1d(blocks, -2, True), -1, False))
    assert n == 1
    return R.range_limit(_descale(blocks[..., :1, :1], 3))


def plane_geometry(plan: dict, s: int):
    """(ph, pw, n_luma, n_chroma): the planes' size in whole MCUs and the blocks' edge per component"""
    n = 8 // s
    if plan["components"] == 1:
        return plan["mcu_rows"] * n, plan["mcu_cols"] * n, n, 0
    return plan["mcu_rows"] * 2 * n, plan["mcu_cols"] * 2 * n, n, 2 * n


def scaled_planes(coef: np.ndarray, plan: dict, s: int):
    """The component planes of the decode at 1 / s in whole MCUs (what the device keeps): [Y] or [Y, Cb, Cr], each [ph, pw] int64"""
    nc = plan["components"]
    mx, my = plan["mcu_cols"], plan["mcu_rows"]
    _, _, n, nch = plane_geometry(plan, s)
    c = coef.astype(np.int64).reshape(my, mx, 6 if nc == 3 else 1, 8, 8)

    def idct(blocks, q, k):                                     # [by, bx, 8, 8] -> [by * k, bx * k]
        r = idct_reduced(blocks * np.array(q, np.int64).reshape(8, 8), k)
        return r.transpose(0, 2, 1, 3).reshape(r.shape[0] * k, r.shape[1] * k)

    if nc == 1:
        return [idct(c[:, :, 0], plan["quant"][0], n)]
    y = c[:, :, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * 2, mx * 2, 8, 8)
    return [idct(y, plan["quant"][0], n), idct(c[:, :, 4], plan["quant"][1], nch), idct(c[:, :, 5], plan["quant"][2], nch)]


def planes_to_pixels(planes, plan: dict, s: int) -> np.ndarray:
    oh, ow = scaled_dims(plan["height"], plan["width"], s)
    if plan["components"] == 1:
        return planes[0][:oh, :ow].astype(np.uint8)
    return np.stack([p[:oh, :ow] for p in planes], axis=2).astype(np.uint8)


def scaled_pixels(data: bytes, s: int, plan: dict = None) -> np.ndarray:
    """uint8 [oh,ow,3] YCbCr triples (4:2:0 files) or [oh,ow] samples (grey files) of ``draft`` with ``decoderconfig == (s, 0)``"""
    plan = plan or J.parse(data)
    coef, _ = J.decode_coefficients(data, plan)
    return planes_to_pixels(scaled_planes(coef, plan, s), plan, s)


# ------------------------------------------------------------------------------------------------------------ the boxed resize
def boxed_resize_plan(ow: int, oh: int, bw: float, bh: float, reducing_gap: float = 2.0):
    """(fx, fy, box float32 (x0, y0, x1, y1) in the reduced image) of ``resize((ow, oh), BICUBIC, box=(0, 0, bw, bh), reducing_gap)``"""
    fx = int(bw / ow / reducing_gap) or 1
    fy = int(bh / oh / reducing_gap) or 1
    box = (0.0, 0.0, bw, bh)
    if fx > 1 or fy > 1:
        box = (0.0, 0.0, bw / fx, bh / fy)                      # _get_safe_box is the whole image: the box ends inside the last pixel
    return fx, fy, tuple(float(np.float32(v)) for v in box)


def boxed_resize(img: np.ndarray, ow: int, oh: int, bw: float, bh: float) -> np.ndarray:
    H, W = img.shape[:2]
    if (W, H) == (ow, oh) and (bw, bh) == (W, H):
        return img
    fx, fy, box = boxed_resize_plan(ow, oh, bw, bh)
    a = R.reduce(img, fx, fy) if (fx > 1 or fy > 1) else img
    return R.resample(a, ow, oh, box)


def thumbnail_of_file(data: bytes, max_dim: int) -> np.ndarray:
    """``Image.open(file).thumbnail((max_dim, max_dim))`` of a 4:2:0 (RGB [h,w,3]) or grey ([h,w]) baseline file"""
    plan = J.parse(data)
    H, W = plan["height"], plan["width"]
    t = R.thumbnail_size(W, H, max_dim)
    s = 1 if t is None else draft_scale(W, H, 2.0 * max_dim, 2.0 * max_dim)
    px = scaled_pixels(data, s, plan) if s > 1 else J.decode_pixels(data, plan)
    if px.ndim == 3:
        px = R.ycc_to_rgb(px[..., 0], px[..., 1], px[..., 2])
    if t is None or (px.shape[1], px.shape[0]) == t:            # thumbnail() resizes only when the drafted size is not the final one
        return px
    return boxed_resize(px, t[0], t[1], W / s, H / s)
