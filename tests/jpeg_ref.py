"""CPU restatement of the extractor's OCR-input down-scaling (``enhanced_extractor.py:486-512``: ``Image.thumbnail`` to 1600 / 2400 px,
then a JPEG file at quality 90 / 95 that easyocr decodes) on the Pillow 12 / libjpeg-turbo semantics of each step, in numpy.  The device
path (csrc/thumb.hip, ``bbocr_ocr_thumbnail``) is compared against it; the installed Pillow is compared against both.

- ``thumbnail_size``: ``Image.thumbnail``'s ``preserve_aspect_ratio``.
- ``resize_plan``: ``Image.resize(..., reducing_gap=2.0)``: the ``reduce`` factors and the float32 box handed to ``ImagingResample``.
- ``reduce``: ``ImagingReduce`` (Reduce.c): the box mean ``((sum + n / 2) * multiplier) >> 24``, multiplier from ``division_UINT32``
  (single-precision float), partial last column / row averaged over the pixels they hold.
- ``resample_coeffs`` / ``resample``: ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` (bicubic a = -0.5, PRECISION_BITS 22) and the
  two passes (horizontal over the rows the vertical pass reads, then vertical; vertical first when the image is more than 100 times
  taller than wide), ``clip8`` after each.
- ``round_trip``: baseline 4:2:0 JPEG, ISLOW: jccolor.c RGB -> YCbCr, edge replication to the MCU, h2v2_downsample (bias 1, 2, ...),
  jfdctint.c, quantisation rounded half away from zero, jidctint.c with the ``& RANGE_MASK`` range limit, h2v2_fancy_upsample (plain
  replication when the chroma plane is at most 2 wide), jdcolor.c YCbCr -> RGB.  Returns (rgb, Y) like ``decode_file`` of the file.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22

STD_LUMINANCE = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
                 112, 100, 103, 99]
STD_CHROMINANCE = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                   99] + [99] * 32


# ------------------------------------------------------------------------------------------------------------------------ geometry
def thumbnail_size(w: int, h: int, max_dim: int):
    """``Image.thumbnail((max_dim, max_dim))``'s target (w, h), or None when the image is left as it is."""
    x, y = max_dim, max_dim
    if x >= w and y >= h:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = w / h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def resize_plan(w: int, h: int, ow: int, oh: int, reducing_gap: float = 2.0):
    """(fx, fy, box) of ``Image.resize((ow, oh), BICUBIC, reducing_gap=2.0)`` on a (w, h) image: the reduce factors and the box (x0, y0,
    x1, y1, float32) in the reduced image that ``ImagingResample`` gets."""
    fx = int(w / ow / reducing_gap) or 1
    fy = int(h / oh / reducing_gap) or 1
    box = (0.0, 0.0, float(w), float(h))
    if fx > 1 or fy > 1:
        # _get_safe_box of the full box is the whole image
        box = (0.0, 0.0, w / fx, h / fy)
    return fx, fy, tuple(float(np.float32(v)) for v in box)


def _division_u32(divider: int) -> int:
    return int(np.float32(4294967296.0) / np.float32(256 * divider))


def reduce(img: np.ndarray, fx: int, fy: int) -> np.ndarray:
    """``ImagingReduce(img, fx, fy)`` of a uint8 [H,W] or [H,W,C] image (whole box)."""
    a = img.astype(np.int64)
    H, W = a.shape[:2]
    oh, ow = -(-H // fy), -(-W // fx)
    pad = [(0, oh * fy - H), (0, ow * fx - W)] + [(0, 0)] * (a.ndim - 2)
    s = np.pad(a, pad).reshape((oh, fy, ow, fx) + a.shape[2:]).sum(axis=(1, 3))
    ny = np.minimum(fy, H - np.arange(oh) * fy)
    nx = np.minimum(fx, W - np.arange(ow) * fx)
    n = ny[:, None] * nx[None, :]
    mult = np.vectorize(_division_u32)(n)
    if a.ndim == 3:
        n, mult = n[..., None], mult[..., None]
    return ((((s + n // 2) * mult) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_coeffs(in_size: int, in0: float, in1: float, out_size: int):
    """``precompute_coeffs`` + ``normalize_coeffs_8bpc``: (bounds int [out, 2] = (xmin, count), coefficients int32 [out, ksize])."""
    f32 = np.float32
    scale = float(f32(in1) - f32(in0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    in0 = float(f32(in0))
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clip8(ss: np.ndarray) -> np.ndarray:
    return np.where(ss >= (1 << PRECISION_BITS << 8), 255, np.where(ss <= 0, 0, ss >> PRECISION_BITS)).astype(np.uint8)


def _apply(a: np.ndarray, bounds, kk, axis: int) -> np.ndarray:
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for i, (xmin, n) in enumerate(bounds):
        ss = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(n):
            ss += a[xmin + k] * int(kk[i, k])
        out[i] = _clip8(ss)
    return np.moveaxis(out, 0, axis)


def resample(img: np.ndarray, ow: int, oh: int, box) -> np.ndarray:
    """``ImagingResample(img, (ow, oh), BICUBIC, box)`` of a uint8 [H,W] or [H,W,C] image."""
    H, W = img.shape[:2]
    need_h = ow != W or box[0] != 0 or box[2] != W
    need_v = oh != H or box[1] != 0 or box[3] != H
    bh, kh = resample_coeffs(W, box[0], box[2], ow)
    bv, kv = resample_coeffs(H, box[1], box[3], oh)
    a = img
    if need_h and need_v and H > 100 * W:
        # Pillow 12 runs the vertical pass first on an image more than 100 times taller than wide (found against the installed Pillow)
        return np.ascontiguousarray(_apply(_apply(img, bv, kv, 0), bh, kh, 1))
    if need_h:
        y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        a = _apply(img[y0:y1], bh, kh, 1)
        bv = bv.copy()
        bv[:, 0] -= y0
    if need_v:
        a = _apply(a, bv, kv, 0)
    return np.ascontiguousarray(a)


def thumbnail(rgb: np.ndarray, max_dim: int) -> np.ndarray:
    """``Image.thumbnail((max_dim, max_dim))`` (bicubic, reducing_gap 2.0) of a uint8 image; the image itself when it is left as is."""
    H, W = rgb.shape[:2]
    t = thumbnail_size(W, H, max_dim)
    if t is None or t == (W, H):
        return rgb
    ow, oh = t
    fx, fy, box = resize_plan(W, H, ow, oh)
    a = reduce(rgb, fx, fy) if (fx > 1 or fy > 1) else rgb
    return resample(a, ow, oh, box)


# --------------------------------------------------------------------------------------------------------------------- JPEG
def qtables(quality: int):
    """``jpeg_set_quality(quality, force_baseline=TRUE)``: (luminance, chrominance), 64 entries each in natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    out = []
    for base in (STD_LUMINANCE, STD_CHROMINANCE):
        out.append(np.array([min(max((b * scale + 50) // 100, 1), 255) for b in base], np.int64).reshape(8, 8))
    return out


def rgb_to_ycc(rgb: np.ndarray):
    """jccolor.c::rgb_ycc_convert (16-bit fixed point tables)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half, off = 1 << 15, 128 << 16
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off + half - 1) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off + half - 1) >> 16
    return y, cb, cr


def ycc_to_rgb(y, cb, cr) -> np.ndarray:
    """jdcolor.c::ycc_rgb_convert (bbocr_op_ycc_to_rgb)."""
    y, cb, cr = (np.asarray(v, np.int64) for v in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819,
         c2562=20995, c3072=25172)
CONST_BITS, PASS1_BITS = 13, 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, axis, first):
    """One jfdctint.c pass along `axis` of int64 blocks [..., 8, 8]."""
    d = np.moveaxis(d, axis, 0)
    t0, t7 = d[0] + d[7], d[0] - d[7]
    t1, t6 = d[1] + d[6], d[1] - d[6]
    t2, t5 = d[2] + d[5], d[2] - d[5]
    t3, t4 = d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
        sh = CONST_BITS - PASS1_BITS
    else:
        o[0], o[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
        sh = CONST_BITS + PASS1_BITS
    z1 = (t12 + t13) * F["c0541"]
    o[2] = _descale(z1 + t13 * F["c0765"], sh)
    o[6] = _descale(z1 - t12 * F["c1847"], sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["c1175"]
    t4, t5, t6, t7 = t4 * F["c0298"], t5 * F["c2053"], t6 * F["c3072"], t7 * F["c1501"]
    z1, z2 = z1 * -F["c0899"], z2 * -F["c2562"]
    z3, z4 = z3 * -F["c1961"] + z5, z4 * -F["c0390"] + z5
    o[7] = _descale(t4 + z1 + z3, sh)
    o[5] = _descale(t5 + z2 + z4, sh)
    o[3] = _descale(t6 + z2 + z3, sh)
    o[1] = _descale(t7 + z1 + z4, sh)
    return np.moveaxis(np.stack(o), 0, axis)


def _idct_1d(c, axis, first):
    """One jidctint.c pass along `axis` of int64 blocks [..., 8, 8] (dequantised input)."""
    c = np.moveaxis(c, axis, 0)
    z2, z3 = c[2], c[6]
    z1 = (z2 + z3) * F["c0541"]
    t2, t3 = z1 - z3 * F["c1847"], z1 + z2 * F["c0765"]
    z2, z3 = c[0], c[4]
    if not first:
        z2 = z2 + (1 << (PASS1_BITS + 2))
    t0, t1 = (z2 + z3) << CONST_BITS, (z2 - z3) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["c1175"]
    t0, t1, t2, t3 = t0 * F["c0298"], t1 * F["c2053"], t2 * F["c3072"], t3 * F["c1501"]
    z1, z2 = z1 * -F["c0899"], z2 * -F["c2562"]
    z3, z4 = z3 * -F["c1961"] + z5, z4 * -F["c0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    if first:
        f = lambda v: _descale(v, CONST_BITS - PASS1_BITS)
    else:
        f = lambda v: v >> (CONST_BITS + PASS1_BITS + 3)
    o = [f(t10 + t3), f(t11 + t2), f(t12 + t1), f(t13 + t0), f(t13 - t0), f(t12 - t1), f(t11 - t2), f(t10 - t3)]
    return np.moveaxis(np.stack(o), 0, axis)


def range_limit(x):
    """jdmaster.c's post-IDCT table at ``x & RANGE_MASK`` (x before the +128 shift)."""
    i = np.asarray(x) & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.int64)


def block_round_trip(plane: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """FDCT -> quantise -> dequantise -> IDCT of a sample plane whose sides are multiples of 8 (int64 0..255)."""
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)         # [by, bx, row, col]
    d = _fdct_1d(_fdct_1d(b, 3, True), 2, False)
    qv = qt * 8
    coef = np.sign(d) * ((np.abs(d) + qv // 2) // qv)
    r = _idct_1d(coef * qt, 2, True)
    r = range_limit(_idct_1d(r, 3, False))
    return r.transpose(0, 2, 1, 3).reshape(h, w)


def _pad_edge(a, h, w):
    return np.pad(a, [(0, h - a.shape[0]), (0, w - a.shape[1])], mode="edge")


def encode_planes(rgb: np.ndarray, quality: int):
    """The reconstructed planes of the decoder: Y' [H,W] and Cb', Cr' [ceil(H/2), ceil(W/2)] (before upsampling)."""
    H, W = rgb.shape[:2]
    ql, qc = qtables(quality)
    y, cb, cr = rgb_to_ycc(rgb)
    yb = block_round_trip(_pad_edge(y, -(-H // 8) * 8, -(-W // 8) * 8), ql)[:H, :W]
    ch, cw = -(-H // 2), -(-W // 2)
    cbw = -(-W // 16) * 8                                   # chroma width_in_blocks * 8
    out = []
    for c in (cb, cr):
        full = _pad_edge(c, 2 * ch, 2 * cbw)                # expand_right_edge of the input rows, the odd last row replicated
        s = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
        bias = np.tile(np.array([1, 2], np.int64), cbw // 2)
        ds = (s + bias[None, :]) >> 2
        ds = _pad_edge(ds, -(-ch // 8) * 8, cbw)            # expand_bottom_edge of the downsampled plane to the iMCU
        out.append(block_round_trip(ds, qc)[:ch, :cw])
    return yb, out[0], out[1]


def upsample(c: np.ndarray, H: int, W: int) -> np.ndarray:
    """jdsample.c h2v2_fancy_upsample (or h2v2_upsample when the plane is at most 2 wide), cropped to [H, W]."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:H, :W]
    up = np.concatenate([c[:1], c[:-1]])
    dn = np.concatenate([c[1:], c[-1:]])
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2] = 3 * c + up
    rows[1::2] = 3 * c + dn
    left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out[:H, :W]


def round_trip_ycc(rgb: np.ndarray, quality: int):
    """(Y', Cb'', Cr'') at full resolution: the YCbCr triple ``decode_file_ycc`` of the saved file holds."""
    H, W = rgb.shape[:2]
    y, cb, cr = encode_planes(rgb, quality)
    return y.astype(np.uint8), upsample(cb, H, W).astype(np.uint8), upsample(cr, H, W).astype(np.uint8)


def round_trip(rgb: np.ndarray, quality: int):
    """``decode_file`` of ``Image.fromarray(rgb).save(JPEG, quality=quality)``: (rgb uint8 [H,W,3], Y uint8 [H,W])."""
    y, cb, cr = round_trip_ycc(rgb, quality)
    return ycc_to_rgb(y, cb, cr), y


def ocr_input(page: np.ndarray, max_dim: int, quality: int):
    """``extractor_batch._ocr_input_array`` for a gray [H,W] or BGR [H,W,3] page (after decoding): (rgb, gray)."""
    rgb = np.ascontiguousarray(np.repeat(page[:, :, None], 3, 2) if page.ndim == 2 else page[:, :, ::-1])
    if max(page.shape[:2]) > max_dim:
        return round_trip(thumbnail(rgb, max_dim), quality)
    if page.ndim == 2:
        return rgb, page.copy()
    a = rgb.astype(np.int64)
    return rgb, ((a[..., 0] * 9797 + a[..., 1] * 19234 + a[..., 2] * 3737) >> 15).astype(np.uint8)
