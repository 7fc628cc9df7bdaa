"""CPU restatement of the extractor's text-region auto-crop (``enhanced_extractor.py::_auto_crop_text_region``) on the OpenCV 4.10
semantics of each call, in numpy / scipy.  The device path (csrc/autocrop.hip, ``bbocr_auto_crop``) is compared against it.

Every cv2 step is restated literally (the device folds the morphology; the tests pin that the two agree):
- ``GaussianBlur(gray, (3, 3), 0)``: the small-kernel table [1/4, 1/2, 1/4] as 8.8 fixed point, REFLECT_101.
- CLAHE 2.0 / 8x8: ``oracle.preprocess.clahe_u8``.
- ``adaptiveThreshold`` MEAN 35 / 10 and GAUSSIAN 31 / 5, ``THRESH_BINARY_INV``, border REPLICATE | ISOLATED.  The mean is boxFilter's
  integer sum times the float 1/1225, rounded half to even; the Gaussian mean is GaussianBlur's bit-exact 8-bit path (31 fixed-point taps,
  ``gaussian_taps_fixed``).  OpenCV 4.x blurs a float32 copy in adaptiveThreshold GAUSSIAN; the fixed-point 8-bit blur here can differ from
  that by one grey level of the local mean on some pixels, which the fixture comparison bounds.
- Otsu (``getThreshVal_Otsu_8u``) of the CLAHE output (``BINARY_INV``) and of the Sobel gradient (``BINARY``).
- morphology CLOSE (2 iterations = one rect of (k - 1) * 2 + 1) / OPEN 3x3 / dilate 11x3, border pixels never take part.
- ``findContours(RETR_EXTERNAL)`` + ``boundingRect``: the bounding boxes of the 8-connected foreground components that touch the image
  edge or are 4-adjacent to the 4-connected background component(s) touching the edge.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import ndimage

from oracle import preprocess as opp

FLT_EPSILON = 1.1920928955078125e-07


def gaussian_taps_fixed(n: int, sigma: float = 0.0):
    """getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (8 fraction bits): the left half rounded half to even with the error
    carried on, mirrored; the centre takes the rest of 256."""
    if sigma <= 0:
        sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    scale2x = -0.125 / (sigma * sigma)
    half = (n - 1) // 2
    v = [math.exp(float(x * x) * scale2x) for x in range(1 - n, 0, 2)]
    s = 0.0
    for t in v:
        s += t
    s = s * 2 + 1
    mul = 1.0 / s
    k = [0] * n
    err, total = 0.0, 0
    for i in range(half):
        adj = v[i] * mul * 256.0 + err
        r = int(round(adj))                     # Python round: half to even, like cvRound
        err = adj - r
        k[i] = k[n - 1 - i] = r
        total += r
    k[half] = 256 - 2 * total
    return k


def to_gray(img: np.ndarray) -> np.ndarray:
    return opp.bgr2gray(img) if img.ndim == 3 else np.ascontiguousarray(img)


def blur3(gray: np.ndarray) -> np.ndarray:
    p = np.pad(gray.astype(np.int64), 1, mode="reflect")
    hor = 64 * p[:, :-2] + 128 * p[:, 1:-1] + 64 * p[:, 2:]
    ver = 64 * hor[:-2] + 128 * hor[1:-1] + 64 * hor[2:]
    return np.clip((ver + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def _window_sum(a: np.ndarray, r: int, axis: int) -> np.ndarray:
    p = np.pad(a, [(r, r) if ax == axis else (0, 0) for ax in range(a.ndim)], mode="edge")
    c = np.cumsum(p, axis=axis, dtype=np.int64)
    c = np.concatenate([np.zeros_like(np.take(c, [0], axis=axis)), c], axis=axis)
    n = a.shape[axis]
    return np.take(c, np.arange(2 * r + 1, n + 2 * r + 1), axis=axis) - np.take(c, np.arange(0, n), axis=axis)


def adaptive_mean_inv(e: np.ndarray, block=35, c=10) -> np.ndarray:
    r = block // 2
    s = _window_sum(_window_sum(e.astype(np.int64), r, 1), r, 0)
    mean = np.rint(s.astype(np.float32) * np.float32(1.0 / (block * block))).astype(np.int64)
    mean = np.clip(mean, 0, 255)
    return e.astype(np.int64) - mean <= -c


def gaussian_fixed_u8(e: np.ndarray, n: int) -> np.ndarray:
    k = gaussian_taps_fixed(n)
    r = n // 2
    p = np.pad(e.astype(np.int64), ((0, 0), (r, r)), mode="edge")
    W = e.shape[1]
    hor = sum(k[i] * p[:, i:i + W] for i in range(n))
    q = np.pad(hor, ((r, r), (0, 0)), mode="edge")
    H = e.shape[0]
    ver = sum(k[i] * q[i:i + H] for i in range(n))
    return np.clip((ver + (1 << 15)) >> 16, 0, 255)


def adaptive_gauss_inv(e: np.ndarray, block=31, c=5) -> np.ndarray:
    return e.astype(np.int64) - gaussian_fixed_u8(e, block) <= -c


def otsu_threshold(img: np.ndarray) -> int:
    """getThreshVal_Otsu_8u, operation for operation in double."""
    h = np.bincount(img.ravel(), minlength=256)
    scale = 1.0 / img.size
    mu = 0.0
    for i in range(256):
        mu += float(i) * float(h[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p_i = float(h[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + float(i) * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma = sigma
            max_val = i
    return max_val


def sobel_grad(e: np.ndarray) -> np.ndarray:
    p = np.pad(e.astype(np.int64), 1, mode="reflect")
    H, W = e.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    dy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return np.minimum(np.minimum(np.abs(dx), 255) + np.minimum(np.abs(dy), 255), 255).astype(np.uint8)


def composite_mask(e: np.ndarray) -> np.ndarray:
    g = sobel_grad(e)
    return adaptive_mean_inv(e) | adaptive_gauss_inv(e) | (e <= otsu_threshold(e)) | (g > otsu_threshold(g))


def dilate(m: np.ndarray, kw: int, kh: int) -> np.ndarray:
    return ndimage.maximum_filter(m.view(np.uint8), size=(kh, kw), mode="constant", cval=0).astype(bool)


def erode(m: np.ndarray, kw: int, kh: int) -> np.ndarray:
    return ndimage.minimum_filter(m.view(np.uint8), size=(kh, kw), mode="constant", cval=1).astype(bool)


def morph_pass(m: np.ndarray, kw: int, kh: int) -> np.ndarray:
    cw, ch = (kw - 1) * 2 + 1, (kh - 1) * 2 + 1          # iterations=2 of a rect kernel, folded as OpenCV does
    closed = erode(dilate(m, cw, ch), cw, ch)
    opened = dilate(erode(closed, 3, 3), 3, 3)
    return dilate(opened, 11, 3)


def merged_mask(comp: np.ndarray) -> np.ndarray:
    return morph_pass(comp, 9, 3) | morph_pass(comp, 15, 5)


def external_components(fg: np.ndarray):
    """(mask of the external components' pixels, [(x, y, w, h)] of each external component)."""
    H, W = fg.shape
    lab, _ = ndimage.label(fg, structure=np.ones((3, 3), bool))
    blab, _ = ndimage.label(~fg, structure=ndimage.generate_binary_structure(2, 1))
    edge = np.zeros_like(fg)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    outer_ids = np.unique(blab[edge & ~fg])
    outer = np.isin(blab, outer_ids[outer_ids > 0])
    near = np.zeros_like(fg)
    near[:, 1:] |= outer[:, :-1]
    near[:, :-1] |= outer[:, 1:]
    near[1:, :] |= outer[:-1, :]
    near[:-1, :] |= outer[1:, :]
    ext_ids = np.unique(lab[fg & (edge | near)])
    ext_ids = ext_ids[ext_ids > 0]
    boxes = []
    objs = ndimage.find_objects(lab)
    for i in ext_ids:
        sy, sx = objs[i - 1]
        boxes.append((int(sx.start), int(sy.start), int(sx.stop - sx.start), int(sy.stop - sy.start)))
    return np.isin(lab, ext_ids), boxes


def crop_box(boxes, H: int, W: int, margin: int = 128):
    """enhanced_extractor.py:283-344: area filter, union, 3 % inflation of a small union, margin.  -> ((x0, y0, x1, y1) | None, kept)."""
    img_area = float(H * W)
    kept = [b for b in boxes if not (float(b[2] * b[3]) < 0.0001 * img_area or float(b[2] * b[3]) > 0.10 * img_area)]
    kept.sort(key=lambda b: (b[1], b[0], b[2], b[3]))
    if not kept:
        return None, kept
    x0 = min(b[0] for b in kept)
    y0 = min(b[1] for b in kept)
    x1 = max(b[0] + b[2] for b in kept)
    y1 = max(b[1] + b[3] for b in kept)
    if float((x1 - x0) * (y1 - y0)) < 0.12 * img_area:
        pad = int(0.03 * max(W, H))
        x0, y0, x1, y1 = max(0, x0 - pad), max(0, y0 - pad), min(W, x1 + pad), min(H, y1 + pad)
    x0, y0, x1, y1 = max(0, x0 - margin), max(0, y0 - margin), min(W, x1 + margin), min(H, y1 + margin)
    if x1 <= x0 or y1 <= y0:
        return None, kept
    return (x0, y0, x1, y1), kept


def stages(img: np.ndarray):
    """All intermediates: dict(clahe, composite, merged, external, boxes)."""
    e = opp.clahe_u8(blur3(to_gray(img)), 2.0)
    comp = composite_mask(e)
    merged = merged_mask(comp)
    ext, boxes = external_components(merged)
    return dict(clahe=e, composite=comp, merged=merged, external=ext, boxes=boxes)


def auto_crop(img: np.ndarray, margin: int = 128):
    """-> ((x0, y0, x1, y1) | None, kept component boxes sorted by (y, x))."""
    st = stages(img)
    return crop_box(st["boxes"], img.shape[0], img.shape[1], margin)
