"""The reference's OCR pre-processing on the device.

``pipeline_demo/ocr_testing/preprocessing/image_preprocessor.py::preprocess_for_book_cover(image_path, output_path=None)``
(:147-160) returns ``(image, output_path, steps_applied)``; the extractor calls it two to three times per page
(``enhanced_extractor.py:431,634,775``) on the CPU.  ``preprocess_for_book_cover`` here has the same signature and return shape
and runs the seven stages as HIP kernels (csrc/preproc.hip) through ``bbocr_preprocess_book_cover``; ``..._device`` keeps the
result in HBM so it can go straight into ``Reader.readtext_device``.

``cv2.imread`` applies the EXIF orientation and returns BGR; ``_imread_bgr`` does the same on the host with Pillow (the JPEG decoders
of OpenCV and Pillow builds may differ in the last bit of a pixel, which is outside this backend).  ``imread_bgr_device`` yields the same
page on the card: a baseline JPEG file goes from its bytes to the oriented BGR page without existing as host pixels (csrc/jpegdec.hip +
csrc/orient.hip); every other file is decoded once on the host, un-oriented, and oriented + channel-ordered on the card.
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np

from ._lib import PAGE_BGR, PAGE_GRAY, PAGE_PX_BYTES, PAGE_RGB, PAGE_YCBCR3, PAGE_YCBCR4  # noqa: F401  (re-exported)

LEGACY_STEPS = ["original", "grayscale", "resize(scale_factor=1.5)", "denoise(strength=5)", "increase_contrast(factor=1.3)",
                "clahe(clip_limit=2.0)", "sharpen(amount=0.2)"]
STEPS = ["original", "grayscale", "resize(scale_factor=1.5)", "denoise(strength=3)", "increase_contrast(factor=1.9)",
         "increase_brightness(factor=1.2)", "clahe(clip_limit=2.5)", "sharpen(amount=0.3)"]


def _imread_bgr(image_path):
    from PIL import Image, ImageOps

    pil = Image.open(image_path)
    pil = ImageOps.exif_transpose(pil)
    rgb = np.asarray(pil.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


ORIENT_TILE = 64                                  # csrc/kernels.h ORIENT_TILE: page_orient's tile edge in pixels (the tests' shapes)
IMREAD_JPEG, IMREAD_YCC, IMREAD_RGB = "jpeg", "ycc", "rgb"       # the path imread_bgr_device took (``.imread_path`` of its result)


def exif_orientation(value):
    """The rule of ``bbocr_jpeg_plan::orientation`` for a tag value read elsewhere: 1 .. 8 as it is, anything else 1"""
    return int(value) if isinstance(value, int) and 1 <= value <= 8 else 1


def page_descriptor(shape, strides, dtype, layouts):
    """``(H, W, row pitch in bytes, channels)`` of a page given as a tensor's ``shape``, ``strides`` (in elements) and ``dtype``: uint8,
    ``[H,W]`` or ``[H,W,C]`` with ``H, W >= 1``, ``C`` the bytes per pixel of one of the allowed ``PAGE_*`` ``layouts``, pixels packed along a
    row, rows at least one row apart (a strided view such as a crop of a larger page qualifies).  ``ValueError`` for anything else."""
    import torch

    ch = int(shape[2]) if len(shape) == 3 else 1
    ok = dtype == torch.uint8 and len(shape) in (2, 3) and any(PAGE_PX_BYTES.get(l) == ch for l in layouts)
    if not ok or shape[0] < 1 or shape[1] < 1 or strides[1] != ch or (len(shape) == 3 and strides[2] != 1) or strides[0] < shape[1] * ch:
        raise ValueError(f"expected a uint8 page of layout {tuple(layouts)} (BBOCR_PAGE_*) as rows of packed pixels, not {dtype} of shape "
                         f"{tuple(shape)} / strides {tuple(strides)}")
    return int(shape[0]), int(shape[1]), int(strides[0]), ch


def _on_device(reader, t):
    if not t.is_cuda or t.device.index != reader.device_index:
        raise ValueError(f"expected a tensor on {reader.device}")


def _page_layout(reader, page_dev, layouts=(PAGE_GRAY, PAGE_BGR)):
    """``page_descriptor`` of a tensor on the reader's device (by default a gray [H,W] or BGR [H,W,3] page)."""
    import torch

    if not isinstance(page_dev, torch.Tensor):
        raise ValueError("expected a uint8 [H,W] or [H,W,C] device tensor")
    d = page_descriptor(page_dev.shape, page_dev.stride(), page_dev.dtype, layouts)
    _on_device(reader, page_dev)
    return d


def orient_page_device(reader, page_dev, layout, orientation, dst_layout=None):
    """``bbocr_page_orient`` of a uint8 device page of the given ``PAGE_*`` layout (rows of packed pixels; a strided row pitch is read in
    place): the page in EXIF ``orientation`` (1 .. 8, ``ImageOps.exif_transpose``'s geometry) as ``dst_layout`` -- ``PAGE_BGR`` (default) or
    ``PAGE_RGB`` ``[H',W',3]`` from every layout, ``PAGE_GRAY`` ``[H',W']`` from a gray page.  A new tensor; the source is left as it is."""
    import torch

    dst_layout = PAGE_BGR if dst_layout is None else dst_layout
    H, W, pitch, _ = _page_layout(reader, page_dev, (layout,))
    if dst_layout not in (PAGE_BGR, PAGE_RGB) and not (dst_layout == PAGE_GRAY and layout == PAGE_GRAY):
        raise ValueError(f"no conversion from layout {layout} to layout {dst_layout}")
    if not isinstance(orientation, int) or not 1 <= orientation <= 8:
        raise ValueError("orientation must be 1 .. 8")
    oh, ow = (W, H) if orientation >= 5 else (H, W)
    out = torch.empty((oh, ow) if dst_layout == PAGE_GRAY else (oh, ow, 3), dtype=torch.uint8, device=page_dev.device)
    torch.cuda.current_stream(reader.device_index).synchronize()       # the library runs on its own stream
    rh, rw = C.c_int(), C.c_int()
    reader._check(reader._lib.bbocr_page_orient(reader._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, int(layout), int(orientation),
                                                int(dst_layout), C.c_void_p(out.data_ptr()), int(out.stride(0)), C.byref(rh), C.byref(rw)))
    return out


def imread_bgr_device(reader, source, device_decode=None):
    """``reader._to_dev(_imread_bgr(source))`` without the host's oriented page: ``cv2.imread``'s BGR page, uint8 ``[H',W',3]`` on the
    reader's device, bit for bit.  ``source``: a path or the file's bytes.  Three paths, tried in this order; the one taken is recorded
    as ``.imread_path`` of the returned tensor:

    * ``IMREAD_JPEG`` -- the device decoder's plan takes the file: only its bytes cross the link (``bbocr_jpeg_imread``); with
      ``device_decode="chroma"`` (None: the reader's ``jpeg_chroma``) that includes a 4:4:4, 4:2:2 or 4:4:0 file (``plan.chroma``);
    * ``IMREAD_YCC``  -- a YCbCr-coded JPEG the plan refuses (progressive, 4:4:4, ...) or whose entropy-coded data the device decoder
      reports damaged: ``decode_file_ycc`` on the host, the un-oriented triples uploaded, oriented and converted on the card;
    * ``IMREAD_RGB``  -- everything else: Pillow's un-oriented ``convert("RGB")``, uploaded, oriented and channel-swapped on the card.

    The orientation is the plan's (EXIF IFD0, OpenCV's rule) for the first two and ``Image.getexif()`` under the same 1 .. 8 rule for the
    third.  ``_imread_bgr`` (Pillow's ``exif_transpose``) also honours an XMP ``tiff:Orientation`` when the EXIF block has no tag; OpenCV
    and this function do not."""
    from PIL import Image

    from .reader import JpegPage, _file_bytes, decode_file_ycc, jpeg_chroma, jpeg_device_plan, jpeg_plan, jpeg_progressive

    chroma = getattr(reader, "jpeg_chroma", False) if device_decode is None else jpeg_chroma(device_decode)
    progressive = getattr(reader, "jpeg_progressive", False) if device_decode is None else jpeg_progressive(device_decode)
    data = _file_bytes(source)
    plan = jpeg_plan(data)
    out = path = None
    taken = jpeg_device_plan(data, chroma, progressive, plan)       # "progressive": a progressive file under its own plan
    if taken is not None:
        pages, status = reader.imread_jpeg_batch([JpegPage(data, taken)])
        if status[0] == 0:
            out, path = pages[0], IMREAD_JPEG
    if out is None:
        ycc = decode_file_ycc(data, padded=True)
        if ycc is not None:
            layout = PAGE_YCBCR4 if ycc.shape[2] == 4 else PAGE_YCBCR3
            out, path = orient_page_device(reader, reader._to_dev(ycc), layout, exif_orientation(plan.orientation)), IMREAD_YCC
    if out is None:
        pil = Image.open(io.BytesIO(data))
        o = exif_orientation(pil.getexif().get(0x0112))
        out, path = orient_page_device(reader, reader._to_dev(np.asarray(pil.convert("RGB"))), PAGE_RGB, o), IMREAD_RGB
    out.imread_path = path
    return out


def preprocess_bgr_device(reader, bgr_dev, legacy=False, **overrides):
    """uint8 torch tensor [H,W,3] (BGR, on the reader's device) -> uint8 torch tensor [int(H*1.5), int(W*1.5)] (gray).
    ``legacy=True``: the parameters of pipeline_components/.../image_preprocessor.py:221-252; ``overrides``: fields of
    ``bbocr_preproc_params`` (a stage whose parameter is 0 is skipped)."""
    import torch

    from . import _lib

    if not isinstance(bgr_dev, torch.Tensor) or bgr_dev.ndim != 3:
        raise ValueError("expected a uint8 [H,W,3] device tensor")
    H, W, ch = bgr_dev.shape
    if (ch != 3 or bgr_dev.dtype != torch.uint8 or not bgr_dev.is_contiguous() or not bgr_dev.is_cuda
            or bgr_dev.device.index != reader.device_index):
        raise ValueError(f"expected a contiguous uint8 [H,W,3] tensor on {reader.device}")
    q = _lib.bbocr_preproc_params()
    reader._lib.bbocr_preproc_defaults(C.byref(q), int(bool(legacy)))
    for k, v in overrides.items():
        if not hasattr(q, k):
            raise ValueError(f"unknown pre-processing parameter {k!r}")
        setattr(q, k, v)
    oh, ow = C.c_int(), C.c_int()
    reader._check(reader._lib.bbocr_preprocess_chain(reader._h, C.c_void_p(bgr_dev.data_ptr()), H, W, C.byref(q), C.c_void_p(None), C.byref(oh),
                                                    C.byref(ow)))
    out = torch.empty((oh.value, ow.value), dtype=torch.uint8, device=bgr_dev.device)
    reader._check(reader._lib.bbocr_preprocess_chain(reader._h, C.c_void_p(bgr_dev.data_ptr()), H, W, C.byref(q), C.c_void_p(out.data_ptr()),
                                                    C.byref(oh), C.byref(ow)))
    return out


def preprocess_for_book_cover(image_path, output_path=None, reader=None, legacy=False, device_decode=False):
    """Drop-in for the reference function: ``(gray uint8 array, output_path, steps_applied)``.  ``image_path`` may also be a
    decoded BGR array.  ``reader`` supplies the device context (any ``bb_ocr_amd.Reader``).  ``legacy=True`` runs the older
    ``preprocess_for_book_cover`` of pipeline_components/img_to_json/ocr_testing/preprocessing/image_preprocessor.py:221-252.
    ``device_decode=True``: a path is read by ``imread_bgr_device`` (same pixels); ``"chroma"``: 4:4:4, 4:2:2 and 4:4:0 files are decoded
    on the card as well."""
    if reader is None:
        raise ValueError("preprocess_for_book_cover needs a bb_ocr_amd.Reader (device context)")
    if isinstance(image_path, np.ndarray):
        page = reader._to_dev(np.ascontiguousarray(image_path))
    else:
        if not os.path.exists(image_path):
            raise ValueError(f"Could not load image from {image_path}")      # image_preprocessor.py:19-20
        page = imread_bgr_device(reader, image_path, device_decode) if device_decode else reader._to_dev(_imread_bgr(image_path))
    out = preprocess_bgr_device(reader, page, legacy=legacy).cpu().numpy()
    if output_path:
        from PIL import Image

        os.makedirs(os.path.dirname(output_path) or ".", exist_ok=True)
        Image.fromarray(out).save(output_path)
    return out, output_path, list(LEGACY_STEPS if legacy else STEPS)


# ------------------------------------------------------------------------------------------------ crops of the extractor's OCR input
def central_edge_crop_box(h, w, percent):
    """``_central_edge_crop`` (enhanced_extractor.py:374-397) as a box: ``(x0, y0, x1, y1)`` with ``percent`` removed from every edge,
    or None where the reference returns None (``percent <= 0``, or what is left is narrower than max(16, 20 %) on either axis)."""
    if percent <= 0.0:
        return None
    mx = int(round(w * (percent / 100.0)))
    my = int(round(h * (percent / 100.0)))
    x0, y0 = max(0, mx), max(0, my)
    x1, y1 = min(w, w - mx), min(h, h - my)
    if x1 - x0 < max(16, w * 0.2) or y1 - y0 < max(16, h * 0.2):
        return None
    return (x0, y0, x1, y1)


def auto_crop_box_device(reader, page_dev, margin=128, with_components=False):
    """``_auto_crop_text_region`` (enhanced_extractor.py:239-372) on the device: the crop box ``(x0, y0, x1, y1)`` of a uint8 gray
    [H,W] or BGR [H,W,3] tensor on the reader's device (a strided view such as an edge crop of a larger page is read in place), or None
    where the reference returns None.  ``with_components=True`` also returns the kept component boxes ``(x, y, w, h)`` sorted by (y, x)."""
    if int(margin) < 0:
        raise ValueError("margin must be >= 0")
    H, W, pitch, ch = _page_layout(reader, page_dev)
    box = (C.c_int * 4)()
    found, n = C.c_int(), C.c_int()
    cap = 4096
    while True:
        comps = (C.c_int * (4 * cap))()
        reader._check(reader._lib.bbocr_auto_crop(reader._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, ch, int(margin), box, C.byref(found),
                                                  comps, cap, C.byref(n)))
        if n.value <= cap or not with_components:
            break
        cap = n.value
    out = tuple(box) if found.value else None
    if with_components:
        return out, [tuple(comps[4 * k:4 * k + 4]) for k in range(n.value)]
    return out


# ------------------------------------------------------------------------------------------------ the OCR input itself (:486-512)
def ocr_thumbnail_rule(image_index=None):
    """(max_dim, JPEG quality) of the extractor's down-scaling step: 1600 / 90 for the cover (``image_index`` None or 0), else 2400 / 95."""
    return (1600, 90) if image_index is None or image_index == 0 else (2400, 95)


def ocr_thumbnail_device(reader, page_dev, layout, max_dim, quality):
    """``bbocr_ocr_thumbnail`` of a uint8 device page of the given ``PAGE_*`` layout (rows of packed pixels; a strided row pitch is read
    in place) -> ``(rgb_dev [h,w,3], gray_dev [h,w])``."""
    import torch

    H, W, pitch, _ = _page_layout(reader, page_dev, (layout,))
    oh, ow = C.c_int(), C.c_int()
    reader._check(reader._lib.bbocr_thumbnail_dims(H, W, int(max_dim), C.byref(oh), C.byref(ow)))
    rgb = torch.empty((oh.value, ow.value, 3), dtype=torch.uint8, device=page_dev.device)
    gray = torch.empty((oh.value, ow.value), dtype=torch.uint8, device=page_dev.device)
    reader._check(reader._lib.bbocr_ocr_thumbnail(reader._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, int(layout), int(max_dim),
                                                  int(quality), C.c_void_p(rgb.data_ptr()), C.c_void_p(gray.data_ptr()), C.byref(oh),
                                                  C.byref(ow)))
    return rgb, gray


def ocr_input_device(reader, page_dev, image_index=None):
    """``extractor_batch._ocr_input_array`` on the device: a uint8 gray [H,W] or BGR [H,W,3] tensor on the reader's device (a strided view
    such as an edge or auto crop is read in place) -> ``(rgb_dev [h,w,3], gray_dev [h,w])``, the pages ``readtext`` sees.  Above 1600 px
    (cover) / 2400 px the page is thumbnailed and goes through the JPEG round trip of the file the reference writes, to the bit."""
    H, W, _, ch = _page_layout(reader, page_dev)
    m, q = ocr_thumbnail_rule(image_index)
    return ocr_thumbnail_device(reader, page_dev, PAGE_GRAY if ch == 1 else PAGE_BGR, m, q)


def ocr_input_ycc_device(reader, ycc_dev, image_index=None):
    """``extractor_batch._ocr_input`` on the device for a YCbCr-coded JPEG file: ``ycc_dev`` is its ``decode_file_ycc`` decode (uint8
    [H,W,4] Pillow's padded pixels, or [H,W,3]) on the reader's device.  ``Image.open(path)`` without EXIF transpose, as the reference
    reads it -> ``(rgb_dev, gray_dev)``."""
    m, q = ocr_thumbnail_rule(image_index)
    layout = PAGE_YCBCR4 if ycc_dev.ndim == 3 and ycc_dev.shape[2] == 4 else PAGE_YCBCR3
    return ocr_thumbnail_device(reader, ycc_dev, layout, m, q)


# ------------------------------------------------------------------------------------------------ the trace previews (:184-199)
PREVIEW_MAX_DIM = 800                                   # _image_to_data_url's max_dim


def _png_data_url(img):
    """``img.save(buf, format="PNG")`` as the ``data:image/png;base64,...`` string of ``_image_to_data_url``"""
    import base64

    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode("utf-8")


def preview_host(source, max_dim=PREVIEW_MAX_DIM):
    """``_image_to_data_url(path, max_dim=max_dim)`` (:184-199) restated with Pillow: ``Image.open(path)``, ``thumbnail((max_dim, max_dim))``
    -- which decodes an unloaded JPEG file at the draft scale -- ``save(format="PNG")``, base64.  ``source``: a path or the file's bytes, or a
    page the reference would have written as a PNG on the way (gray [H,W] or BGR [H,W,3] uint8).  The mode is kept (L stays L), the
    file's ICC profile goes into the PNG, and the EXIF orientation is not applied.  The yardstick of ``preview_device``, and the path of
    sources the device does not take."""
    from PIL import Image

    if isinstance(source, np.ndarray):
        img = Image.fromarray(np.ascontiguousarray(source if source.ndim == 2 else source[:, :, ::-1]))
    else:
        img = Image.open(io.BytesIO(source) if isinstance(source, (bytes, bytearray)) else source)
    img.thumbnail((max_dim, max_dim))
    return _png_data_url(img)


def thumbnail_box_device(reader, page_dev, layout, out_h, out_w, box_w, box_h):
    """``bbocr_thumbnail_box``: ``Image.resize((out_w, out_h), BICUBIC, box=(0, 0, box_w, box_h), reducing_gap=2.0)`` of a uint8 device page
    of the given ``PAGE_*`` layout (a strided row pitch is read in place), for a box that ends inside the last pixel -> RGB
    ``[out_h,out_w,3]``, or ``[out_h,out_w]`` for a gray page."""
    import torch

    H, W, pitch, _ = _page_layout(reader, page_dev, (layout,))
    out = torch.empty((out_h, out_w) if layout == PAGE_GRAY else (out_h, out_w, 3), dtype=torch.uint8, device=page_dev.device)
    torch.cuda.current_stream(reader.device_index).synchronize()       # the library runs on its own stream
    reader._check(reader._lib.bbocr_thumbnail_box(reader._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, int(layout), int(out_h), int(out_w),
                                                  float(box_w), float(box_h), C.c_void_p(out.data_ptr())))
    return out


def preview_draft_scale(plan, max_dim=PREVIEW_MAX_DIM):
    """The scale ``Image.thumbnail((max_dim, max_dim))`` decodes an unloaded JPEG file of the plan's size at: ``draft(None, size *
    reducing_gap)``'s, 1 for a file that is not resized"""
    from .reader import draft_scale

    H, W = int(plan.height), int(plan.width)
    return draft_scale(W, H, int(max_dim * 2.0), int(max_dim * 2.0)) if max(H, W) > int(max_dim) else 1


def _preview_of_decode(reader, page, plan, s, max_dim):
    """``Image.thumbnail((max_dim, max_dim))``'s pixels from the file's decode at its draft scale ``s`` (``page``: the decoder's own tensor,
    padded YCbCr [oh,ow,4] or gray [oh,ow]): RGB [h,w,3] or gray [h,w] on the card"""
    H, W = int(plan.height), int(plan.width)
    oh, ow = C.c_int(), C.c_int()
    reader._check(reader._lib.bbocr_thumbnail_dims(H, W, int(max_dim), C.byref(oh), C.byref(ow)))
    oh, ow = oh.value, ow.value
    layout = PAGE_GRAY if page.ndim == 2 else PAGE_YCBCR4
    if max(H, W) <= int(max_dim) or (page.shape[0], page.shape[1]) == (oh, ow):         # no resize: the (drafted) decode itself
        return page if layout == PAGE_GRAY else reader.pages_from_ycc(page[None])[0][0]
    return thumbnail_box_device(reader, page, layout, oh, ow, W / s, H / s)


def _preview_jpeg_device(reader, data, plan, max_dim):
    """``Image.open(file).thumbnail((max_dim, max_dim))`` of a file the decoder takes, on the card: the pixels (RGB [h,w,3] or gray [h,w],
    a device tensor), or None when the decoder reports the entropy-coded data damaged.  A file of a chroma class goes through
    ``bbocr_jpeg_decode_scales``, which decodes it at every scale; every other file through ``bbocr_jpeg_decode_scaled`` as before."""
    from .reader import JpegPage

    s = preview_draft_scale(plan, max_dim)
    if plan.supported:
        t, status = reader.decode_jpeg_batch([JpegPage(data, plan)], padded=True, scale=s)
        page = t[0]
    else:
        decodes, status = reader.decode_jpeg_scales_batch([JpegPage(data, plan)], (s,))
        page = decodes[0][s]
    if status[0] != 0:
        return None
    return _preview_of_decode(reader, page, plan, s, max_dim)


PNG_PILLOW, PNG_DEVICE = "pillow", "device"               # who writes a preview's PNG file (the `png` argument)


def png_writer(png=None):
    """The ``png`` argument of the preview functions resolved: ``"pillow"`` (the reference's strings) or ``"device"`` (``Reader.encode_png``:
    other strings that decode to the same image).  None: ``"device"`` when the environment has ``BBOCR_PNG_DEVICE=1``, else ``"pillow"``."""
    if png is None:
        return PNG_DEVICE if os.environ.get("BBOCR_PNG_DEVICE") == "1" else PNG_PILLOW
    if png not in (PNG_PILLOW, PNG_DEVICE):
        raise ValueError(f"png must be {PNG_PILLOW!r} or {PNG_DEVICE!r}, not {png!r}")
    return png


def _preview_string(px, icc, reader=None, png=PNG_PILLOW):
    """the preview of the pixels made on the card (a device tensor, gray [h,w] or RGB [h,w,3]), the file's ICC profile embedded:
    ``png="pillow"`` -- the pixels come back and Pillow writes the PNG; ``"device"`` -- ``reader.encode_png`` writes it on the card and only
    the file comes back (lossless, same mode / size / pixels / profile when decoded, but not Pillow's bytes)"""
    from PIL import Image

    if png == PNG_DEVICE:
        import base64

        data = reader.encode_png(px, PAGE_GRAY if px.ndim == 2 else PAGE_RGB, icc)
        return "data:image/png;base64," + base64.b64encode(data).decode("utf-8")
    img = Image.fromarray(px.cpu().numpy())
    if icc:
        img.info["icc_profile"] = icc
    return _png_data_url(img)


PREVIEW_JPEG, PREVIEW_PAGE, PREVIEW_HOST = "device-jpeg", "device-page", "host"     # preview_device's routes (info["route"])


def preview_device(reader, source, max_dim=PREVIEW_MAX_DIM, device_decode=True, info=None, png=None):
    """``preview_host(source, max_dim)``, character for character, with the pixels made on the card; only the page of at most ``max_dim``
    pixels comes back, and Pillow writes the PNG from it.  ``info``: a dict that receives the route taken as ``info["route"]`` (the
    strings are equal whichever it is).  ``png="device"`` (opt-in; default ``png_writer()``: ``"pillow"`` unless ``BBOCR_PNG_DEVICE=1``):
    on the two device routes the PNG file is written on the card as well (``Reader.encode_png``) and the pixels never come back.  The string
    is then NOT the reference's: the file is lossless and decodes to the same image -- mode, size, pixels, ``info["icc_profile"]`` -- but
    its bytes are not Pillow's.  The ``"host"`` route keeps Pillow either way.

    * ``"device-jpeg"`` -- a JPEG path or bytes the device decoder's plan supports (4:2:0 or grey baseline) and ``device_decode``: plan ->
      draft scale -> ``bbocr_jpeg_decode_scaled`` -> libjpeg's RGB -> ``bbocr_thumbnail_box``; the file's ICC profile is carried into the
      PNG as Pillow carries it.  ``device_decode="chroma"``: a 4:4:4, 4:2:2 or 4:4:0 file (``plan.chroma``) as well, decoded at its
      draft scale by ``bbocr_jpeg_decode_scales``; ``device_decode="progressive"``: those, and a progressive file its own plan supports
      (``bbocr_jpeg_decode_progressive``);
    * ``"device-page"`` -- a page already on the card (a uint8 tensor, gray [H,W] or BGR [H,W,3], a strided view included -- the f2 output
      or a crop): the whole-image thumbnail (``bbocr_ocr_thumbnail`` without its JPEG round trip); a gray page stays mode L;
    * ``"host"`` -- everything else (PNG, progressive / CMYK JPEG, 4:4:4 / 4:2:2 / 4:4:0 JPEG unless asked for, a file whose data is
      damaged, host arrays): ``preview_host``."""
    from PIL import Image

    from .reader import _file_bytes, jpeg_chroma, jpeg_device_plan, jpeg_progressive

    png = png_writer(png)
    px, icc, route = None, None, PREVIEW_HOST
    if hasattr(source, "is_cuda"):
        H, W, _, ch = _page_layout(reader, source)
        rgb, gray = ocr_thumbnail_device(reader, source, PAGE_GRAY if ch == 1 else PAGE_BGR, max_dim, 0)
        px, route = (gray if ch == 1 else rgb), PREVIEW_PAGE
    elif device_decode and not isinstance(source, np.ndarray):
        data = _file_bytes(source)
        plan = jpeg_device_plan(data, jpeg_chroma(device_decode), jpeg_progressive(device_decode))
        if plan is not None:
            px = _preview_jpeg_device(reader, data, plan, max_dim)
            icc = Image.open(io.BytesIO(data)).info.get("icc_profile")          # headers only
            source = data
            if px is not None:
                route = PREVIEW_JPEG
    if info is not None:
        info["route"] = route
    if px is None:
        return preview_host(source, max_dim)
    return _preview_string(px, icc, reader, png)


def _read_page(image_path_or_array):
    if isinstance(image_path_or_array, np.ndarray):
        return np.ascontiguousarray(image_path_or_array)
    if not os.path.exists(image_path_or_array):
        return None                                                   # cv2.imread -> None -> the reference returns None
    return _imread_bgr(image_path_or_array)


def auto_crop_text_region(image_path_or_array, margin=128, reader=None, device_decode=False):
    """Drop-in for ``_auto_crop_text_region(image_path, margin)``: the cropped page (an array, where the reference writes it to a PNG
    and returns the path) or None.  A path is decoded like ``cv2.imread`` (BGR, EXIF-transposed); an array may be gray or BGR.
    ``device_decode=True``: a path is read by ``imread_bgr_device``, and only the crop comes back from the card (same pixels);
    ``"chroma"``: 4:4:4, 4:2:2 and 4:4:0 files are decoded on the card as well."""
    if reader is None:
        raise ValueError("auto_crop_text_region needs a bb_ocr_amd.Reader (device context)")
    if device_decode and not isinstance(image_path_or_array, np.ndarray):
        if not os.path.exists(image_path_or_array):
            return None
        page = imread_bgr_device(reader, image_path_or_array, device_decode)
        b = auto_crop_box_device(reader, page, margin)
        return None if b is None else page[b[1]:b[3], b[0]:b[2]].contiguous().cpu().numpy()
    img = _read_page(image_path_or_array)
    if img is None:
        return None
    b = auto_crop_box_device(reader, reader._to_dev(img), margin)
    return None if b is None else img[b[1]:b[3], b[0]:b[2]].copy()


def central_edge_crop(image_path_or_array, percent):
    """Drop-in for ``_central_edge_crop(image_path, percent)``: the cropped page (an array) or None."""
    if percent <= 0.0:
        return None
    img = _read_page(image_path_or_array)
    if img is None:
        return None
    b = central_edge_crop_box(img.shape[0], img.shape[1], percent)
    return None if b is None else img[b[1]:b[3], b[0]:b[2]].copy()


# ------------------------------------------------------------------------------------------------ the model input (:399-411, :801-812)
def model_image_rule(image_index):
    """(max_dim, JPEG quality) the extractor passes to ``_encode_image_for_model`` (:809-810): 2000 / 88 for image 0, else 3200 / 95."""
    return (2000, 88) if image_index == 0 else (3200, 95)


def model_image_quality(quality):
    """``_encode_image_for_model``'s clamp of its ``jpeg_quality`` (:406)"""
    return int(max(50, min(95, quality)))


def model_image_host(source, max_dim, quality):
    """``_encode_image_for_model(path, max_dim=max_dim, jpeg_quality=quality)`` (:399-408) before its base64 step, restated with Pillow:
    ``Image.open(...).convert("RGB")``, ``thumbnail((max_dim, max_dim))``, ``save(format="JPEG", quality=clamp(quality, 50, 95))`` -> the
    file's bytes.  ``source``: a path or the file's bytes, or a page the reference would have written as a PNG on the way (gray [H,W] or
    BGR [H,W,3] uint8).  The yardstick of ``model_image_device``, and the path of sources the device decoder does not take."""
    from PIL import Image

    if isinstance(source, np.ndarray):
        img = Image.fromarray(np.ascontiguousarray(source if source.ndim == 2 else source[:, :, ::-1])).convert("RGB")
    else:
        img = Image.open(io.BytesIO(source) if isinstance(source, (bytes, bytearray)) else source).convert("RGB")
    img.thumbnail((max_dim, max_dim))
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=model_image_quality(quality))
    return buf.getvalue()


def model_image_device(reader, page_dev, layout, max_dim, quality, comment=None):
    """``model_image_host`` of a page that is on the card, byte for byte: a uint8 device page of the given ``PAGE_*`` layout (rows of packed
    pixels; a strided row pitch is read in place) above ``max_dim`` is thumbnailed there (``bbocr_ocr_thumbnail`` with quality 0: the
    resized RGB page, no round trip), then ``Reader.encode_jpeg`` writes the file (three components, quality clamped to 50 .. 95 like the
    reference's); a page at or below ``max_dim`` is encoded as it is.  ``comment``: the source file's ``info["comment"]``, which Pillow
    carries into the file it saves."""
    H, W, _, _ = _page_layout(reader, page_dev, (layout,))
    if max(H, W) > int(max_dim):
        page_dev, layout = ocr_thumbnail_device(reader, page_dev, layout, max_dim, 0)[0], PAGE_RGB
    return reader.encode_jpeg(page_dev, layout, quality=model_image_quality(quality), components=3, comment=comment)
