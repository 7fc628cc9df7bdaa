"""Caller-side batching for the reference's extractor.

``pipeline_demo/extractor/enhanced_extractor.py`` runs OCR page by page: the loop at :680-688 calls
``extract_text_with_ocr`` per image, which (after the optional crop logic) applies the down-scaling rule of :486-512 and then
``reader.readtext(path, paragraph=False, batch_size=1, workers=0)`` (:520), joins ``result[1]`` with spaces (:521) and maps any
exception to the empty string (:529-531).  ``extract_texts`` does the same for ALL pages of a book (or of many books) with ONE
``readtext_batched`` call per page shape, so the backend sees 64-page batches instead of single pages.

The LLM steps of the extractor stay where they are.  The optional OCR-input steps in front of the down-scaling (:425-485) run on
the card when asked for: ``use_preprocessing`` (f2, csrc/preproc.hip), ``edge_crop_percent`` (a strided view, no copy) and
``crop_for_ocr`` (the text-region auto-crop, csrc/autocrop.hip); only the final crop is downloaded.  The down-scaling rule is
restated exactly, including its JPEG round trip (the reference writes the thumbnail as JPEG quality 90/95 and lets easyocr decode it).
"""
from __future__ import annotations

import collections
import dataclasses
import io
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def _jpg_page(source, device_decode=True):
    """``("jpg", JpegPage, None)`` when the device decoder takes the file (a path or its bytes), else None.  ``device_decode``: the
    caller's option; ``"chroma"`` adds 4:4:4, 4:2:2 and 4:4:0 files (``reader.jpeg_chroma``), ``"progressive"`` those and progressive
    files (``reader.jpeg_progressive``)."""
    from .reader import jpeg_chroma, jpeg_page, jpeg_progressive

    page = jpeg_page(source, jpeg_chroma(device_decode), jpeg_progressive(device_decode))
    return None if page is None else ("jpg", page, None)


def _png_page(source):
    """``("png", PngPage, None)`` when the device PNG decoder takes the file (a path or its bytes), else None"""
    from .reader import png_page

    page = png_page(source)
    return None if page is None else ("png", page, None)


def _tiff_page(source, tiff_decode=True):
    """``("tiff", TiffPage, None)`` when the device TIFF decoder takes the file (a path or its bytes), else None.  ``tiff_decode``: the
    option's level as ``_tiff_level`` gives it -- with ``"fax"`` a CCITT file is taken as well"""
    from .reader import tiff_page

    page = tiff_page(source, tiff_decode == "fax")
    return None if page is None else ("tiff", page, None)


def _tiff_level(reader, tiff_decode):
    """the ``tiff_decode`` keyword of a caller (None: the Reader's) -> False, True or ``"fax"``"""
    from .reader import tiff_fax

    value = getattr(reader, "tiff_decode", False) if tiff_decode is None else tiff_decode
    return "fax" if value is not None and tiff_fax(value) else bool(value)


def _gif_page(source):
    """``("gif", GifPage, None)`` when the device GIF decoder takes the file (a path or its bytes), else None"""
    from .reader import gif_page

    page = gif_page(source)
    return None if page is None else ("gif", page, None)


def _bmp_page(source):
    """``("bmp", BmpPage, None)`` when the device BMP decoder takes the file (a path or its bytes), else None"""
    from .reader import bmp_page

    page = bmp_page(source)
    return None if page is None else ("bmp", page, None)


def _host_page(source, decode_once=True):
    """The host decode of a file (a path or its bytes) as a page: ``("ycc", triples, None)`` when it is a YCbCr-coded JPEG and
    ``decode_once`` (decoded once, RGB + Y plane derived on the card: reader.decode_file_ycc), else ``("rgb", rgb, gray)``."""
    from .reader import decode_file, decode_file_ycc

    if not isinstance(source, (bytes, bytearray)):
        source = os.fspath(source)
    ycc = decode_file_ycc(source, padded=True) if decode_once else None
    return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(decode_file(source))


def _thumbnail_jpeg(size, image_index, load_rgb):
    """The host's down-scaling step (:486-512) for a page of ``size`` (either order): above the page's limit (``ocr_thumbnail_rule``) the
    RGB image ``load_rgb()`` returns is ``Image.thumbnail``-ed and written as JPEG -> the file's bytes; None (nothing loaded) otherwise."""
    from .preprocess import ocr_thumbnail_rule

    max_dim, quality = ocr_thumbnail_rule(image_index)
    if max(size) <= max_dim:
        return None
    img = load_rgb()
    img.thumbnail((max_dim, max_dim))
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def _ocr_input(image_path, image_index=None, decode_once=True, device_decode=False, png_decode=False, tiff_decode=False, gif_decode=False, bmp_decode=False):
    """``ocr_input_image`` for the batching loop: ``("ycc", triples, None)`` when the file easyocr would be given is a YCbCr-coded JPEG
    (``_host_page``) -- every thumbnail is, it is written as one -- else ``("rgb", rgb, gray)``.  ``device_decode``: the file easyocr
    would be given travels as its bytes (``("jpg", JpegPage, None)``) when the device decoder takes it -- the original at or below the
    limit (only its header is read here), or the thumbnail as written."""
    from PIL import Image

    source = image_path
    try:
        img = Image.open(image_path)
        source = _thumbnail_jpeg(img.size, image_index, lambda: img.convert("RGB")) or image_path
    except Exception:
        pass                                                      # :511-514: any failure falls back to the original file
    page = _jpg_page(source, device_decode) if device_decode else None
    if page is None and png_decode and source is image_path:       # the original file, at or below the limit (a thumbnail is a JPEG)
        page = _png_page(source)
    if page is None and tiff_decode and source is image_path:      # likewise a TIFF file
        page = _tiff_page(source, tiff_decode)
    if page is None and gif_decode and source is image_path:       # likewise a GIF file
        page = _gif_page(source)
    if page is None and bmp_decode and source is image_path:       # likewise a BMP file
        page = _bmp_page(source)
    return page if page is not None else _host_page(source, decode_once)


def _ocr_input_array(page, image_index=None, decode_once=True):
    """``_ocr_input`` for a page the reference would have written as a PNG (its pre-processed / cropped file): gray [H,W] or BGR
    [H,W,3] uint8.  Gray pages are read back as three equal channels, so the RGB thumbnail is the gray one replicated."""
    from PIL import Image

    from .reader import decode_file

    rgb = np.ascontiguousarray(np.repeat(page[:, :, None], 3, axis=2) if page.ndim == 2 else page[:, :, ::-1])
    data = _thumbnail_jpeg(page.shape[:2], image_index, lambda: Image.fromarray(rgb))
    if data is not None:
        return _host_page(data, decode_once)
    if page.ndim == 2:
        return ("rgb", rgb, np.ascontiguousarray(page))
    buf = io.BytesIO()                                            # a colour page: through the PNG file the reference writes
    Image.fromarray(rgb).save(buf, format="PNG")
    return ("rgb",) + tuple(decode_file(buf.getvalue()))


def _ocr_input_device(reader, image_path, image_index=None, decode_once=True, device_decode=False):
    """``_ocr_input`` with the down-scaling on the card: a YCbCr-coded JPEG above the page's limit is decoded once on the host, uploaded
    and thumbnailed + JPEG round-tripped on the device (``("dev", rgb_dev, gray_dev)``); every other file takes ``_ocr_input``.
    ``device_decode``: a colour file the device decoder takes is decoded there as well -- above the limit it goes from its bytes to the
    OCR input without ever existing as host pixels; at or below it travels as ``"jpg"``."""
    from .preprocess import ocr_input_ycc_device, ocr_thumbnail_rule
    from .reader import decode_file_ycc

    m, _ = ocr_thumbnail_rule(image_index)
    page = _jpg_page(image_path, device_decode) if device_decode else None
    if page is not None and page[1].shape[2] == 3:
        if max(page[1].shape[:2]) <= m:
            return page
        ycc, status = reader.decode_jpeg_batch([page[1]], padded=True)
        if status[0] == 0:
            return ("dev",) + tuple(ocr_input_ycc_device(reader, ycc[0], image_index))
    ycc = decode_file_ycc(os.fspath(image_path), padded=True)
    if ycc is None:
        return _ocr_input(image_path, image_index, decode_once)        # PNG, gray or CMYK JPEG, ...: the host path
    if max(ycc.shape[0], ycc.shape[1]) <= m:
        return "ycc", ycc, None                                       # no thumbnail: what _ocr_input returns for it
    return ("dev",) + tuple(ocr_input_ycc_device(reader, reader._to_dev(ycc), image_index))


def ocr_page_crop(reader, image_path, use_preprocessing=False, edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128, on_device=False,
                  device_decode=False, applied=None, pages=None, page=None):
    """The page ``extract_text_with_ocr`` would hand to the down-scaling step (:425-485), as a host array: decoded like ``cv2.imread``
    (BGR, EXIF-transposed), uploaded, pre-processed on the card (gray), edge-cropped (a view) and auto-cropped on the card; only the
    final crop comes back.  A step that returns None in the reference leaves the page as it was.  ``on_device=True``: the crop stays on
    the card, as a (possibly strided) view of the device page.  ``device_decode=True``: the page is read by
    ``preprocess.imread_bgr_device`` -- a baseline JPEG file is decoded, oriented and channel-ordered on the card (same pixels);
    ``device_decode="chroma"``: 4:4:4, 4:2:2 and 4:4:0 files as well.  ``applied``: a list that receives the names of the steps that changed the page (where it stays empty the reference goes on with the
    original file).  ``pages``: a dict that receives, under the same names, the device page each of those steps left (views of one another
    where the step is a crop) -- what ``trace_previews`` draws from.  ``page``: ``cv2.imread``'s page of the file, already on the card (BGR
    ``[H',W',3]``, as ``imread_bgr_device`` returns it): the file is then not read again."""
    from .preprocess import _imread_bgr, auto_crop_box_device, central_edge_crop_box, imread_bgr_device, preprocess_bgr_device

    applied = [] if applied is None else applied

    def done(step):
        applied.append(step)
        if pages is not None:
            pages[step] = page

    if page is None:
        page = imread_bgr_device(reader, image_path, device_decode) if device_decode else reader._to_dev(_imread_bgr(image_path))
    if use_preprocessing:
        page = preprocess_bgr_device(reader, page)
        done("preprocess")
    if edge_crop_percent > 0.0:
        b = central_edge_crop_box(page.shape[0], page.shape[1], edge_crop_percent)
        if b is not None:
            page = page[b[1]:b[3], b[0]:b[2]]
            done("edge_crop")
    if crop_for_ocr:
        b = auto_crop_box_device(reader, page, crop_margin)
        if b is not None:
            page = page[b[1]:b[3], b[0]:b[2]]
            done("auto_crop")
    if on_device:
        return page
    return page.contiguous().cpu().numpy()


def ocr_input_image(image_path, image_index=None):
    """The pixels ``extract_text_with_ocr`` hands to easyocr for ``image_path`` (enhanced_extractor.py:486-512): pages whose
    longer side exceeds 1600 px (cover, ``image_index`` None or 0) / 2400 px (other pages) are ``Image.thumbnail``-ed to that
    size in RGB and re-encoded as JPEG quality 90 / 95; everything else is read as is.  Returns what ``reformat_input`` would
    produce for the file easyocr is given: (RGB uint8 [H,W,3], gray uint8 [H,W])."""
    from PIL import Image

    from .reader import decode_file, reformat_input

    try:
        img = Image.open(image_path)
        data = _thumbnail_jpeg(img.size, image_index, lambda: img.convert("RGB"))
        if data is not None:
            return decode_file(data)                              # what easyocr's loader sees: a JPEG file on disk
    except Exception:
        pass                                                      # :511-514: any failure falls back to the original file
    return reformat_input(os.fspath(image_path))


def extract_texts(reader, image_paths, ocr_image_indices=None, max_batch=64, decode_workers=None, decode_once=True, use_preprocessing=False,
                  edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128, device_thumbnail=False, device_decode=False, mixed=None,
                  png_decode=None, tiff_decode=None, gif_decode=None, bmp_decode=None, **readtext_kw):
    """``{index: text}`` for every index of ``ocr_image_indices`` (default: all pages), text = ``" ".join(r[1] for r in results)``
    exactly as :521; a page whose OCR fails gets ``""`` like :529-531.  Pages of equal (down-scaled) shape travel in one device
    batch of at most ``max_batch`` pages (``read_files`` with the reference's OCR-input rule as the decode step).
    ``use_preprocessing`` / ``edge_crop_percent`` / ``crop_for_ocr`` / ``crop_margin``: the extractor's settings of the same names
    (``ocr_page_crop``); with all of them off the pages are read as before.  ``device_thumbnail=True``: the down-scaling + JPEG round trip
    of :486-512 runs on the card (csrc/thumb.hip, identical pixels): a cropped page stays on the card from upload to OCR, and a
    YCbCr-coded JPEG above the limit is uploaded as decoded and shrunk there.  ``device_decode=True``: the decode step only reads the file
    and plans it (``bbocr_host_jpeg_plan``); baseline JPEG files -- the thumbnails included -- reach the card as their bytes and are
    decoded there, a whole batch by one call (csrc/jpegdec.hip, identical pixels); every other file, and a file whose data turns out
    damaged, takes the host decode as before.  With the crop settings the page is read like ``cv2.imread``, EXIF orientation included, and
    ``device_decode=True`` does that on the card as well (``preprocess.imread_bgr_device``: csrc/jpegdec.hip + csrc/orient.hip).
    ``device_decode="chroma"``: the same, and 4:4:4, 4:2:2 and 4:4:0 files -- which ``True`` leaves to the host -- are decoded there too.
    ``mixed``: ``read_files``' keyword -- pages of different (down-scaled) shapes share device batches.
    ``png_decode`` (None: the Reader's ``png_decode``): a PNG file at or below its page's limit that the device PNG decoder takes reaches
    the card as its bytes (kind ``"png"``); with the crop settings or ``device_thumbnail`` on, and above the limit, a PNG keeps today's path.
    ``tiff_decode`` (None: the Reader's ``tiff_decode``): the same for a TIFF file the device TIFF decoder takes (kind ``"tiff"``); ``"fax"``:
    CCITT files as well.
    ``gif_decode`` (None: the Reader's ``gif_decode``): the same for a GIF file the device GIF decoder takes (kind ``"gif"``).
    ``bmp_decode`` (None: the Reader's ``bmp_decode``): the same for a BMP file the device BMP decoder takes (kind ``"bmp"``)."""
    from .preprocess import ocr_input_device

    png_decode = bool(getattr(reader, "png_decode", False)) if png_decode is None else bool(png_decode)
    tiff_decode = _tiff_level(reader, tiff_decode)
    gif_decode = bool(getattr(reader, "gif_decode", False)) if gif_decode is None else bool(gif_decode)
    bmp_decode = bool(getattr(reader, "bmp_decode", False)) if bmp_decode is None else bool(bmp_decode)

    if use_preprocessing or edge_crop_percent > 0.0 or crop_for_ocr:
        if crop_margin < 0:
            raise ValueError("crop_margin must be >= 0")

        def decode(path, i):
            page = ocr_page_crop(reader, path, use_preprocessing, edge_crop_percent, crop_for_ocr, crop_margin, on_device=device_thumbnail,
                                 device_decode=device_decode)
            if device_thumbnail:
                return ("dev",) + tuple(ocr_input_device(reader, page, i))
            return _ocr_input_array(page, i, decode_once)
    elif device_thumbnail:
        decode = lambda path, i: _ocr_input_device(reader, path, i, decode_once, device_decode)
    else:
        decode = lambda path, i: _ocr_input(path, i, decode_once, device_decode, png_decode, tiff_decode, gif_decode, bmp_decode)
    res = read_files(reader, image_paths, ocr_image_indices, max_batch, decode_workers, decode=decode, mixed=mixed, **readtext_kw)
    return {i: " ".join(t[1] for t in r) for i, r in res.items()}


def _plain_input(path, i=None):
    """Decode step of ``read_files`` without the extractor's thumbnail rule: what ``Reader.readtext(path)`` would hold."""
    return _host_page(path)


def _plain_input_device(path, i=None, device_decode=True, png_decode=False, tiff_decode=False, gif_decode=False, bmp_decode=False):
    """``_plain_input`` with the device decoders: the file's bytes when one of them takes them (``png_decode``: PNG files too,
    ``tiff_decode``: TIFF files too, ``gif_decode``: GIF files too, ``bmp_decode``: BMP files too)"""
    return ((_jpg_page(path, device_decode) if device_decode else None) or (_png_page(path) if png_decode else None)
            or (_tiff_page(path, tiff_decode) if tiff_decode else None) or (_gif_page(path) if gif_decode else None)
            or (_bmp_page(path) if bmp_decode else None) or _plain_input(path, i))


@dataclasses.dataclass
class Batch:
    """What the stages of ``read_files`` hand on: the pages ``ids`` of one ``kind`` and one shape.  ``host`` / ``dev``: the kind's host and
    device payload (``KINDS``), None where there is none (yet, or after a failed upload); ``status``: per page, non-zero where the device
    payload does not hold it -- such a page is read on its own (``read_page``); None: it holds every page."""
    kind: str
    ids: list
    host: object = None
    dev: object = None
    status: list = None


def _dev_stack(ids, pages):
    import torch

    rgb, gray = torch.stack([a for a, _ in pages]), torch.stack([g for _, g in pages])
    torch.cuda.current_stream(rgb.device).synchronize()       # the library runs on its own stream
    return Batch("dev", ids, dev=(rgb, gray))


def _jpg_to_device(reader, b):
    # ONE decode call for the group, on the context's JPEG stream outside the call slots: it runs while both device workers are inside
    # their calls, like an upload.  (When it raises, the device worker decodes every page on the host.)
    dev, b.status = reader.decode_jpeg_batch(b.host, padded=True)
    return dev


def _jpg_read(reader, b, kw):
    from .reader import Reader

    good = [k for k, s in enumerate(b.status) if s == 0]
    pages = b.dev if len(good) == len(b.ids) else b.dev[good]
    return reader.readtext_device(*Reader.pages_from_jpeg(reader, pages), **kw)     # (unbound: a test double need not have the method)


def _jpg_read_page(reader, b, k, kw):
    kind, a, g = _host_page(b.host[k].data)              # the host decode of the file: what _plain_input returns for it
    return KINDS[kind].read_page(reader, KINDS[kind].stack(b.ids[k:k + 1], [(a, g)]), 0, kw)


def _png_to_device(reader, b):
    # ONE decode call for the group, on the context's decode stream outside the call slots, like a "jpg" group's
    dev, b.status = reader.decode_png_batch(b.host)
    return dev


def _png_read(reader, b, kw):
    good = [k for k, s in enumerate(b.status) if s == 0]
    rgb, gray = b.dev if len(good) == len(b.ids) else (b.dev[0][good], b.dev[1][good])
    return reader.readtext_device(rgb, gray, **kw)


def _tiff_to_device(reader, b):
    # ONE decode call for the group, on the context's decode stream outside the call slots, like a "png" group's
    dev, b.status = reader.decode_tiff_batch(b.host)
    return dev


def _pages_to_device(decode_pages):
    """the upload step of a kind whose decode call takes a shape per file (``decode_gif_pages``): ONE call for the group, its planes stacked"""
    def to_device(reader, b):
        import torch

        planes, b.status = getattr(reader, decode_pages)(b.host)
        rgb, gray = torch.stack([a for a, _ in planes]), torch.stack([g for _, g in planes])
        if rgb.is_cuda:
            torch.cuda.current_stream(rgb.device).synchronize()   # the library runs on its own stream
        return rgb, gray

    return to_device


# The page kinds.  A decoded page is the pair (a, b) of the decode callback's ``(kind, a, b)``; its grouping key is ``_page_key``.  Per kind:
#   stack(ids, pages) -> Batch           the assembler's step for a group
#   to_device(reader, batch) -> dev      the upload stage's step: the device payload (it may raise: the batch then travels without one)
#   read(reader, batch, kw)              ONE device call on the device payload, for the pages of status 0 -> their results
#   read_host(reader, batch, kw)         the same from the host payload, where a kind has one that a call takes; else None
#   read_page(reader, batch, k, kw)      page k alone, the retry unit -> its result
Kind = collections.namedtuple("Kind", "stack to_device read read_host read_page")
KINDS = {
    # host pages travel as LISTS: the Reader uploads them one by one into the device batch (no 236-MB np.stack on this thread)
    "rgb": Kind(stack=lambda ids, pages: Batch("rgb", ids, host=([a for a, _ in pages], [g for _, g in pages])),
                to_device=lambda r, b: (r._to_dev(b.host[0]), r._to_dev(b.host[1])),
                read=lambda r, b, kw: r.readtext_device(*b.dev, **kw),
                read_host=lambda r, b, kw: r.readtext_arrays(*b.host, **kw),
                read_page=lambda r, b, k, kw: r.readtext_arrays(b.host[0][k:k + 1], b.host[1][k:k + 1], **kw)[0]),
    # once-decoded YCbCr pages: RGB and the Y plane are derived on the card
    "ycc": Kind(stack=lambda ids, pages: Batch("ycc", ids, host=[a for a, _ in pages]),
                to_device=lambda r, b: r._to_dev(b.host),
                read=lambda r, b, kw: r.readtext_device(*r.pages_from_ycc(b.dev), **kw),
                read_host=lambda r, b, kw: r.readtext_ycc_arrays(b.host, **kw),
                read_page=lambda r, b, k, kw: r.readtext_ycc_arrays(b.host[k:k + 1], **kw)[0]),
    # pages already in HBM: one concatenation on the card, nothing to upload; the page-by-page retry reads slices of the same tensors
    "dev": Kind(stack=_dev_stack, to_device=lambda r, b: b.dev, read=lambda r, b, kw: r.readtext_device(*b.dev, **kw), read_host=None,
                read_page=lambda r, b, k, kw: r.readtext_device(b.dev[0][k:k + 1], b.dev[1][k:k + 1], **kw)[0]),
    # file bytes (JpegPage): decoded by the upload stage; a page it could not decode takes the host decode
    "jpg": Kind(stack=lambda ids, pages: Batch("jpg", ids, host=[p for p, _ in pages]), to_device=_jpg_to_device, read=_jpg_read,
                read_host=None, read_page=_jpg_read_page),
    # file bytes (PngPage): both planes decoded by the upload stage; a page it could not decode takes the host decode of its bytes
    "png": Kind(stack=lambda ids, pages: Batch("png", ids, host=[p for p, _ in pages]), to_device=_png_to_device, read=_png_read,
                read_host=None, read_page=_jpg_read_page),
    # file bytes (TiffPage): the "png" kind's grouping and retry rule
    "tiff": Kind(stack=lambda ids, pages: Batch("tiff", ids, host=[p for p, _ in pages]), to_device=_tiff_to_device, read=_png_read,
                 read_host=None, read_page=_jpg_read_page),
    # file bytes (GifPage): likewise; the decode call takes a shape per file, the group's planes are stacked behind it
    "gif": Kind(stack=lambda ids, pages: Batch("gif", ids, host=[p for p, _ in pages]), to_device=_pages_to_device("decode_gif_pages"),
                read=_png_read, read_host=None, read_page=_jpg_read_page),
    # file bytes (BmpPage): likewise
    "bmp": Kind(stack=lambda ids, pages: Batch("bmp", ids, host=[p for p, _ in pages]), to_device=_pages_to_device("decode_bmp_pages"),
                read=_png_read, read_host=None, read_page=_jpg_read_page),
}

# kinds of a mixed batch whose pages of ANY shapes share one decode call: kind -> the Reader's method
_PAGES_CALL = {"tiff": "decode_tiff_pages", "gif": "decode_gif_pages", "bmp": "decode_bmp_pages"}


def _mixed_stack(ids, pages):
    """``pages``: the decode callback's ``(kind, a, b)`` tuples themselves -- a mixed batch holds pages of any kind and shape"""
    return Batch("mixed", ids, host=list(pages))


def _mixed_to_device(reader, b):
    """Every page of a mixed batch as ``(rgb_dev [H,W,3], gray_dev [H,W] or None)``, by its own kind's upload step -- kept as a list, not
    stacked.  ``"jpg"`` pages of one decoded shape share one decode call, and so do ``"png"`` pages; ``"tiff"`` pages of ANY shapes share one
    (``bbocr_tiff_decode`` takes a shape per file), and so do ``"gif"`` and ``"bmp"`` pages (``_PAGES_CALL``).  ``status``: non-zero where a page did not reach the card.
    A failure is kept per page, as the reference's failure rule is per page: such a page is read on its own from its host copy
    (``_read_batch``) while the others still share the call.  The price: an upload failure that hits EVERY page (the card out of memory)
    turns the batch into single-page host reads without an error -- slower, same results -- exactly as a failed ``_upload`` does for a
    batch of one shape."""
    from .reader import Reader

    n = len(b.ids)
    dev, b.status = [None] * n, [-1] * n
    jpg, png, any_shape = {}, {}, {}
    for k, (kind, a, g) in enumerate(b.host):
        try:
            if kind in _PAGES_CALL:
                any_shape.setdefault(kind, []).append(k)
                continue
            if kind in ("jpg", "png"):
                (jpg if kind == "jpg" else png).setdefault(a.shape, []).append(k)
                continue
            if kind == "dev":                                  # already on the card: the (possibly strided) views are read in place
                dev[k], b.status[k] = (a, g), 0
                continue
            sub = KINDS[kind].stack(b.ids[k:k + 1], [(a, g)])
            d = KINDS[kind].to_device(reader, sub)
            rgb, gray = reader.pages_from_ycc(d) if kind == "ycc" else d
            dev[k], b.status[k] = (rgb[0], None if gray is None else gray[0]), 0
        except Exception:
            pass
    for ks in jpg.values():
        try:
            t, status = reader.decode_jpeg_batch([b.host[k][1] for k in ks], padded=True)
            rgb, gray = Reader.pages_from_jpeg(reader, t)
            for j, k in enumerate(ks):
                if status[j] == 0:
                    dev[k], b.status[k] = (rgb[j], gray[j]), 0
        except Exception:
            pass
    for ks in png.values():
        try:
            (rgb, gray), status = reader.decode_png_batch([b.host[k][1] for k in ks])
            for j, k in enumerate(ks):
                if status[j] == 0:
                    dev[k], b.status[k] = (rgb[j], gray[j]), 0
        except Exception:
            pass
    for kind, ks in any_shape.items():
        try:
            planes, status = getattr(reader, _PAGES_CALL[kind])([b.host[k][1] for k in ks])
            for j, k in enumerate(ks):
                if status[j] == 0:
                    dev[k], b.status[k] = planes[j], 0
        except Exception:
            pass
    return dev


def _mixed_read_page(reader, b, k, kw):
    kind, a, g = b.host[k]
    sub = KINDS[kind].stack(b.ids[k:k + 1], [(a, g)])
    return KINDS[kind].read_page(reader, sub, 0, kw)


# pages of any kind and shape in one batch (``mixed=True``): ONE ``readtext_pages`` call reads the pages that reached the card; the retry
# unit is the page, read as its own kind reads it
KINDS["mixed"] = Kind(stack=_mixed_stack, to_device=_mixed_to_device,
                      read=lambda r, b, kw: r.readtext_pages([b.dev[k] for k, s in enumerate(b.status) if s == 0], **kw),
                      read_host=None, read_page=_mixed_read_page)


def _page_key(kind, a):
    """Grouping key of a decoded page: every kind's first element carries the page's shape (a ``JpegPage``: that of its decode)"""
    return kind, tuple(a.shape)


def _read_batch(reader, batch, kw):
    """``{index: result}`` of a batch: one call for its pages of status 0, on the device payload, then (where the kind can) on the host
    payload; when that fails, and for a page of another status, page by page -- the reference loses ONE page when its OCR fails
    (enhanced_extractor.py:529-531), and that page maps to ``[]``."""
    kind = KINDS[batch.kind]
    status = batch.status or [0] * len(batch.ids)
    good = [k for k, s in enumerate(status) if s == 0]
    res = {}
    attempts = [kind.read] if batch.dev is not None and good else []
    if kind.read_host is not None:
        attempts.append(kind.read_host)
    for read in attempts:
        try:
            res = dict(zip(good, read(reader, batch, kw)))
            break
        except Exception:
            pass
    for k in range(len(batch.ids)):
        if k not in res:
            try:
                res[k] = kind.read_page(reader, batch, k, kw)
            except Exception:
                res[k] = []
    return {batch.ids[k]: r for k, r in res.items()}


def _default_decode_workers(reader, n_files):
    """half of the process's CPU share (affinity mask and cgroup quota, bbocr_host_cpu_share), at most 8: the library's own host pool, the
    upload stage and the two device-call threads need the rest (16-CPU share: 4 threads 700-780 pages/s, 8: 720-790, 16: 755-825)"""
    try:
        share = int(reader._lib.bbocr_host_cpu_share())
    except Exception:
        share = os.cpu_count() or 1
    return max(1, min(8, share // 2, n_files))


def _assemble(decode_one, idxs, max_batch, decode_workers, batches, mixed=False):
    """Assembler thread: decode pool -> groups of one kind and shape -> ``batches`` (a full group travels as one ``Batch``; None ends it).
    ``mixed``: ONE group for every kind and shape, closed by page count and by the pixel budget (``reader.mixed_pixel_budget``).
    Back-pressure end to end: at most `window` decoded pages exist outside the two assembled batches the queue may hold (a decode is only
    submitted once a slot is free, and a slot is released when its page has been copied into a batch), so the resident set is bounded by
    ~4 batches however many files are queued."""
    window = max(2 * max_batch, 2 * decode_workers)
    slots = threading.Semaphore(window)
    groups = {}
    open_px = 0                                                 # mixed: pixels of the pages in the one open group
    if mixed:
        from .reader import mixed_pixel_budget

        budget = mixed_pixel_budget()

    def flush(key):
        nonlocal open_px
        group = groups.pop(key)
        if key == ("mixed",):
            open_px = 0
        batches.put(KINDS[key[0]].stack([i for i, _ in group], [page for _, page in group]))
        for _ in group:
            slots.release()

    try:
        with ThreadPoolExecutor(max_workers=decode_workers) as pool:
            pending = collections.deque()
            it = iter(idxs)
            done_submitting = False
            while pending or not done_submitting:
                while not done_submitting and len(pending) < window and slots.acquire(blocking=not pending):
                    i = next(it, None)
                    if i is None:
                        slots.release()
                        done_submitting = True
                        break
                    pending.append((i, pool.submit(decode_one, i)))
                if not pending:
                    continue
                i, fut = pending.popleft()
                page = fut.result()
                del fut                                         # the future would keep the decoded arrays alive
                if page is None or page[0] not in KINDS:
                    slots.release()
                    continue
                kind, a, b = page                               # the decode callback's tuple ends here
                if mixed:
                    key = ("mixed",)
                    px = a.shape[0] * a.shape[1]
                    if key in groups and open_px + px > budget:
                        flush(key)                              # the page would overrun the pixel budget: it opens the next batch
                    groups.setdefault(key, []).append((i, page))
                    open_px += px
                else:
                    key = _page_key(kind, a)
                    groups.setdefault(key, []).append((i, (a, b)))
                if len(groups[key]) >= max_batch:
                    flush(key)
                elif not pending and not done_submitting:
                    # nothing is being decoded: the next submission needs a slot.  If every slot is held by pages waiting in partial
                    # groups (many distinct shapes), send the largest group -- only then: while decodes are pending their pages hold
                    # slots too, and flushing on that account cut full batches into single pages (round 3: the faster the decode
                    # pool, the smaller the device batches)
                    if slots.acquire(blocking=False):
                        slots.release()
                    else:
                        flush(max(groups, key=lambda k: len(groups[k])))
            for key in list(groups):
                flush(key)
    finally:
        batches.put(None)


def _upload(reader, batch):
    """Stage between the assembler and the device calls: the batch's pages reach the card (one GIL-free C call on the context's upload
    stream, outside the call slots) while both device workers are still inside their calls -- a worker that uploaded its own batch left
    the card idle for that long, and the two workers fell into step.  Readers without the upload entry (test doubles) and a failed upload
    leave the batch without a device payload: the device worker reads it from the host pages and reports per page."""
    try:
        batch.dev = KINDS[batch.kind].to_device(reader, batch)
    except Exception:
        pass
    return batch


def _device_stage(reader, batches, texts, kw):
    """This thread is the upload stage, one batch ahead of the device workers; two device batches in flight on the one Reader
    (bbocr_config::call_slots, the reference's own ThreadPoolExecutor contract, batch_processor_enhanced.py:215): the H2D copy and
    detector of batch k+1 run while batch k's host thread finishes its boxes and strings."""
    in_flight = threading.Semaphore(2)
    with ThreadPoolExecutor(max_workers=2, thread_name_prefix="bbocr-ocr") as device_pool:
        futs = []
        while True:
            batch = batches.get()
            if batch is None:
                break
            batch = _upload(reader, batch)
            in_flight.acquire()
            fut = device_pool.submit(lambda b: texts.update(_read_batch(reader, b, kw)), batch)
            fut.add_done_callback(lambda _f: in_flight.release())
            futs.append(fut)
            del batch
        for fut in futs:
            fut.result()


def read_files(reader, image_paths, indices=None, max_batch=64, decode_workers=None, decode=None, device_decode=False, mixed=None,
               png_decode=None, tiff_decode=None, gif_decode=None, bmp_decode=None, **readtext_kw):
    """``{index: readtext result}`` for the files ``image_paths[i]``, i in ``indices`` (default: all): the result lists
    ``Reader.readtext(path)`` returns page by page, from 64-page device batches.  A page whose decode or OCR fails maps to ``[]``.

    Decoding (and the thumbnail + JPEG round trip) is what bounds the application once the OCR itself runs at hundreds of pages
    per second: a 1280x960 JPEG costs ~9 ms of one core decoded twice (RGB and the Y plane), ~4.6 ms decoded once into YCbCr triples
    (reader.decode_file_ycc: both planes are then derived on the card).  The files are therefore decoded by ``decode_workers`` threads (default:
    the host's cores, at most 16; PIL releases the GIL while decoding) and a shape group is sent to the device as soon as it is
    full, so the decode of later pages overlaps the device batch of earlier ones (ctypes releases the GIL during the C call).
    ``decode(path, index)`` returns ``("ycc", triples, None)``, ``("rgb", rgb, gray)``, ``("dev", rgb_dev, gray_dev)`` or
    ``("jpg", JpegPage, None)``.  ``device_decode=True`` (or a ``decode`` that returns ``"jpg"`` pages): baseline JPEG files are only read
    and planned here and travel as their bytes, grouped by decoded shape; the upload stage decodes a group on the card with one call,
    straight into the batch tensor (``device_decode="chroma"``: 4:4:4, 4:2:2 and 4:4:0 files too).  Three overlapped stages: decode pool -> assembler thread (``_assemble``) -> this thread
    (``_device_stage``: upload, two device calls in flight, result strings); what they hand on is a ``Batch`` of one of the ``KINDS``.
    ``mixed`` (None: the environment variable ``BBOCR_MIXED_BATCH``, off unless ``1``): batches are closed by page count
    (``max_batch``, at most ``BBOCR_MAX_DEVICE_BATCH``) and a pixel budget instead of by shape, pages of all four kinds travel together, and each
    batch is read by one ``Reader.readtext_pages`` call; same results, same failure rule.
    ``png_decode`` (None: the Reader's ``png_decode``, off by default): PNG files the device decoder takes (``reader.png_plan``) travel as
    their bytes too, kind ``"png"``, and a group is decoded by one ``bbocr_png_decode`` call (csrc/pngdec.hip, identical pixels); a file
    the plan refuses (Adam7, 16 bit, APNG, ...) or whose data turns out damaged takes the host decode as before.
    ``tiff_decode`` (None: the Reader's ``tiff_decode``, off by default): likewise TIFF files the device decoder takes (``reader.tiff_plan``:
    strips of raw, PackBits, LZW or Deflate data), kind ``"tiff"``, a group decoded by one ``bbocr_tiff_decode`` call (csrc/tiffdec.hip,
    identical pixels) -- with ``mixed`` the TIFF pages of a batch share one call whatever their shapes; a file the plan refuses (tiles,
    CCITT, 16 bit, ...) or whose data turns out damaged takes the host decode as before.  ``tiff_decode="fax"``: CCITT files (compression 2,
    3, 4: ``reader.tiff_fax_plan``) are taken as well, and a call that holds one goes to ``bbocr_tiff_decode_fax`` (csrc/tiff_fax.h).
    ``gif_decode`` (None: the Reader's ``gif_decode``, off by default): likewise GIF files (``reader.gif_plan``), kind ``"gif"``: the group --
    with ``mixed`` every GIF page of the batch, whatever its shape -- is decoded by one ``bbocr_gif_decode`` call (csrc/gifdec.hip, identical
    pixels); a file the plan refuses or whose code stream turns out damaged takes the host decode as before.
    ``bmp_decode`` (None: the Reader's ``bmp_decode``, off by default): likewise BMP files (``reader.bmp_plan``), kind ``"bmp"``, one
    ``bbocr_bmp_decode`` call -- one launch -- per group (csrc/bmpdec.hip, identical pixels); a file the plan refuses (RLE, ...) takes the
    host decode as before."""
    from .reader import mixed_batch_enabled

    mixed = mixed_batch_enabled(mixed)
    png_decode = bool(getattr(reader, "png_decode", False)) if png_decode is None else bool(png_decode)
    tiff_decode = _tiff_level(reader, tiff_decode)
    gif_decode = bool(getattr(reader, "gif_decode", False)) if gif_decode is None else bool(gif_decode)
    bmp_decode = bool(getattr(reader, "bmp_decode", False)) if bmp_decode is None else bool(bmp_decode)
    if mixed:
        max_batch = max(1, min(max_batch, int(os.environ.get("BBOCR_MAX_DEVICE_BATCH", "64"))))
    if decode is None:
        on_device = device_decode or png_decode or tiff_decode or gif_decode or bmp_decode
        decode = ((lambda path, i: _plain_input_device(path, i, device_decode, png_decode, tiff_decode, gif_decode, bmp_decode)) if on_device
                  else _plain_input)
    if indices is None:
        indices = range(len(image_paths))
    idxs = [i for i in indices if 0 <= i < len(image_paths)]
    texts = {i: [] for i in idxs}
    if not idxs:
        return texts
    if decode_workers is None:
        decode_workers = _default_decode_workers(reader, len(idxs))

    def decode_one(i):
        try:
            return decode(image_paths[i], i)
        except Exception:
            return None

    batches = queue.Queue(maxsize=2)
    worker = threading.Thread(target=_assemble, args=(decode_one, idxs, max_batch, decode_workers, batches, mixed), daemon=True)
    worker.start()
    _device_stage(reader, batches, texts, readtext_kw)
    worker.join()
    return texts


# ------------------------------------------------------------------------------------------------ the model input (:763-813)
def _model_image_plain(reader, path, max_dim, quality, device_decode):
    """``_encode_image_for_model`` of the file itself: ``Image.open`` does not transpose, and carries the file's comment into the JPEG it
    saves.  The pixels reach the card as the file's bytes (``device_decode`` and the device decoder takes them) or as Pillow's RGB decode;
    a file the device decoder refuses or reports damaged takes ``model_image_host``."""
    from PIL import Image

    from .preprocess import PAGE_GRAY, PAGE_RGB, PAGE_YCBCR4, model_image_device, model_image_host

    if device_decode:
        page = _jpg_page(path, device_decode)
        if page is not None:
            comment = Image.open(path).info.get("comment")                # headers only
            dev, status = reader.decode_jpeg_batch([page[1]], padded=True)
            if status[0] == 0:
                return model_image_device(reader, dev[0], PAGE_GRAY if dev.ndim == 3 else PAGE_YCBCR4, max_dim, quality, comment)
        return model_image_host(path, max_dim, quality)
    img = Image.open(path)
    rgb = np.asarray(img.convert("RGB"))
    return model_image_device(reader, reader._to_dev(rgb), PAGE_RGB, max_dim, quality, img.info.get("comment"))


def encode_images_for_model(reader, image_paths, use_preprocessing=False, edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128,
                            device_decode=False, rule=None):
    """The base64 strings the extractor sends to the vision model (enhanced_extractor.py:763-813), one per image, string for string: the
    preprocess -> edge-crop -> auto-crop chain of the OCR input (``ocr_page_crop``, on the card), then ``_encode_image_for_model``
    (:399-411) with ``rule(i) -> (max_dim, quality)`` (default ``preprocess.model_image_rule``: 2000 / 88 for image 0, 3200 / 95 for the
    others; the quality is clamped to 50 .. 95) -- thumbnail and JPEG encoder on the card as well (``preprocess.model_image_device``:
    csrc/thumb.hip + csrc/jpegenc.hip), so that only the file's bytes cross the link.  Where the chain changes the page the reference reads
    it through ``cv2.imread`` (EXIF orientation applied; the PNG it writes carries no comment); where no step applies it encodes the
    original file, which ``Image.open`` does not transpose and whose comment the saved JPEG keeps.  ``device_decode=True``: baseline JPEG
    files are decoded on the card too (``"chroma"``: 4:4:4, 4:2:2 and 4:4:0 files among them).  A file Pillow cannot read maps to the base64 of its bytes, like :409-411."""
    import base64

    from .preprocess import PAGE_BGR, PAGE_GRAY, model_image_device, model_image_quality, model_image_rule

    if crop_margin < 0:
        raise ValueError("crop_margin must be >= 0")
    rule = rule or model_image_rule
    out = []
    for i, path in enumerate(image_paths):
        max_dim, quality = rule(i)
        quality = model_image_quality(quality)
        data = None
        if use_preprocessing or edge_crop_percent > 0.0 or crop_for_ocr:
            applied = []
            try:
                page = ocr_page_crop(reader, path, use_preprocessing, edge_crop_percent, crop_for_ocr, crop_margin, on_device=True,
                                     device_decode=device_decode, applied=applied)
            except (OSError, ValueError):
                applied = []                                          # :778-797: a step that fails leaves the original file
            if applied:
                data = model_image_device(reader, page, PAGE_GRAY if page.ndim == 2 else PAGE_BGR, max_dim, quality)
        if data is None:
            try:
                data = _model_image_plain(reader, path, max_dim, quality, device_decode)
            except OSError:                                           # Pillow cannot read the file
                with open(path, "rb") as f:
                    data = f.read()
        out.append(base64.b64encode(data).decode("utf-8"))
    return out


# ------------------------------------------------------------------------------------------------ the processing trace's previews (:184-199)
TRACE_KEYS = {"preprocess": "preprocessed_b64", "edge_crop": "edge_cropped_b64", "auto_crop": "auto_cropped_b64"}


def trace_previews(reader, image_paths, use_preprocessing=False, edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128, device_decode=True,
                   png=None):
    """The preview strings ``extract_text_with_ocr`` puts into an image's trace (``capture_trace=True``, :421-476), one dict per image,
    string for string: ``original_b64`` -- ``_image_to_data_url`` of the file itself (``Image.open`` does not transpose; an unloaded JPEG
    is decoded at the draft scale) -- and, where the step changed the page, ``preprocessed_b64``, ``edge_cropped_b64`` and
    ``auto_cropped_b64`` of the PNG the reference wrote after it; a key is absent where its step is off or returns None in the
    reference.  The pages are those of ``ocr_page_crop`` (pre-processed once, crops as views) thumbnailed on the card
    (``preprocess.preview_device``): only pages of at most 800 pixels come back.  ``device_decode``: baseline 4:2:0 / grey JPEG files --
    ``"chroma"``: 4:4:4, 4:2:2 and 4:4:0 files as well -- are decoded on the card; everything else takes ``preprocess.preview_host``.  A
    file the decoder takes is read once and, with a crop setting on, decoded ONCE (``Reader.decode_jpeg_scales_batch``): one run of the
    entropy stages yields the decode at the draft scale for the original's preview and ``cv2.imread``'s full-scale page the crop chain
    starts from; when the draft scale is 1 the two are one decode, oriented on the card.  ``png="device"`` (opt-in; default
    ``preprocess.png_writer()``): the PNG files of the previews made on the card are written there too (``Reader.encode_png``) -- the strings
    are then not the reference's, but each decodes to the same image (mode, size, pixels, ICC profile)."""
    from .preprocess import png_writer, preview_device
    from .reader import _file_bytes

    if crop_margin < 0:
        raise ValueError("crop_margin must be >= 0")
    chain = use_preprocessing or edge_crop_percent > 0.0 or crop_for_ocr
    png = png_writer(png)
    out = []
    for path in image_paths:
        source = _file_bytes(path) if device_decode else path             # read once
        once = _trace_decode_once(reader, source, device_decode, png) if device_decode and chain else None
        trace = {"original_b64": once[0] if once else preview_device(reader, source, device_decode=device_decode, png=png)}
        if chain:
            pages = {}
            ocr_page_crop(reader, source, use_preprocessing, edge_crop_percent, crop_for_ocr, crop_margin, on_device=True,
                          device_decode=device_decode, pages=pages, page=once[1] if once else None)
            for step, page in pages.items():
                trace[TRACE_KEYS[step]] = preview_device(reader, page, png=png)
        out.append(trace)
    return out


def _trace_decode_once(reader, data, device_decode, png="pillow"):
    """Both uses of a traced file from one run of the entropy stages: ``(original_b64, cv2.imread's page on the card)``, or None for a
    file the device decoder does not take or whose entropy-coded data it reports damaged (the caller keeps its two-step path)."""
    import io

    from PIL import Image

    from .preprocess import PAGE_GRAY, PAGE_YCBCR4, PREVIEW_MAX_DIM, _preview_of_decode, _preview_string, orient_page_device, preview_draft_scale
    from .reader import JpegPage, jpeg_chroma, jpeg_device_plan, jpeg_progressive

    plan = jpeg_device_plan(data, jpeg_chroma(device_decode), jpeg_progressive(device_decode))
    if plan is None:
        return None
    s = preview_draft_scale(plan, PREVIEW_MAX_DIM)
    decodes, status = reader.decode_jpeg_scales_batch([JpegPage(data, plan)], (1,) if s == 1 else (1, s), imread=s != 1)
    if status[0] != 0:
        return None
    drafted = decodes[0][s]
    if s == 1:                                                            # one decode: the un-oriented pixels, oriented for the crop chain
        page = orient_page_device(reader, drafted, PAGE_GRAY if drafted.ndim == 2 else PAGE_YCBCR4, int(plan.orientation))
    else:
        page = decodes[0][1]
    icc = Image.open(io.BytesIO(data)).info.get("icc_profile")              # headers only
    return _preview_string(_preview_of_decode(reader, drafted, plan, s, PREVIEW_MAX_DIM), icc, reader, png), page
