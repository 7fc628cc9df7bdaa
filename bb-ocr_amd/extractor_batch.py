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

import io
import os

import numpy as np


def _jpg_page(source):
    """``("jpg", JpegPage, None)`` when the device decoder takes the file (a path or its bytes), else None"""
    from .reader import jpeg_page

    page = jpeg_page(source)
    return None if page is None else ("jpg", page, None)


def _ocr_input(image_path, image_index=None, decode_once=True, device_decode=False):
    """``ocr_input_image`` for the batching loop: ``("ycc", triples, None)`` when the file easyocr would be given is a YCbCr-coded JPEG
    (decoded once, RGB + Y plane derived on the card: reader.decode_file_ycc) -- every thumbnail is, it is written as one -- else
    ``("rgb", rgb, gray)``.  ``device_decode``: the file easyocr would be given travels as its bytes (``("jpg", JpegPage, None)``) when the
    device decoder takes it -- the original at or below the limit (only its header is read here), or the thumbnail as written."""
    from PIL import Image

    from .reader import decode_file, decode_file_ycc, reformat_input

    cover = image_index is None or image_index == 0
    max_dim = 1600 if cover else 2400
    try:
        img = Image.open(image_path)
        if max(img.size) > max_dim:
            img = img.convert("RGB")
            img.thumbnail((max_dim, max_dim))
            buf = io.BytesIO()
            img.save(buf, format="JPEG", quality=(90 if cover else 95))
            data = buf.getvalue()
            page = _jpg_page(data) if device_decode else None
            if page is not None:
                return page
            ycc = decode_file_ycc(data, padded=True) if decode_once else None
            return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(decode_file(data))
    except Exception:
        pass                                                      # :511-514: any failure falls back to the original file
    page = _jpg_page(image_path) if device_decode else None
    if page is not None:
        return page
    ycc = decode_file_ycc(os.fspath(image_path), padded=True) if decode_once else None
    return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(reformat_input(os.fspath(image_path)))


def _ocr_input_array(page, image_index=None, decode_once=True):
    """``_ocr_input`` for a page the reference would have written as a PNG (its pre-processed / cropped file): gray [H,W] or BGR
    [H,W,3] uint8.  Gray pages are read back as three equal channels, so the RGB thumbnail is the gray one replicated."""
    from PIL import Image

    from .reader import decode_file, decode_file_ycc

    cover = image_index is None or image_index == 0
    max_dim = 1600 if cover else 2400
    rgb = np.ascontiguousarray(np.repeat(page[:, :, None], 3, axis=2) if page.ndim == 2 else page[:, :, ::-1])
    if max(page.shape[0], page.shape[1]) > max_dim:
        img = Image.fromarray(rgb)
        img.thumbnail((max_dim, max_dim))
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=(90 if cover else 95))
        data = buf.getvalue()
        ycc = decode_file_ycc(data, padded=True) if decode_once else None
        return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(decode_file(data))
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
    page = _jpg_page(image_path) if device_decode else None
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


def ocr_page_crop(reader, image_path, use_preprocessing=False, edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128, on_device=False):
    """The page ``extract_text_with_ocr`` would hand to the down-scaling step (:425-485), as a host array: decoded like ``cv2.imread``
    (BGR, EXIF-transposed), uploaded, pre-processed on the card (gray), edge-cropped (a view) and auto-cropped on the card; only the
    final crop comes back.  A step that returns None in the reference leaves the page as it was.  ``on_device=True``: the crop stays on
    the card, as a (possibly strided) view of the device page."""
    from .preprocess import _imread_bgr, auto_crop_box_device, central_edge_crop_box, preprocess_bgr_device

    page = reader._to_dev(_imread_bgr(image_path))
    if use_preprocessing:
        page = preprocess_bgr_device(reader, page)
    if edge_crop_percent > 0.0:
        b = central_edge_crop_box(page.shape[0], page.shape[1], edge_crop_percent)
        if b is not None:
            page = page[b[1]:b[3], b[0]:b[2]]
    if crop_for_ocr:
        b = auto_crop_box_device(reader, page, crop_margin)
        if b is not None:
            page = page[b[1]:b[3], b[0]:b[2]]
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

    cover = image_index is None or image_index == 0
    max_dim = 1600 if cover else 2400
    try:
        img = Image.open(image_path)
        if max(img.size) > max_dim:
            img = img.convert("RGB")
            img.thumbnail((max_dim, max_dim))
            buf = io.BytesIO()
            img.save(buf, format="JPEG", quality=(90 if cover else 95))
            return decode_file(buf.getvalue())                    # what easyocr's loader sees: a JPEG file on disk
    except Exception:
        pass                                                      # :511-514: any failure falls back to the original file
    return reformat_input(os.fspath(image_path))


def extract_texts(reader, image_paths, ocr_image_indices=None, max_batch=64, decode_workers=None, decode_once=True, use_preprocessing=False,
                  edge_crop_percent=0.0, crop_for_ocr=False, crop_margin=128, device_thumbnail=False, device_decode=False, **readtext_kw):
    """``{index: text}`` for every index of ``ocr_image_indices`` (default: all pages), text = ``" ".join(r[1] for r in results)``
    exactly as :521; a page whose OCR fails gets ``""`` like :529-531.  Pages of equal (down-scaled) shape travel in one device
    batch of at most ``max_batch`` pages (``read_files`` with the reference's OCR-input rule as the decode step).
    ``use_preprocessing`` / ``edge_crop_percent`` / ``crop_for_ocr`` / ``crop_margin``: the extractor's settings of the same names
    (``ocr_page_crop``); with all of them off the pages are read as before.  ``device_thumbnail=True``: the down-scaling + JPEG round trip
    of :486-512 runs on the card (csrc/thumb.hip, identical pixels): a cropped page stays on the card from upload to OCR, and a
    YCbCr-coded JPEG above the limit is uploaded as decoded and shrunk there.  ``device_decode=True``: the decode step only reads the file
    and plans it (``bbocr_host_jpeg_plan``); baseline JPEG files -- the thumbnails included -- reach the card as their bytes and are
    decoded there, a whole batch by one call (csrc/jpegdec.hip, identical pixels); every other file, and a file whose data turns out
    damaged, takes the host decode as before.  (The crop settings read the page like ``cv2.imread`` and keep their host decode.)"""
    from .preprocess import ocr_input_device

    if use_preprocessing or edge_crop_percent > 0.0 or crop_for_ocr:
        if crop_margin < 0:
            raise ValueError("crop_margin must be >= 0")

        def decode(path, i):
            page = ocr_page_crop(reader, path, use_preprocessing, edge_crop_percent, crop_for_ocr, crop_margin, on_device=device_thumbnail)
            if device_thumbnail:
                return ("dev",) + tuple(ocr_input_device(reader, page, i))
            return _ocr_input_array(page, i, decode_once)
    elif device_thumbnail:
        decode = lambda path, i: _ocr_input_device(reader, path, i, decode_once, device_decode)
    else:
        decode = lambda path, i: _ocr_input(path, i, decode_once, device_decode)
    res = read_files(reader, image_paths, ocr_image_indices, max_batch, decode_workers, decode=decode, **readtext_kw)
    return {i: " ".join(t[1] for t in r) for i, r in res.items()}


def _plain_input(path, i=None):
    """Decode step of ``read_files`` without the extractor's thumbnail rule: what ``Reader.readtext(path)`` would hold."""
    from .reader import decode_file_ycc, reformat_input

    ycc = decode_file_ycc(os.fspath(path), padded=True)
    return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(reformat_input(os.fspath(path)))


def _plain_input_device(path, i=None):
    """``_plain_input`` with the device decoder: the file's bytes when it takes them"""
    return _jpg_page(path) or _plain_input(path, i)


def _host_input(page):
    """The host decode of a ``JpegPage`` (the retry of a page whose device decode failed): what ``_plain_input`` returns for its file"""
    from .reader import decode_file, decode_file_ycc

    ycc = decode_file_ycc(page.data, padded=True)
    return ("ycc", ycc, None) if ycc is not None else ("rgb",) + tuple(decode_file(page.data))


def read_files(reader, image_paths, indices=None, max_batch=64, decode_workers=None, decode=None, device_decode=False, **readtext_kw):
    """``{index: readtext result}`` for the files ``image_paths[i]``, i in ``indices`` (default: all): the result lists
    ``Reader.readtext(path)`` returns page by page, from 64-page device batches.  A page whose decode or OCR fails maps to ``[]``.

    Decoding (and the thumbnail + JPEG round trip) is what bounds the application once the OCR itself runs at hundreds of pages
    per second: a 1280x960 JPEG costs ~9 ms of one core decoded twice (RGB and the Y plane), ~4.6 ms decoded once into YCbCr triples
    (reader.decode_file_ycc: both planes are then derived on the card).  The files are therefore decoded by ``decode_workers`` threads (default:
    the host's cores, at most 16; PIL releases the GIL while decoding) and a shape group is sent to the device as soon as it is
    full, so the decode of later pages overlaps the device batch of earlier ones (ctypes releases the GIL during the C call).
    ``decode(path, index)`` returns ``("ycc", triples, None)`` or ``("rgb", rgb, gray)``.  ``device_decode=True`` (or a ``decode`` that
    returns ``("jpg", JpegPage, None)``): baseline JPEG files are only read and planned here and travel as their bytes, grouped by decoded
    shape; the upload stage decodes a group on the card with one call, straight into the batch tensor."""
    import collections
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor

    if decode is None:
        decode = _plain_input_device if device_decode else _plain_input
    if indices is None:
        indices = range(len(image_paths))
    idxs = [i for i in indices if 0 <= i < len(image_paths)]
    texts = {i: [] for i in idxs}
    if not idxs:
        return texts
    if decode_workers is None:
        # half of the process's CPU share (affinity mask and cgroup quota, bbocr_host_cpu_share), at most 8: the library's own host pool, the
        # upload stage and the two device-call threads need the rest (16-CPU share: 4 threads 700-780 pages/s, 8: 720-790, 16: 755-825)
        try:
            share = int(reader._lib.bbocr_host_cpu_share())
        except Exception:
            share = os.cpu_count() or 1
        decode_workers = max(1, min(8, share // 2, len(idxs)))

    # three overlapped stages: decode pool -> assembler thread (groups pages by shape, hands a full group on as one batch)
    # -> this thread (device call + result strings).  Back-pressure end to end: at most `window` decoded pages exist outside the two
    # assembled batches the queue may hold (a decode is only submitted once a slot is free, and a slot is released when its page has
    # been copied into a batch), so the resident set is bounded by ~4 batches however many files are queued.
    batches = queue.Queue(maxsize=2)
    window = max(2 * max_batch, 2 * decode_workers)
    slots = threading.Semaphore(window)

    def decode_one(i):
        try:
            return decode(image_paths[i], i)
        except Exception:
            return None

    def assemble():
        try:
            by_shape = {}

            def flush(group):
                if hasattr(group[0][1], "data") and isinstance(group[0][1].data, bytes):
                    batches.put(("jpg", [p[0] for p in group], [p[1] for p in group]))     # file bytes: decoded by the upload stage
                    for _ in group:
                        slots.release()
                    return
                if not isinstance(group[0][1], np.ndarray):
                    # "dev" pages (already in HBM): one concatenation on the card, nothing to upload
                    import torch

                    rgb, gray = torch.stack([p[1] for p in group]), torch.stack([p[2] for p in group])
                    torch.cuda.current_stream(rgb.device).synchronize()                       # the library runs on its own stream
                    batches.put(("dev", [p[0] for p in group], rgb, gray))
                    for _ in group:
                        slots.release()
                    return
                # pages travel as LISTS: the Reader uploads them one by one into the device batch (no 236-MB np.stack on this thread)
                gray = None if group[0][2] is None else [p[2] for p in group]                 # None: a group of once-decoded YCbCr pages
                batches.put(([p[0] for p in group], [p[1] for p in group], gray))
                for _ in group:
                    slots.release()

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
                    if page is None:
                        slots.release()
                        continue
                    kind, rgb, gray = page                          # kind "ycc": rgb holds the YCbCr triples, gray is None
                    key = (kind, tuple(rgb.shape))                  # kind "dev": device tensors (rgb, gray)
                    group = by_shape.setdefault(key, [])
                    group.append((i, rgb, gray))
                    if len(group) >= max_batch:
                        flush(by_shape.pop(key))
                    elif not pending and not done_submitting:
                        # nothing is being decoded: the next submission needs a slot.  If every slot is held by pages waiting in partial
                        # groups (many distinct shapes), send the largest group -- only then: while decodes are pending their pages hold
                        # slots too, and flushing on that account cut full batches into single pages (round 3: the faster the decode
                        # pool, the smaller the device batches)
                        if slots.acquire(blocking=False):
                            slots.release()
                        else:
                            big = max(by_shape, key=lambda k: len(by_shape[k]))
                            flush(by_shape.pop(big))
                for group in by_shape.values():
                    if group:
                        flush(group)
        finally:
            batches.put(None)

    def upload(item):
        """Stage between the assembler and the device calls: the batch's pages reach the card (one GIL-free C call on the context's upload
        stream, outside the call slots) while both device workers are still inside their calls -- a worker that uploaded its own batch left
        the card idle for that long, and the two workers fell into step.  Readers without the upload entry (test doubles) pass through."""
        if item[0] == "dev":
            return item
        if item[0] == "jpg":
            _, ids, pages = item
            try:
                # ONE decode call for the group, on the context's JPEG stream outside the call slots: it runs while both device workers
                # are inside their calls, like an upload
                batch, status = reader.decode_jpeg_batch(pages, padded=True)
                return "jpgdev", ids, pages, batch, status
            except Exception:
                return "jpgdev", ids, pages, None, [-1] * len(ids)       # the device worker decodes every page on the host
        ids, rgb, gray = item
        to_dev = getattr(reader, "_to_dev", None)
        if to_dev is None:
            return item
        try:
            return ids, to_dev(rgb), (to_dev(gray) if gray is not None else None), rgb, gray
        except Exception:
            return item                                  # the device worker retries from the host pages and reports per page

    def ocr_host_page(i, page):
        """the existing host path for one page of a "jpg" group"""
        try:
            kind, rgb, gray = _host_input(page)
            if kind == "ycc":
                texts[i] = reader.readtext_ycc_arrays([rgb], **readtext_kw)[0]
            else:
                texts[i] = reader.readtext_arrays([rgb], [gray], **readtext_kw)[0]
        except Exception:
            texts[i] = []

    def ocr(item):
        if item[0] == "jpgdev":
            _, ids, pages, batch, status = item
            good = [k for k in range(len(ids)) if status[k] == 0]
            if good:
                try:
                    if len(good) < len(ids):
                        batch = batch[good]
                    if batch.ndim == 4:
                        rgb_dev, gray_dev = reader.pages_from_ycc(batch)
                    else:                                # 1-component files: the samples, replicated for RGB
                        rgb_dev, gray_dev = batch[..., None].expand(-1, -1, -1, 3).contiguous(), batch
                    res = reader.readtext_device(rgb_dev, gray_dev, **readtext_kw)
                    for k, r in zip(good, res):
                        texts[ids[k]] = r
                except Exception:
                    good = []
            for k in range(len(ids)):
                if k not in good:
                    ocr_host_page(ids[k], pages[k])
            return
        if item[0] == "dev":                             # device pages: the page-by-page retry reads slices of the same tensors
            _, ids, rgb_dev, gray_dev = item
            try:
                res = reader.readtext_device(rgb_dev, gray_dev, **readtext_kw)
            except Exception:
                res = []
                for k in range(len(ids)):
                    try:
                        res.append(reader.readtext_device(rgb_dev[k:k + 1], gray_dev[k:k + 1], **readtext_kw)[0])
                    except Exception:
                        res.append([])
            for i, r in zip(ids, res):
                texts[i] = r
            return
        if len(item) == 5:                               # uploaded: device tensors + the host pages for the page-by-page retry
            ids, rgb_dev, gray_dev, rgb, gray = item
            try:
                if gray is None:
                    res = reader.readtext_device(*reader.pages_from_ycc(rgb_dev), **readtext_kw)
                else:
                    res = reader.readtext_device(rgb_dev, gray_dev, **readtext_kw)
                for i, r in zip(ids, res):
                    texts[i] = r
                return
            except Exception:
                pass
            del rgb_dev, gray_dev
        else:
            ids, rgb, gray = item
        read = (lambda a, g: reader.readtext_ycc_arrays(a, **readtext_kw)) if gray is None else (lambda a, g: reader.readtext_arrays(a, g, **readtext_kw))
        try:
            res = read(rgb, gray)
        except Exception:
            # the reference loses ONE page when its OCR fails (enhanced_extractor.py:529-531): retry the batch page by page
            res = []
            for k in range(len(ids)):
                try:
                    res.append(read(rgb[k:k + 1], None if gray is None else gray[k:k + 1])[0])
                except Exception:
                    res.append([])
        for i, r in zip(ids, res):
            texts[i] = r

    worker = threading.Thread(target=assemble, daemon=True)
    worker.start()
    # two device batches in flight on the one Reader (bbocr_config::call_slots, the reference's own ThreadPoolExecutor contract,
    # batch_processor_enhanced.py:215): the H2D copy and detector of batch k+1 run while batch k's host thread finishes its boxes and strings
    in_flight = threading.Semaphore(2)
    with ThreadPoolExecutor(max_workers=2, thread_name_prefix="bbocr-ocr") as device_pool:
        futs = []
        while True:
            item = batches.get()
            if item is None:
                break
            item = upload(item)                          # this thread is the upload stage: it runs one batch ahead of the device workers
            in_flight.acquire()
            fut = device_pool.submit(ocr, item)
            fut.add_done_callback(lambda _f: in_flight.release())
            futs.append(fut)
            del item
        for fut in futs:
            fut.result()
    worker.join()
    return texts
