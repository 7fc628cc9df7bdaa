"""``Reader``: the host-side mirror of ``easyocr.Reader`` for the one path BB-OCR uses.

Reference call sites this class stands in for (same names, argument meaning, return
shape and error behaviour):
  * ``easyocr.Reader(["en"], gpu=use_gpu)``        pipeline_demo/extractor/enhanced_extractor.py:153
  * ``reader.readtext(path, paragraph=False, batch_size=1, workers=0)``          ...:520
    consumed as ``" ".join(result[1] for result in results)`` (:521), any exception is
    caught by the caller and turns into empty text (:529-531)
  * ``for (bbox, text, prob) in reader.readtext(path)``   pipeline_components/img_to_json/
    ocr_testing/ocr_engines/test_easyocr.py:23,50
Upstream semantics followed: easyocr==1.7.2 ``easyocr/easyocr.py::Reader.{__init__,detect,
recognize,readtext,readtext_batched}``.

Everything numeric happens in libbbocr.so (HIP kernels) through the C ABI in
``include/bbocr.h``; torch is used only to hold device memory.  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
import io
import os
import threading

import numpy as np

from . import _lib
from . import weights as _weights

# english_g2 character list (easyocr/config.py); index 0 of the class axis is the CTC blank
_SYMBOLS = "0123456789!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ €"
CHARSET = _SYMBOLS + "ABCDEFGHIJKLMNOPQRSTUVWXYZ" + "abcdefghijklmnopqrstuvwxyz"
CHARACTER = ["[blank]"] + list(CHARSET)
# byte per class index (the CTC blank never reaches the decoded text): lets _collect build all texts with ONE latin-1 decode (a memcpy-grade
# operation; the utf-32 decode it replaces cost 0.45 ms per 100 k characters).  The one non-latin-1 character of the english_g2 charset,
# the euro sign, travels as byte 0x80 and is put back afterwards.
_EURO_BYTE = 0x80
_CLASS_BYTES = np.array([ord("?")] + [(_EURO_BYTE if c == "\u20ac" else ord(c)) for c in CHARSET], dtype=np.uint8)
assert all(ord(c) < 0x80 or c == "\u20ac" for c in CHARSET)

_DET_KW = ("min_size", "text_threshold", "low_text", "link_threshold", "canvas_size", "mag_ratio", "slope_ths", "ycenter_ths",
           "height_ths", "width_ths", "add_margin")


def _gray_bgr2gray(a: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(a, COLOR_BGR2GRAY) on the channels as given: OpenCV 4's 15-bit fixed point (R 9798, G 19235, B 3735,
    round to nearest) -- pinned by the reference's stored pre-processing outputs (tests/golden/legacy_preprocess)."""
    a = a.astype(np.int32)
    return ((a[..., 2] * 9798 + a[..., 1] * 19235 + a[..., 0] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


_DECODE_POOL = None


def _decode_pool():
    global _DECODE_POOL
    if _DECODE_POOL is None:
        from concurrent.futures import ThreadPoolExecutor

        _DECODE_POOL = ThreadPoolExecutor(max_workers=4, thread_name_prefix="bbocr-decode")     # helpers of concurrent single-page callers
    return _DECODE_POOL


def _file_bytes(source):
    """The bytes of a file given as a path or as its bytes"""
    if isinstance(source, (bytes, bytearray)):
        return bytes(source)
    with open(os.path.expanduser(os.fspath(source)), "rb") as f:
        return f.read()


def _open_image(source):
    """``PIL.Image.open`` of a path or of a file's bytes"""
    from PIL import Image

    return Image.open(io.BytesIO(source)) if isinstance(source, (bytes, bytearray)) else Image.open(os.path.expanduser(str(source)))


def decode_file(source, parallel=False):
    """What upstream's path branch holds after ``cv2.imread(path, IMREAD_GRAYSCALE)`` + ``loadImage(path)`` (skimage -> RGB):
    ``(rgb uint8 HWC, gray uint8 HW)``.  ONE stated rule for the gray plane, by container:
      * JPEG: libjpeg decodes straight to its Y plane (``out_color_space = JCS_GRAYSCALE``) -- PIL's ``draft('L')`` asks
        libjpeg for exactly that, so no RGB -> gray formula is involved;
      * single-channel files (PNG/TIFF/... mode L, 1): the stored samples;
      * every other colour file (OpenCV's PNG reader: ``png_set_rgb_to_gray(1, 0.299, 0.587)``): libpng's truncating
        15-bit sum ``(9797 R + 19234 G + 3737 B) >> 15``, grey pixels unchanged.
    ``source`` is a path or a bytes object holding the file."""
    pil = _open_image(source)
    if pil.format in ("JPEG", "MPO") and pil.mode in ("RGB", "YCbCr"):
        # two libjpeg passes over the same file (RGB, and the Y plane alone).  `parallel` (the single-page call Reader.readtext(path),
        # the reference's own pattern): side by side on two threads -- PIL releases the GIL while it decodes, so the page costs one decode
        # time instead of two (8.9 -> 4.9 ms for 1280x960).  Callers that already decode on a thread pool (extractor_batch) keep it serial.
        def _y_plane():
            y = _open_image(source)
            y.draft("L", y.size)
            return np.ascontiguousarray(y.convert("L"))

        fut = _decode_pool().submit(_y_plane) if parallel else None
        rgb = np.ascontiguousarray(pil.convert("RGB"))
        grey = fut.result() if fut is not None else _y_plane()
        if grey.shape != rgb.shape[:2]:                      # draft() may not scale; keep the rule total
            grey = np.ascontiguousarray(pil.convert("L"))
        return rgb, grey
    rgb = np.ascontiguousarray(pil.convert("RGB"))
    if pil.mode in ("L", "1"):
        return rgb, np.ascontiguousarray(pil.convert("L"))
    a = rgb.astype(np.int32)
    return rgb, ((a[..., 0] * 9797 + a[..., 1] * 19234 + a[..., 2] * 3737) >> 15).astype(np.uint8)


def _pil_pixels_zero_copy(pil):
    """``uint8 [H,W,4]`` view of a loaded 3-band PIL image's own storage (4 bytes per pixel), or None when this Pillow / pyarrow cannot
    export it (older Pillow, image held in several memory blocks, pyarrow absent).  The view keeps the image alive."""
    try:
        import pyarrow as pa

        pil.load()
        arr = pa.array(pil)                                          # Image.__arrow_c_array__: fixed_size_list<uint8>[4], no copy
        v = arr.values.to_numpy(zero_copy_only=True)
        W, H = pil.size
        return v.reshape(H, W, 4) if v.size == H * W * 4 and v.dtype == np.uint8 else None
    except Exception:
        return None


def decode_file_ycc(source, padded=False):
    """A YCbCr-coded JPEG (JFIF, or Adobe marker with transform 1) decoded ONCE into libjpeg's YCbCr triples, ``uint8 [H,W,3]``; ``None``
    for every other file (callers fall back to ``decode_file``).  The two planes upstream's path branch reads are both functions of this
    one decode: the Y channel is ``cv2.imread(path, IMREAD_GRAYSCALE)``'s plane, and the RGB image is libjpeg's pointwise
    ``ycc_rgb_convert`` of the triple, which the device applies (``bbocr_op_ycc_to_rgb``) -- half the host's decode work of
    ``decode_file`` (8.9 -> 4.6 ms of one core for a 1280x960 page) and no second pass over the file.  ``source``: path or bytes.

    ``padded=True`` (decode pools): the result may be ``uint8 [H,W,4]`` -- Pillow's own pixel storage (Y Cb Cr x), exported without a copy
    through the Arrow C data interface (Pillow >= 11.2 + pyarrow) -- instead of the tight ``[H,W,3]`` that ``tobytes`` assembles while holding
    the interpreter lock (1.3 ms per page: with eight decode threads that serialised copy was what bounded the pool)."""
    try:
        pil = _open_image(source)
        if pil.format not in ("JPEG", "MPO") or pil.mode != "RGB":
            return None                                              # greyscale / CMYK / YCCK files and other containers
        if "jfif" not in pil.info and pil.info.get("adobe_transform") != 1:
            return None                                              # may be RGB-coded (libjpeg guesses from the component ids): not taken
        size = pil.size
        pil.draft("YCbCr", size)
        if pil.mode != "YCbCr" or pil.size != size:
            return None
        if padded:
            v = _pil_pixels_zero_copy(pil)
            if v is not None:
                return v
        ycc = np.asarray(pil)
        if ycc.ndim != 3 or ycc.shape[2] != 3 or ycc.dtype != np.uint8:
            return None
        return np.ascontiguousarray(ycc)
    except Exception:
        return None


class JpegPage:
    """A baseline JPEG file the device decoder takes (``jpeg_plan``): its bytes and the shape of its decode, ``(H, W, components)``.  The
    page kind ``"jpg"`` of ``extractor_batch.read_files``: pages of one shape are decoded by one ``bbocr_jpeg_decode`` call.
    ``orientation``: the plan's EXIF orientation (1 .. 8), which ``shape`` does not reflect -- ``readtext`` reads files un-oriented, and
    only ``Reader.imread_jpeg_batch`` (``cv2.imread``'s page) applies it.  ``progressive``: the page was made from
    ``jpeg_progressive_plan`` -- a progressive file, for which the Reader's batch calls use ``bbocr_jpeg_decode_progressive``."""
    __slots__ = ("data", "shape", "orientation", "progressive")

    def __init__(self, data, plan):
        self.data = data
        self.shape = (int(plan.height), int(plan.width), int(plan.components))
        self.orientation = int(plan.orientation)
        # made from ``jpeg_progressive_plan``: a progressive file, which only ``bbocr_jpeg_decode_progressive`` decodes
        self.progressive = isinstance(plan, _lib.bbocr_jpeg_progressive_plan)


def jpeg_plan(data):
    """``bbocr_host_jpeg_plan`` of a file's bytes (no GPU): geometry, sampling, restart interval, scan range, ``supported`` and the
    ``BBOCR_JPEG_*`` reason a file outside the device decoder's scope is refused with; ``chroma``: 1 / 2 / 3 for a 4:4:4 / 4:2:2 / 4:4:0
    file that the decoder takes when asked to (``device_decode="chroma"``) although ``supported`` is 0."""
    plan = _lib.bbocr_jpeg_plan()
    rc = _lib.load().bbocr_host_jpeg_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_jpeg_plan failed with status {rc}")
    return plan


def jpeg_progressive_plan(data):
    """``bbocr_host_jpeg_progressive_plan`` of a file's bytes (no GPU): the frame, ``supported`` / ``reason`` and the scan script --
    ``plan.scans[k]`` for ``k < plan.n_scans``: components, ``ss, se, ah, al``, the restart interval in force, segments, byte range and
    table ids.  A baseline file is refused by this plan (reason ``BBOCR_JPEG_SOF``): it has ``jpeg_plan``."""
    plan = _lib.bbocr_jpeg_progressive_plan()
    rc = _lib.load().bbocr_host_jpeg_progressive_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_jpeg_progressive_plan failed with status {rc}")
    return plan


JPEG_SCALES = (1, 2, 4, 8)   # bbocr_jpeg_decode_scaled's scales: libjpeg's scale_denom for the ISLOW decode Pillow's draft configures


def draft_scale(W, H, req_w, req_h):
    """``JpegImageFile.draft(None, (req_w, req_h))``'s scale for a ``W x H`` file: the largest of 8, 4, 2, 1 that is at most
    ``min(W // req_w, H // req_h)`` -- the file then decodes to ``ceil(W / scale) x ceil(H / scale)`` and ``Image.thumbnail`` resizes from
    the box ``(0, 0, W / scale, H / scale)``."""
    s = min(W // req_w, H // req_h)
    return 8 if s >= 8 else 4 if s >= 4 else 2 if s >= 2 else 1


DECODE_CHROMA = "chroma"   # the value of ``device_decode`` / ``BBOCR_DEVICE_DECODE`` that adds 4:4:4, 4:2:2 and 4:4:0 files to the device decoder's


DECODE_PROGRESSIVE = "progressive"   # the value that means "chroma" plus the progressive files ``jpeg_progressive_plan`` supports


def jpeg_progressive(device_decode):
    """True for ``device_decode="progressive"``: ``"chroma"``'s scope and progressive files"""
    return isinstance(device_decode, str) and device_decode.strip().lower() == DECODE_PROGRESSIVE


def jpeg_chroma(device_decode):
    """True for ``device_decode="chroma"`` (and ``"progressive"``, which includes it): device decode with the wider scope -- the files
    whose plan has ``chroma`` set although ``supported`` is 0.  Every other value (``True``, ``"1"``, ``False``, ``None``) is today's scope."""
    return isinstance(device_decode, str) and device_decode.strip().lower() in (DECODE_CHROMA, DECODE_PROGRESSIVE)


def jpeg_device_plan(data, chroma=False, progressive=False, plan=None):
    """The plan under which the device decoder takes a file's bytes, or ``None``: ``jpeg_plan``'s (``plan``, when the caller has it) if it
    supports the file or, with ``chroma``, names its class; with ``progressive``, ``jpeg_progressive_plan``'s for a progressive file it
    supports.  ``JpegPage(data, that plan)`` is the page to decode."""
    plan = jpeg_plan(data) if plan is None else plan
    if plan.supported or (chroma and plan.chroma):
        return plan
    if progressive and plan.reason != _lib.JPEG_NOT_JPEG:   # any file with an SOI: the baseline walk may stop before it reaches the SOF2 marker
        pplan = jpeg_progressive_plan(data)
        if pplan.supported:
            return pplan
    return None


def jpeg_page(source, chroma=False, progressive=False):
    """``JpegPage`` of a path or a bytes object when the device decoder takes the file, else ``None`` (the caller keeps its host path).
    ``chroma``: a 4:4:4, 4:2:2 or 4:4:0 file (``plan.chroma``) is taken as well; ``progressive``: so is a progressive file that
    ``jpeg_progressive_plan`` supports."""
    try:
        data = _file_bytes(source)
        plan = jpeg_device_plan(data, chroma, progressive)
        return JpegPage(data, plan) if plan is not None else None
    except Exception:
        return None


class PngPage:
    """A PNG file the device decoder takes (``png_plan``): its bytes and the shape of its decode, ``(H, W, 3)`` -- every PNG page has an RGB
    and a gray plane.  The page kind ``"png"`` of ``extractor_batch.read_files``: pages of one shape are decoded by one ``bbocr_png_decode``
    call."""
    __slots__ = ("data", "shape", "plan")

    def __init__(self, data, plan):
        self.data = data
        self.shape = (int(plan.height), int(plan.width), 3)
        self.plan = plan


def png_plan(data):
    """``bbocr_host_png_plan`` of a file's bytes (no GPU): geometry, depth, colour type, the filtered scanline's ``channels`` / ``row_bytes`` /
    ``bpp``, ``palette_entries``, the IDAT chunks' count and total payload, ``supported`` and the ``BBOCR_PNG_*`` reason of a refusal."""
    plan = _lib.bbocr_png_plan()
    rc = _lib.load().bbocr_host_png_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_png_plan failed with status {rc}")
    return plan


def png_page(source):
    """``PngPage`` of a path or a bytes object when the device decoder takes the file, else ``None`` (the caller keeps its host path)"""
    try:
        data = _file_bytes(source)
        plan = png_plan(data)
        return PngPage(data, plan) if plan.supported else None
    except Exception:
        return None


def png_decode_enabled(png_decode=None):
    """The ``png_decode`` keyword: None means the environment variable ``BBOCR_PNG_DECODE`` (``1`` = on; off when unset)"""
    return os.environ.get("BBOCR_PNG_DECODE", "0").strip() == "1" if png_decode is None else bool(png_decode)


class TiffPage:
    """A TIFF file the device decoder takes (``tiff_plan``): its bytes and the shape of its decode, ``(H, W, 3)`` -- every TIFF page has an
    RGB and a gray plane.  The page kind ``"tiff"`` of ``extractor_batch.read_files``: pages of one shape are decoded by one
    ``bbocr_tiff_decode`` call, and with ``mixed=True`` so are pages of any shapes.  ``fax``: the page is a CCITT file taken under
    ``tiff_fax_plan`` (``fax_plan``: its ``bbocr_tiff_fax``), so a call that holds it goes to ``bbocr_tiff_decode_fax``."""
    __slots__ = ("data", "shape", "plan", "fax", "fax_plan")

    def __init__(self, data, plan, fax_plan=None):
        self.data = data
        self.shape = (int(plan.height), int(plan.width), 3)
        self.plan = plan
        self.fax_plan = fax_plan
        self.fax = fax_plan is not None and int(fax_plan.scheme) != 0


def tiff_plan(data):
    """``bbocr_host_tiff_plan`` of a file's bytes (no GPU): one walk over the header and the first IFD -- geometry, ``bits``, ``samples``,
    ``photometric``, ``compression``, ``predictor``, the byte order, ``rows_per_strip`` / ``strips``, ``row_bytes``, the strips' stored
    bytes, ``supported`` and the ``BBOCR_TIFF_*`` reason of a refusal."""
    plan = _lib.bbocr_tiff_plan()
    rc = _lib.load().bbocr_host_tiff_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_tiff_plan failed with status {rc}")
    return plan


def tiff_fax_plan(data):
    """``bbocr_host_tiff_fax_plan`` of a file's bytes (no GPU) -> ``(plan, fax)``: ``tiff_plan``'s walk in the mode that goes on behind a
    CCITT compression (2, 3, 4) and a fill order other than 1, then the checks of the CCITT decoder.  ``plan.supported``: the plain plan or
    the fax plan takes the file; ``fax.scheme`` (0: no CCITT file), ``fax.t4_options``, ``fax.fill_order`` and the ``BBOCR_FAX_*``
    reason."""
    plan, fax = _lib.bbocr_tiff_plan(), _lib.bbocr_tiff_fax()
    rc = _lib.load().bbocr_host_tiff_fax_plan(data, len(data), C.byref(plan), C.byref(fax))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_tiff_fax_plan failed with status {rc}")
    return plan, fax


def tiff_page(source, fax=False):
    """``TiffPage`` of a path or a bytes object when the device decoder takes the file, else ``None`` (the caller keeps its host path).
    ``fax``: under ``tiff_fax_plan``, so a CCITT file is taken as well."""
    try:
        data = _file_bytes(source)
        if fax:
            plan, fax_plan = tiff_fax_plan(data)
            return TiffPage(data, plan, fax_plan) if plan.supported else None
        plan = tiff_plan(data)
        return TiffPage(data, plan) if plan.supported else None
    except Exception:
        return None


DECODE_FAX = "fax"


def tiff_fax(tiff_decode):
    """True for ``tiff_decode="fax"`` (None: for ``BBOCR_TIFF_DECODE=fax``): the device TIFF decoder with CCITT files in its scope.  Every
    other value (``True``, ``"1"``, ``False``) is the plain scope."""
    if tiff_decode is None:
        tiff_decode = os.environ.get("BBOCR_TIFF_DECODE", "0")
    return isinstance(tiff_decode, str) and tiff_decode.strip().lower() == DECODE_FAX


def tiff_decode_enabled(tiff_decode=None):
    """The ``tiff_decode`` keyword: None means the environment variable ``BBOCR_TIFF_DECODE`` (``1`` = on, ``fax`` = on with CCITT files;
    off when unset).  -> False, True or ``"fax"``"""
    if tiff_fax(tiff_decode):
        return DECODE_FAX
    return os.environ.get("BBOCR_TIFF_DECODE", "0").strip() == "1" if tiff_decode is None else bool(tiff_decode)


class GifPage:
    """A GIF file the device decoder takes (``gif_plan``): its bytes and the shape of its decode, ``(canvas_h, canvas_w, 3)`` -- Pillow's
    frame 0 on its canvas.  The page kind ``"gif"`` of ``extractor_batch.read_files``: pages of any shapes share one ``bbocr_gif_decode``
    call."""
    __slots__ = ("data", "shape", "plan")

    def __init__(self, data, plan):
        self.data = data
        self.shape = (int(plan.canvas_h), int(plan.canvas_w), 3)
        self.plan = plan


def gif_plan(data):
    """``bbocr_host_gif_plan`` of a file's bytes (no GPU): one walk up to the end of frame 0's data -- the screen, the frame rectangle, the
    canvas, ``interlace``, the table in force (``table_len``, ``local_table``, ``table``: the RGB plane's lookup), ``transparency``,
    ``min_code``, ``mode_l``, ``payload_bytes``, ``supported`` and the ``BBOCR_GIF_*`` reason of a refusal."""
    plan = _lib.bbocr_gif_plan()
    rc = _lib.load().bbocr_host_gif_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_gif_plan failed with status {rc}")
    return plan


def gif_page(source):
    """``GifPage`` of a path or a bytes object when the device decoder takes the file, else ``None`` (the caller keeps its host path)"""
    try:
        data = _file_bytes(source)
        plan = gif_plan(data)
        return GifPage(data, plan) if plan.supported else None
    except Exception:
        return None


def gif_decode_enabled(gif_decode=None):
    """The ``gif_decode`` keyword: None means the environment variable ``BBOCR_GIF_DECODE`` (``1`` = on; off when unset)"""
    return os.environ.get("BBOCR_GIF_DECODE", "0").strip() == "1" if gif_decode is None else bool(gif_decode)


class BmpPage:
    """A BMP file the device decoder takes (``bmp_plan``): its bytes and the shape of its decode, ``(H, W, 3)``.  The page kind ``"bmp"`` of
    ``extractor_batch.read_files``: pages of any shapes share one ``bbocr_bmp_decode`` call."""
    __slots__ = ("data", "shape", "plan")

    def __init__(self, data, plan):
        self.data = data
        self.shape = (int(plan.height), int(plan.width), 3)
        self.plan = plan


def bmp_plan(data):
    """``bbocr_host_bmp_plan`` of a file's bytes (no GPU): Pillow's ``_bitmap`` restated -- geometry, ``bits``, ``compression``,
    ``header_size``, ``top_down``, the table (``colors``, ``table_offset``, ``table_entry``), ``mode`` (0 P, 1 Pillow's 1, 2 L, 3 direct
    colour), the bytes of R, G and B, ``row_stride``, ``data_offset``, ``supported`` and the ``BBOCR_BMP_*`` reason of a refusal."""
    plan = _lib.bbocr_bmp_plan()
    rc = _lib.load().bbocr_host_bmp_plan(data, len(data), C.byref(plan))
    if rc != 0:
        raise RuntimeError(f"bbocr_host_bmp_plan failed with status {rc}")
    return plan


def bmp_page(source):
    """``BmpPage`` of a path or a bytes object when the device decoder takes the file, else ``None`` (the caller keeps its host path)"""
    try:
        data = _file_bytes(source)
        plan = bmp_plan(data)
        return BmpPage(data, plan) if plan.supported else None
    except Exception:
        return None


def bmp_decode_enabled(bmp_decode=None):
    """The ``bmp_decode`` keyword: None means the environment variable ``BBOCR_BMP_DECODE`` (``1`` = on; off when unset)"""
    return os.environ.get("BBOCR_BMP_DECODE", "0").strip() == "1" if bmp_decode is None else bool(bmp_decode)


def reformat_input(image, device_gray=False, parallel_decode=False):
    """easyocr/utils.py::reformat_input -> (RGB uint8 HWC, gray uint8 HW); decode is host work (PIL).

    ``device_gray=True`` returns ``None`` for the gray plane wherever upstream derives it from the colour array with
    ``cv2.cvtColor(BGR2GRAY)``: the device computes exactly that (``gray_kernel``), which saves ~2 ms of numpy per 1280x960 page."""
    from PIL import Image

    _gray = (lambda a: None) if device_gray else _gray_bgr2gray

    if isinstance(image, (str, os.PathLike)):
        return decode_file(image, parallel=parallel_decode)
    if isinstance(image, (bytes, bytearray)):
        pil = Image.open(io.BytesIO(bytes(image)))
        img = np.ascontiguousarray(pil.convert("RGB"))
        return img, _gray(img)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError("Invalid input type. numpy input must be uint8")
        if image.ndim == 2:
            return np.ascontiguousarray(np.repeat(image[:, :, None], 3, axis=2)), np.ascontiguousarray(image)
        if image.ndim == 3 and image.shape[2] == 1:
            g = np.ascontiguousarray(image[:, :, 0])
            return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)), g
        if image.ndim == 3 and image.shape[2] == 3:
            return np.ascontiguousarray(image), _gray(image)
        if image.ndim == 3 and image.shape[2] == 4:
            img = np.ascontiguousarray(image[:, :, :3][:, :, ::-1])
            return img, _gray(img)
    elif hasattr(image, "convert"):
        arr = np.asarray(image.convert("RGB"))
        return np.ascontiguousarray(arr[:, :, ::-1]), _gray_bgr2gray(arr)     # (gray of the UN-flipped array: not what the device would derive)
    raise ValueError("Invalid input type. Supporting format = string(file path or url), bytes, numpy array")


def format_output(result, output_format="standard", paragraph=False, detail=1):
    """Tail of easyocr.Reader.readtext: ``detail == 0`` (already text only) wins, then 'dict' / 'json' re-shape each item; the confidence key
    is spelled 'confident' upstream."""
    if detail == 0 or output_format == "standard":
        return result
    if output_format == "dict":
        if paragraph:
            return [{"boxes": item[0], "text": item[1]} for item in result]
        return [{"boxes": item[0], "text": item[1], "confident": item[2]} for item in result]
    if output_format == "json":
        import json

        if paragraph:
            return [json.dumps({"boxes": [list(map(int, lst)) for lst in item[0]], "text": item[1]}, ensure_ascii=False) for item in result]
        return [json.dumps({"boxes": [list(map(int, lst)) for lst in item[0]], "text": item[1], "confident": item[2]}, ensure_ascii=False)
                for item in result]
    raise NotImplementedError(f"output_format {output_format!r}")


def ignore_mask(character, lang_char, allowlist=None, blocklist=None):
    """easyocr.Reader.recognize's ``ignore_char`` rule as a class mask, bit ``c & 31`` of word ``c >> 5`` removing class ``c``: with an allowlist
    every character outside it, else the blocklist, else the characters of the model that are not in the language list (none for
    ``['en']`` + english_g2).  Class index = position in ``character`` (0 is the CTC blank and is never ignored).  Up to 128 classes these
    are the four words of ``bbocr_params.ignore_mask``; a wider model gets ``ceil(len(character) / 32)`` words for ``bbocr_set_class_mask``."""
    if allowlist:
        ignore = set(character[1:]) - set(allowlist)
    elif blocklist:
        ignore = set(blocklist)
    else:
        ignore = set(character[1:]) - set(lang_char)
    words = [0] * max(4, (len(character) + 31) // 32)
    for i, ch in enumerate(character):
        if i and ch in ignore:
            words[i >> 5] |= 1 << (i & 31)
    return words


_NETWORK_PARAMS = {"input_channel": 1, "output_channel": 256, "hidden_size": 256}     # every generation-2 model of easyocr, english_g2 included


def resolve_recog_network(lang_list, recog_network="standard", model_storage_directory=None, user_network_directory=None, character=None,
                          lang_char=None):
    """What ``Reader.__init__`` needs to know about the recogniser, without a device: ``{"character", "lang_char", "model_path", "lang_list"}``.

    ``recog_network="standard"`` is english_g2 and wants ``lang_list == ["en"]``.  Any other name follows easyocr's custom-model convention:
    ``NAME.yaml`` in the user network directory (default ``~/.EasyOCR/user_network``) gives ``network_params``, ``imgH``, ``lang_list`` and
    ``character_list``; ``NAME.pth`` in the model directory (default ``~/.EasyOCR/model``) holds the state-dict.  The architecture is fixed --
    the CRNN every generation-2 model shares -- so ``NAME.py`` is never imported and other ``network_params`` / ``imgH`` are a ValueError.
    ``character`` (a string or a list of class strings, WITHOUT the blank) stands in for the yaml on hosts that have no model files.
    ``character = ['[blank]'] + list(character_list)`` as CTCLabelConverter builds it.  ``lang_char`` defaults to every character of the
    model: easyocr's per-language ``*_char.txt`` tables are not shipped, so nothing is ignored unless the caller says so."""
    model_path = None
    if character is not None:
        chars = list(character)
    elif recog_network == "standard":
        if list(lang_list) != ["en"]:
            raise ValueError(f"{list(lang_list)} is not supported by recog_network='standard' (english_g2, ['en']): pass recog_network=NAME of a "
                             "generation-2 model with its NAME.yaml / NAME.pth, or character=")
        chars = list(CHARSET)
    else:
        import yaml

        user_dir = user_network_directory or os.path.expanduser("~/.EasyOCR/user_network")
        model_dir = model_storage_directory or os.environ.get("BBOCR_WEIGHTS_DIR") or os.path.expanduser("~/.EasyOCR/model")
        path = os.path.join(user_dir, recog_network + ".yaml")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found (recog_network={recog_network!r}; this backend never downloads model files)")
        with open(path, encoding="utf8") as fh:
            cfg = yaml.safe_load(fh) or {}
        params = cfg.get("network_params") or {}
        got = {k: params.get(k) for k in _NETWORK_PARAMS}
        if got != _NETWORK_PARAMS:
            raise ValueError(f"{path}: network_params {got} -- only the generation-2 CRNN {_NETWORK_PARAMS} is implemented")
        if cfg.get("imgH", 64) != 64:
            raise ValueError(f"{path}: imgH {cfg.get('imgH')!r} -- only 64 is implemented")
        if cfg.get("character_list") is None:
            raise ValueError(f"{path}: no character_list")
        chars = list(cfg["character_list"])
        lang_list = cfg.get("lang_list") or lang_list
        model_path = os.path.join(model_dir, recog_network + ".pth")
    chars = [str(c) for c in chars]
    if not 2 <= len(chars) + 1 <= _lib.REC_CLASSES_MAX:
        raise ValueError(f"{len(chars) + 1} classes (blank included): 2 .. {_lib.REC_CLASSES_MAX} are supported")
    return {"character": ["[blank]"] + chars, "lang_char": list(chars) if lang_char is None else list(lang_char), "model_path": model_path,
            "lang_list": list(lang_list)}


def load_dictionary(source, character):
    """The word list of ``decoder='wordbeamsearch'`` as the library takes it, without a device.  ``source``: a path, a list of paths (every
    item an ``os.PathLike`` or the name of an existing file) or an iterable of words; ``None``: the ``os.pathsep``-separated paths of
    ``BBOCR_DICTIONARY`` (unset: no dictionary, ``None`` is returned).  Files hold one word per line and are read as ``utf-8-sig`` with
    ``splitlines()``, upstream's way.  Words are mapped to class indices through ``character`` (the model's list, class 0 the blank); empty
    lines, duplicates and words with a character the model lacks (or the space, which separates words, or more than 1024 characters) are
    dropped and counted.  A model without ``' '`` has no word separator: ``ValueError``.

    -> ``{"words", "symbols" (uint16), "word_off" (int32, [words + 1]), "space", "dropped_foreign", "dropped_empty",
    "dropped_duplicates", "unmatchable_repeats"}``; ``unmatchable_repeats`` counts kept words with a doubled letter, which a decoded text
    equals only through a labelling that holds a blank symbol between the pair (the collapse removes adjacent repeats from the labelling)."""
    if source is None:
        env = os.environ.get("BBOCR_DICTIONARY", "")
        source = [p for p in env.split(os.pathsep) if p]
        if not source:
            return None
        paths = source
    elif isinstance(source, (str, os.PathLike)):
        paths = [source]
    else:
        source = list(source)
        is_paths = bool(source) and all(isinstance(x, os.PathLike) or (isinstance(x, str) and os.path.isfile(x)) for x in source)
        paths = source if is_paths else None
    if paths is not None:
        lines = []
        for path in paths:
            with open(path, "r", encoding="utf-8-sig") as fh:
                lines += fh.read().splitlines()
    else:
        lines = [str(w) for w in source]
    if " " not in character[1:]:
        raise ValueError("decoder='wordbeamsearch' needs a model with a ' ' class: it separates the word groups")
    cls = {ch: i for i, ch in enumerate(character) if i and len(ch) == 1}
    space = cls[" "]
    out = {"words": [], "space": space, "dropped_foreign": 0, "dropped_empty": 0, "dropped_duplicates": 0, "unmatchable_repeats": 0}
    seen, symbols, word_off = set(), [], [0]
    for w in lines:
        if not w:
            out["dropped_empty"] += 1
        elif w in seen:
            out["dropped_duplicates"] += 1
        elif len(w) > 1024 or any(ch == " " or ch not in cls for ch in w):
            out["dropped_foreign"] += 1
        else:
            seen.add(w)
            out["words"].append(w)
            symbols += [cls[ch] for ch in w]
            word_off.append(len(symbols))
            out["unmatchable_repeats"] += any(a == b for a, b in zip(w, w[1:]))
    out["symbols"] = np.array(symbols, dtype=np.uint16)
    out["word_off"] = np.array(word_off, dtype=np.int32)
    return out


def text_table(character):
    """``bbocr_result.text_idx`` -> text for any character list: a uint32 array of code points when every class is ONE code point (a numpy
    take and one utf-32 decode serve a whole result), else the list itself (a class of several code points: joined box by box)."""
    if all(len(c) == 1 for c in character[1:]):
        return np.array([ord("?")] + [ord(c) for c in character[1:]], dtype="<u4")
    return list(character)


def decode_text(table, idx, text_off):
    """the strings of a result: ``idx`` = its class indices (int array), ``text_off`` = [boxes + 1] offsets into it"""
    if isinstance(table, np.ndarray):
        chars = table[idx].tobytes().decode("utf-32-le") if len(idx) else ""       # one code point per class: the offsets stay valid
        return [chars[a:b] for a, b in zip(text_off[:-1], text_off[1:])]
    idx = np.asarray(idx).tolist()
    return ["".join(table[i] for i in idx[a:b]) for a, b in zip(text_off[:-1], text_off[1:])]


def get_paragraph(raw_result, x_ths=1, y_ths=0.5, mode="ltr"):
    """easyocr/utils.py::get_paragraph: greedy clustering of result boxes into paragraphs (a box joins the current group when one
    of its x extremes and one of its y extremes fall inside the group's extent grown by x_ths / y_ths mean heights), then reading
    order inside a group: repeatedly the left-most (ltr) box among those within 0.4 mean heights of the top-most centre.
    Returns ``[[box, text]]`` (no confidence), like upstream."""
    box_group = []
    for box in raw_result:
        all_x = [int(coord[0]) for coord in box[0]]
        all_y = [int(coord[1]) for coord in box[0]]
        min_x, max_x, min_y, max_y = min(all_x), max(all_x), min(all_y), max(all_y)
        box_group.append([box[1], min_x, max_x, min_y, max_y, max_y - min_y, 0.5 * (min_y + max_y), 0])
    current_group = 1
    while len([b for b in box_group if b[7] == 0]) > 0:
        box_group0 = [b for b in box_group if b[7] == 0]
        if len([b for b in box_group if b[7] == current_group]) == 0:
            box_group0[0][7] = current_group
        else:
            cur = [b for b in box_group if b[7] == current_group]
            mean_height = float(np.mean([b[5] for b in cur]))
            min_gx = min(b[1] for b in cur) - x_ths * mean_height
            max_gx = max(b[2] for b in cur) + x_ths * mean_height
            min_gy = min(b[3] for b in cur) - y_ths * mean_height
            max_gy = max(b[4] for b in cur) + y_ths * mean_height
            add_box = False
            for b in box_group0:
                same_h = (min_gx <= b[1] <= max_gx) or (min_gx <= b[2] <= max_gx)
                same_v = (min_gy <= b[3] <= max_gy) or (min_gy <= b[4] <= max_gy)
                if same_h and same_v:
                    b[7] = current_group
                    add_box = True
                    break
            if not add_box:
                current_group += 1
    result = []
    for i in sorted(set(b[7] for b in box_group)):
        cur = [b for b in box_group if b[7] == i]
        mean_height = float(np.mean([b[5] for b in cur]))
        min_gx, max_gx = min(b[1] for b in cur), max(b[2] for b in cur)
        min_gy, max_gy = min(b[3] for b in cur), max(b[4] for b in cur)
        text = ""
        while len(cur) > 0:
            highest = min(b[6] for b in cur)
            candidates = [b for b in cur if b[6] < highest + 0.4 * mean_height]
            if mode == "ltr":
                key = min(b[1] for b in candidates)
                best = [b for b in candidates if b[1] == key][-1]
            else:
                key = max(b[2] for b in candidates)
                best = [b for b in candidates if b[2] == key][-1]
            text += " " + best[0]
            cur.remove(best)
        result.append([[[min_gx, min_gy], [max_gx, min_gy], [max_gx, max_gy], [min_gx, max_gy]], text[1:]])
    return result


def mixed_batch_enabled(mixed=None):
    """The ``mixed`` keyword of the batching callers: None means the environment variable ``BBOCR_MIXED_BATCH`` (``1`` = on; off when unset)"""
    return os.environ.get("BBOCR_MIXED_BATCH", "0").strip() == "1" if mixed is None else bool(mixed)


def mixed_pixel_budget():
    """Pixels per mixed device batch: ``BBOCR_MIXED_PIXEL_BUDGET``, default 64 pages of 1280x960"""
    return int(os.environ.get("BBOCR_MIXED_PIXEL_BUDGET", str(64 * 1280 * 960)))


def mixed_batches(pixels, max_pages, budget=None):
    """Indices ``0 .. len(pixels) - 1`` cut, in order, into batches of at most ``max_pages`` pages and at most ``budget`` pixels (a page
    larger than the budget travels alone)"""
    budget = mixed_pixel_budget() if budget is None else budget
    out, cur, used = [], [], 0
    for i, px in enumerate(pixels):
        if cur and (len(cur) >= max_pages or used + px > budget):
            out.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += px
    if cur:
        out.append(cur)
    return out


def auto_host_threads(local_world=None, cpus=None):
    """``bbocr_config::host_threads`` for this process: 0 (the library sizes its pools from the process's own CPU share) unless several
    ranks share the node un-pinned (torchrun sets LOCAL_WORLD_SIZE): then this rank's share of the CPUs it may run on, at most 16."""
    if local_world is None:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1)
    if local_world <= 1:
        return 0
    if cpus is None:
        cpus = len(os.sched_getaffinity(0))
    return max(1, min(16, cpus // local_world))


def _as_tensor(torch, a):
    """CPU tensor sharing ``a``'s memory, as the SOURCE of a copy.  Arrays decoded by PIL are read-only views of a bytes object; torch only
    warns about those because a write through the tensor would be undefined -- nothing here writes, so the warning is silenced for this
    one call instead of paying a 3.7-MB copy per page to make the array writable."""
    if a.flags.writeable:
        return torch.from_numpy(a)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(a)


class Reader:
    """Drop-in for ``easyocr.Reader`` (English ``english_g2`` recogniser + CRAFT detector) on one MI355X."""

    def __init__(self, lang_list, gpu=True, model_storage_directory=None, user_network_directory=None,
                 detect_network="craft", recog_network="standard", download_enabled=True, detector=True, recognizer=True,
                 verbose=True, quantize=True, cudnn_benchmark=False, weights=None, device_index=None, det_sub_batch=0,
                 rec_max_cols=0, precision=None, call_slots=0, host_threads=None, device_decode=None, rec_quant=None, character=None,
                 lang_char=None, beam_wide=None, png_decode=None, tiff_decode=None, gif_decode=None, bmp_decode=None, dictionary=None,
                 **_ignored):
        import torch

        net = resolve_recog_network(lang_list, recog_network, model_storage_directory, user_network_directory, character, lang_char)
        if rec_quant is None:       # the sequence half in easyocr's CPU default arithmetic (dynamic int8, bbocr_config::rec_quant); `quantize` stays ignored
            rec_quant = os.environ.get("BBOCR_REC_QUANT", "").strip() == "1"
        if rec_quant and len(net["character"]) != len(CHARACTER):
            raise ValueError(f"rec_quant is implemented for english_g2's {len(CHARACTER)} classes only, this model has {len(net['character'])} "
                             "(bbocr_create refuses the pair)")
        if detect_network != "craft":
            raise ValueError("only detect_network='craft' is implemented")
        if not torch.cuda.is_available():
            raise RuntimeError("bb_ocr_amd.Reader needs a HIP device (MI355X); there is no CPU path")
        self._torch = torch
        self.device_index = torch.cuda.current_device() if device_index is None else int(device_index)
        self.device = f"cuda:{self.device_index}"
        self._lib = _lib.load()
        self.rec_quant = bool(rec_quant)
        if self.rec_quant and precision is None:
            precision = "exact_rec"     # what is quantised are the fp32 path's features: the exact recogniser delivers them to 1e-5
        if self.rec_quant and precision in ("bf16", "fp16", "mixed"):
            raise ValueError("rec_quant needs precision 'exact' or 'exact_rec'")
        if precision is None:       # the reference constructs Reader(["en"], gpu=...) (enhanced_extractor.py:153): the mode comes from the environment
            # default "fp16": the cheapest mode whose boxes AND strings equalled the fp32 CPU path's on everything measured -- 2,051 boxes
            # of synthetic pages, 471 of dense A4 scans, 110 on the reference's seven real images.  "mixed" (bf16
            # detector) is 1.6 % faster and equally exact on binary-ink pages, but flips threshold decisions on continuous-tone images
            precision = os.environ.get("BBOCR_PRECISION", "fp16").strip().lower()
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")      # see bbocr_config::precision (include/bbocr.h)
        self.precision = precision
        if host_threads is None:
            host_threads = auto_host_threads()
        self.host_threads = int(host_threads)
        if device_decode is None:   # baseline JPEG files decoded on the card (csrc/jpegdec.hip) by readtext(path); off unless asked for
            env = os.environ.get("BBOCR_DEVICE_DECODE", "0").strip().lower()
            device_decode = env if env in (DECODE_CHROMA, DECODE_PROGRESSIVE) else env == "1"
        self.device_decode = bool(device_decode)
        self.jpeg_chroma = jpeg_chroma(device_decode)     # "chroma": 4:4:4, 4:2:2 and 4:4:0 files are decoded on the card as well
        self.jpeg_progressive = jpeg_progressive(device_decode)   # "progressive": those, and progressive files (csrc/jpegprog.hip)
        # PNG files decoded on the card (csrc/pngdec.hip) by readtext(path) and the file callers; an option of its own (None:
        # BBOCR_PNG_DECODE=1), not a value of device_decode, whose strings are a ladder of JPEG scopes; off unless asked for
        self.png_decode = png_decode_enabled(png_decode)
        # TIFF files decoded on the card (csrc/tiffdec.hip), likewise an option of its own (None: BBOCR_TIFF_DECODE=1); off unless asked for;
        # "fax" (BBOCR_TIFF_DECODE=fax): CCITT files as well (csrc/tiff_fax.h)
        self.tiff_decode = tiff_decode_enabled(tiff_decode)
        # GIF files decoded on the card (csrc/gifdec.hip), likewise (None: BBOCR_GIF_DECODE=1); off unless asked for
        self.gif_decode = gif_decode_enabled(gif_decode)
        # BMP files decoded on the card (csrc/bmpdec.hip), likewise (None: BBOCR_BMP_DECODE=1); off unless asked for
        self.bmp_decode = bmp_decode_enabled(bmp_decode)
        if beam_wide is None:       # decoder='beamsearch' of a model of more than 128 classes searched on the card (csrc/ctc_beam_wide.hip); off unless asked for
            beam_wide = os.environ.get("BBOCR_BEAM_WIDE", "").strip() == "1"
        self.beam_wide = bool(beam_wide)
        kw = dict(device=self.device_index, det_sub_batch=int(det_sub_batch), rec_max_cols=int(rec_max_cols),
                  precision=_lib.PRECISIONS[precision], call_slots=int(call_slots), host_threads=self.host_threads,
                  rec_quant=int(self.rec_quant), rec_classes=0 if net["character"] == CHARACTER else len(net["character"]))
        h = C.c_void_p()
        if self.beam_wide:          # the appended field travels in bbocr_config_v2; without it bbocr_create's 32 bytes say everything
            rc = self._lib.bbocr_create_v2(C.byref(_lib.bbocr_config_v2(beam_wide=1, **kw)), C.byref(h))
        else:
            rc = self._lib.bbocr_create(C.byref(_lib.bbocr_config(**kw)), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"bbocr_create failed with status {rc}")
        self._h = h
        self.character = CHARACTER if net["character"] == CHARACTER else net["character"]
        self.lang_char = net["lang_char"]
        self._wide = len(self.character) > 128                                  # the class mask travels through bbocr_set_class_mask
        self._text_table = None if self.character is CHARACTER else text_table(self.character)   # None: the English latin-1 fast path
        # the word list of decoder='wordbeamsearch' (None: the files of BBOCR_DICTIONARY; neither: no dictionary, and the decoder stays
        # NotImplementedError as ever)
        self._dictionary = None
        self.set_dictionary(dictionary)
        if isinstance(weights, str) and weights == "empty":
            # multi-GPU receiver: the packed plans are laid out without values and filled by import_weights_blob (dist.broadcast_packed)
            for which, wanted in ((0, detector), (1, recognizer)):
                if wanted:
                    self._check(self._lib.bbocr_alloc_weights(self._h, which))
            return
        craft_state, crnn_state = self._resolve_weights(weights, model_storage_directory, net["model_path"], detector, recognizer)
        if detector:
            self._load(0, craft_state)
        if recognizer:
            self._load(1, crnn_state)

    # -- weights -------------------------------------------------------------------
    @staticmethod
    def _resolve_weights(weights, model_storage_directory, model_path=None, detector=True, recognizer=True):
        if isinstance(weights, tuple):
            return weights
        if weights == "synthetic" or os.environ.get("BBOCR_SYNTHETIC_WEIGHTS", "") == "1":
            return _weights.designed_craft_state(0), _weights.synthetic_crnn_state(0)
        directory = model_storage_directory or os.environ.get("BBOCR_WEIGHTS_DIR") or os.path.expanduser("~/.EasyOCR/model")
        if model_path is not None:        # a custom recogniser (recog_network=NAME): its NAME.pth beside the detector's checkpoint
            wanted = [os.path.join(directory, "craft_mlt_25k.pth") if detector else None, model_path if recognizer else None]
            for p in wanted:                      # only the half that was asked for is looked for and read
                if p is not None and not os.path.exists(p):
                    raise FileNotFoundError(f"{p} not found (this backend never downloads model files)")
            return tuple(None if p is None else _weights.load_checkpoint(p) for p in wanted)
        return _weights.load_checkpoint_dir(directory)

    def _load(self, which, state):
        arr, keep = _weights.to_descs(state)
        self._check(self._lib.bbocr_load_weights(self._h, which, arr, len(arr)))
        del keep

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.bbocr_last_error(self._h)
            raise RuntimeError(f"libbbocr status {rc}: {msg.decode(errors='replace') if msg else ''}")

    # -- packed weights as one device blob (multi-GPU broadcast, include/bbocr.h) -------
    def weights_blob_size(self):
        n = C.c_size_t()
        self._check(self._lib.bbocr_weights_blob_size(self._h, C.byref(n)))
        return int(n.value)

    def export_weights_blob(self):
        """-> uint8 device tensor holding every packed weight block of this context (BN folded, element type rounded, MFMA order)."""
        blob = self._torch.empty(self.weights_blob_size(), dtype=self._torch.uint8, device=self.device)
        self._check(self._lib.bbocr_weights_export(self._h, C.c_void_p(blob.data_ptr()), blob.numel()))
        return blob

    def import_weights_blob(self, blob):
        """Fill a ``Reader(weights="empty")`` from another rank's blob (same precision, same networks)."""
        self._dev_u8(blob, "weight blob", 1, (self.weights_blob_size(),))
        self._check(self._lib.bbocr_weights_import(self._h, C.c_void_p(blob.data_ptr()), blob.numel()))

    # -- rec_quant stage entry points (bbocr_op_qlinear / bbocr_op_qlstm): what the tests pin against tests/quant_ref.py -------
    def _q_seqs(self, seqs):
        flat = [int(v) for pair in seqs for v in pair]
        return (C.c_int * len(flat))(*flat), len(flat) // 2

    def _dev_f32(self, t, name, shape):
        torch = self._torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device_index or t.dtype != torch.float32 \
                or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or min(t.shape) <= 0:
            raise ValueError(f"{name}: expected a contiguous float32 tensor {tuple(shape)} on {self.device}")
        return t

    def qlinear_device(self, x, seqs, layer):
        """One dynamically quantised product of a ``rec_quant`` Reader.  x: float32 device tensor [rows, K]; seqs: (first row, T) per crop, tiling
        the rows in order; layer: 0 / 1 input projection of BiLSTM 0 / 1 (K 256 -> 2048), 2 / 3 the Linear behind it (512 -> 256), 4 Prediction
        (256 -> 112).  -> (out float32 [rows, N], codes uint8 [rows, K], params float32 [crops, 2] = (scale, zero point)) -- out and codes on
        the device, params a numpy array."""
        import numpy as np

        torch = self._torch
        if layer not in (0, 1, 2, 3, 4):
            raise ValueError("layer: 0 / 1 input projections, 2 / 3 the Linear layers, 4 Prediction")
        K = 512 if layer in (2, 3) else 256
        N = {0: 2048, 1: 2048, 2: 256, 3: 256, 4: 112}[layer]
        rows = int(x.shape[0]) if hasattr(x, "shape") and len(x.shape) == 2 else 0
        self._dev_f32(x, "x", (rows, K))
        tab, nseq = self._q_seqs(seqs)
        out = torch.empty((rows, N), dtype=torch.float32, device=self.device)
        codes = torch.empty((rows, K), dtype=torch.uint8, device=self.device)
        params = np.zeros((nseq, 2), np.float32)
        self._check(self._lib.bbocr_op_qlinear(self._h, C.c_void_p(x.data_ptr()), rows, tab, nseq, int(layer), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(codes.data_ptr()), params.ctypes.data_as(C.POINTER(C.c_float))))
        return out, codes, params

    def qlstm_device(self, g, seqs, layer):
        """The int8 recurrence of BiLSTM ``layer`` of a ``rec_quant`` Reader.  g: float32 device tensor [rows, 2048], the input projection
        (column dir * 1024 + gate * 256 + unit); seqs as in qlinear_device.  -> device tensors (h [rows, 512], c [rows, 512], hcodes uint8
        [rows, 512], hparams [rows, 2, 2]): h and c AFTER step t of each direction, and the codes and (scale, zero point) of the h that entered it."""
        torch = self._torch
        if layer not in (0, 1):
            raise ValueError("layer: 0 or 1")
        rows = int(g.shape[0]) if hasattr(g, "shape") and len(g.shape) == 2 else 0
        self._dev_f32(g, "g", (rows, 2048))
        tab, nseq = self._q_seqs(seqs)
        h = torch.zeros((rows, 512), dtype=torch.float32, device=self.device)
        c = torch.zeros((rows, 512), dtype=torch.float32, device=self.device)
        hcodes = torch.zeros((rows, 512), dtype=torch.uint8, device=self.device)
        hparams = torch.zeros((rows, 2, 2), dtype=torch.float32, device=self.device)
        self._check(self._lib.bbocr_op_qlstm(self._h, C.c_void_p(g.data_ptr()), rows, tab, nseq, int(layer), C.c_void_p(h.data_ptr()),
                                             C.c_void_p(c.data_ptr()), C.c_void_p(hcodes.data_ptr()), C.c_void_p(hparams.data_ptr())))
        return h, c, hcodes, hparams

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.bbocr_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------
    def _params(self, kw):
        p = _lib.bbocr_params()
        self._lib.bbocr_default_params(C.byref(p))
        for k in _DET_KW + ("contrast_ths", "adjust_contrast"):
            if k in kw and kw[k] is not None:
                setattr(p, k, kw[k])
        words = ignore_mask(self.character, self.lang_char, kw.get("allowlist"), kw.get("blocklist"))
        if self._wide:                   # kept by the library for THIS thread's next pipeline call; always set, so that no earlier mask lingers
            arr = (C.c_uint32 * len(words))(*words)
            self._check(self._lib.bbocr_set_class_mask(self._h, arr, len(words) if any(words) else 0))
        else:
            for i, w in enumerate(words):
                p.ignore_mask[i] = w
        decoder = kw.get("decoder", "greedy")
        self._unsupported(decoder, None, None, None, False, "standard")
        rotation = list(kw.get("rotation_info") or [])
        if len(rotation) > 3 or any(a not in (90, 180, 270) for a in rotation):
            raise ValueError("rotation_info: up to three angles out of 90, 180, 270")
        for i, a in enumerate(rotation):
            p.rotation_info[i] = int(a)
        if decoder == "beamsearch":          # BBOCR_DECODER_BEAMSEARCH
            p.decoder, p.beam_width = 1, int(kw.get("beamWidth", 5))
        if decoder == "wordbeamsearch":      # BBOCR_DECODER_WORDBEAMSEARCH, over set_dictionary's words
            p.decoder, p.beam_width = 2, int(kw.get("beamWidth", 5))
        return p

    def _to_dev(self, arr):
        """Host array -> device tensor; a LIST of equal-shape arrays -> one device tensor ``[len, ...]`` filled page by page (no host-side
        ``np.stack``: for 64 decoded pages that copy is 236 MB on one thread, the largest serial cost of a decode-bound caller)."""
        torch = self._torch
        if isinstance(arr, (list, tuple)):
            if not arr:
                raise ValueError("empty page list")
            pages = [np.ascontiguousarray(a) for a in arr]           # (kept alive until the call below has returned)
            first = pages[0]
            if any(a.dtype != np.uint8 or a.shape != first.shape for a in pages):
                raise ValueError("pages of one batch must be uint8 arrays of one shape")
            t = torch.empty((len(pages),) + first.shape, dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device_index).synchronize()
            ptrs = (C.c_void_p * len(pages))(*[a.ctypes.data for a in pages])
            # ONE call for the whole batch: the interpreter lock is released once, not once per page (with a decode pool running, every
            # re-acquisition can wait for a thread that holds it)
            self._check(self._lib.bbocr_upload_pages(self._h, ptrs, len(pages), first.nbytes, C.c_void_p(t.data_ptr())))
            return t
        arr = np.ascontiguousarray(arr)
        t = _as_tensor(torch, arr).to(self.device)
        torch.cuda.current_stream(self.device_index).synchronize()
        return t

    def _dev_u8(self, t, name, ndim, shape=None):
        """A tensor about to cross the C ABI as a raw pointer: anything but a contiguous uint8 tensor of the expected shape on THIS
        context's device would be an out-of-bounds device access (a GPU fault kills the process; the reference relies on exceptions,
        enhanced_extractor.py:529-531) -> ValueError before the ctypes call."""
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch uint8 device tensor, got {type(t).__name__}")
        if not t.is_cuda or t.device.index != self.device_index:
            raise ValueError(f"{name}: tensor lives on {t.device}, this Reader runs on {self.device}")
        if t.dtype != torch.uint8:
            raise ValueError(f"{name}: dtype must be uint8, got {t.dtype}")
        if t.ndim != ndim or (shape is not None and tuple(t.shape) != tuple(shape)) or min(t.shape) <= 0:
            raise ValueError(f"{name}: bad shape {tuple(t.shape)}" + (f", expected {tuple(shape)}" if shape is not None else f" ({ndim}-D expected)"))
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        return t

    def _collect(self, res_p, detail=1):
        """bbocr_result -> per-page [(bbox, text, conf)] (upstream's list shape); numpy views instead of per-element ctypes access."""
        r = res_p.contents
        out = []
        try:
            B = r.n_images
            box_off = np.ctypeslib.as_array(r.box_off, shape=(B + 1,)).tolist()
            nb = box_off[-1]
            items = []
            if nb:
                quads = np.ctypeslib.as_array(r.quads, shape=(nb, 8))
                text_off = np.ctypeslib.as_array(r.text_off, shape=(nb + 1,)).tolist()
                conf = np.ctypeslib.as_array(r.conf, shape=(nb,)).tolist()
                nt = text_off[-1]
                # every box's text in ONE decode, then plain str slices (a per-box join over numpy objects cost 3 ms per 64 pages); a euro sign
                # is one character before and after the substitution, so the offsets stay valid
                tidx = np.ctypeslib.as_array(r.text_idx, shape=(max(nt, 1),))[:nt]
                if self._text_table is not None:                                     # any other character list: code points, or joined strings
                    texts = decode_text(self._text_table, tidx, text_off)
                chars = _CLASS_BYTES[tidx].tobytes().decode("latin-1") if nt and self._text_table is None else ""
                if "\x80" in chars:
                    chars = chars.replace("\x80", "\u20ac")
                boxes = quads.astype(np.int64).reshape(nb, 4, 2).tolist()          # horizontal boxes: python ints, like upstream
                free = np.flatnonzero(np.ctypeslib.as_array(r.is_free, shape=(nb,)))
                if free.size:                                                        # free boxes keep their float corners
                    for i, q in zip(free.tolist(), quads[free].reshape(-1, 4, 2).tolist()):
                        boxes[i] = q
                if self._text_table is None:
                    texts = [chars[a:b] for a, b in zip(text_off[:-1], text_off[1:])]
                items = list(zip(boxes, texts, conf))
            out = [items[box_off[b]:box_off[b + 1]] for b in range(B)]
        finally:
            self._lib.bbocr_free_result(res_p)
        if detail == 0:
            return [[item[1] for item in page] for page in out]
        return out

    def set_dictionary(self, dictionary):
        """Set or replace the word list of ``decoder='wordbeamsearch'`` (``load_dictionary``'s sources; ``None``: the files of
        ``BBOCR_DICTIONARY``).  No source, or one without a usable word, clears it: the decoder is ``NotImplementedError`` again."""
        d = load_dictionary(dictionary, self.character)
        if d is None and self._dictionary is None:
            return
        if d is not None and len(d["words"]):
            self._check(self._lib.bbocr_set_dictionary(self._h, d["symbols"].ctypes.data_as(C.POINTER(C.c_uint16)),
                                                       d["word_off"].ctypes.data_as(C.POINTER(C.c_int)), len(d["words"]), d["space"]))
        else:
            self._check(self._lib.bbocr_set_dictionary(self._h, None, None, 0, 0))
        self._dictionary = d if d is not None and len(d["words"]) else None

    def dictionary_stats(self):
        """``{"words", "dropped_foreign", "unmatchable_repeats", "slots", "longest_probe"}`` of the dictionary in use (zeros without one):
        the words kept, the lines dropped for a character the model lacks, the kept words with a doubled letter -- matched only through
        a labelling with a blank symbol between the pair, as the collapse removes adjacent repeats from the labelling -- and the device table's size and longest probe run."""
        w, sl, pr, un = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.bbocr_dictionary_stats(self._h, C.byref(w), C.byref(sl), C.byref(pr), C.byref(un)))
        return {"words": w.value, "dropped_foreign": self._dictionary["dropped_foreign"] if self._dictionary else 0,
                "unmatchable_repeats": un.value, "slots": sl.value, "longest_probe": pr.value}

    def last_ctc_route(self):
        """Where the text of this thread's last recognise / readtext call came from (bbocr_last_ctc_route): 0 greedy, 1 beam search on the host,
        2 beam search on the device, 3 greedy with Prediction inside the CTC kernel (more than 128 classes, 16-bit modes), 4 beam search on the
        device over more than 128 classes (beam_wide), 5 word beam search on the host, 6 word beam search on the device, -1 no pass yet"""
        route = C.c_int(-1)
        self._check(self._lib.bbocr_last_ctc_route(self._h, C.byref(route)))
        return int(route.value)

    def last_ctc_host_sequences(self):
        """Sequences of this thread's last recognise / readtext call that the wide device beam search (route 4) left to the host search
        because one of their rows had more than 128 candidate classes (bbocr_last_ctc_host_sequences)"""
        n = C.c_int(0)
        self._check(self._lib.bbocr_last_ctc_host_sequences(self._h, C.byref(n)))
        return int(n.value)

    def stage_times(self):
        ms = (C.c_float * 8)()
        self._check(self._lib.bbocr_stage_times(self._h, ms, 8))
        keys = ("detector_net", "ccl_device", "box_geometry_host", "crops", "recognizer_net", "ctc", "contrast_retry", "total")
        return dict(zip(keys, [float(v) for v in ms]))

    def set_profiling(self, on: bool):
        """Time every conv_mfma launch with HIP events on the library's stream (bench.py roofline leg)."""
        self._check(self._lib.bbocr_set_profiling(self._h, int(on)))      # 0 off, 1/True detector launches, 2 also the recogniser's

    def conv_profile(self, group: int):
        """-> (sum of launch ms, sum of algorithmic flops, launches) for group 0 (detector) / 1 (recogniser)."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_longlong()
        self._check(self._lib.bbocr_conv_profile(self._h, group, C.byref(ms), C.byref(fl), C.byref(n)))
        return ms.value, fl.value, n.value

    # -- easyocr surface ---------------------------------------------------------------
    def readtext_device(self, rgb_dev, gray_dev=None, **kw):
        """Batch entry for pages already resident in HBM: uint8 torch tensors [B,H,W,3] (+ optional [B,H,W])."""
        self._dev_u8(rgb_dev, "rgb", 4)
        B, H, W, ch = rgb_dev.shape
        if ch != 3:
            raise ValueError(f"rgb: last dimension must be 3, got {ch}")
        if gray_dev is not None:
            self._dev_u8(gray_dev, "gray", 3, (B, H, W))
        p = self._params(kw)
        res = C.POINTER(_lib.bbocr_result)()
        gp = C.c_void_p(gray_dev.data_ptr()) if gray_dev is not None else C.c_void_p(None)
        self._check(self._lib.bbocr_readtext_batch(self._h, C.c_void_p(rgb_dev.data_ptr()), gp, B, H, W, C.byref(p), C.byref(res)))
        return self._shape_results(res, kw)

    def _page_view(self, t, name, px):
        """A page about to cross the C ABI as pointer + row pitch: a uint8 tensor ``[H,W,3]`` (``px`` 3) or ``[H,W]`` (``px`` 1) on this
        Reader's device.  A view with packed pixels and a positive row stride is taken as it is -- only one whose pixels are not packed (a
        channel flip, a column step) is made contiguous first.  -> ``(tensor to keep alive, pitch in bytes)``; ``ValueError`` otherwise."""
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch uint8 device tensor, got {type(t).__name__}")
        if not t.is_cuda or t.device.index != self.device_index:
            raise ValueError(f"{name}: tensor lives on {t.device}, this Reader runs on {self.device}")
        if t.dtype != torch.uint8:
            raise ValueError(f"{name}: dtype must be uint8, got {t.dtype}")
        if t.ndim != (3 if px == 3 else 2) or (px == 3 and t.shape[2] != 3) or min(t.shape) <= 0:
            raise ValueError(f"{name}: bad shape {tuple(t.shape)}, expected " + ("[H,W,3]" if px == 3 else "[H,W]"))
        packed = t.stride(1) == px and (px == 1 or t.stride(2) == 1)
        if not packed or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * px):
            t = t.contiguous()
        return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1] * px)

    def readtext_pages(self, pages, **kw):
        """Pages of individually given shapes already resident in HBM, read by ONE device call (``bbocr_readtext_pages``): ``pages`` is a
        list of uint8 device tensors ``[H,W,3]`` or of ``(rgb, gray)`` pairs (``gray`` ``[H,W]`` or None: derived on the card, as
        ``readtext_device`` derives it).  Strided views -- crops of larger device pages -- are passed by pointer and row pitch and read in
        place.  Keywords and return value are ``readtext_device``'s: one result list per page, equal to what ``readtext_device`` returns
        for each page on its own."""
        pages = list(pages)
        if not pages:
            raise ValueError("readtext_pages: no pages")
        arr = (_lib.bbocr_page * len(pages))()
        keep = []
        for k, page in enumerate(pages):
            rgb, gray = page if isinstance(page, (tuple, list)) else (page, None)
            rgb, pitch = self._page_view(rgb, f"page {k} rgb", 3)
            keep.append(rgb)
            arr[k].dev_rgb, arr[k].H, arr[k].W, arr[k].rgb_pitch = rgb.data_ptr(), rgb.shape[0], rgb.shape[1], pitch
            if gray is not None:
                gray, gpitch = self._page_view(gray, f"page {k} gray", 1)
                if tuple(gray.shape) != tuple(rgb.shape[:2]):
                    raise ValueError(f"page {k} gray: bad shape {tuple(gray.shape)}, expected {tuple(rgb.shape[:2])}")
                keep.append(gray)
                arr[k].dev_gray, arr[k].gray_pitch = gray.data_ptr(), gpitch
        p = self._params(kw)
        res = C.POINTER(_lib.bbocr_result)()
        self._torch.cuda.current_stream(self.device_index).synchronize()     # copies made above; the library runs on its own stream
        self._check(self._lib.bbocr_readtext_pages(self._h, arr, len(pages), C.byref(p), C.byref(res)))
        del keep
        return self._shape_results(res, kw)

    def _shape_results(self, res, kw):
        """The tail of a pipeline call: ``bbocr_result`` -> per-page lists, through ``get_paragraph`` when asked for"""
        if kw.get("paragraph"):
            # Reader.readtext tail: get_paragraph on the raw result, then detail == 0 keeps the text only
            pages = [get_paragraph(page, x_ths=kw.get("x_ths", 1.0), y_ths=kw.get("y_ths", 0.5), mode="ltr") for page in self._collect(res, 1)]
            return [[item[1] for item in page] for page in pages] if kw.get("detail", 1) == 0 else pages
        return self._collect(res, kw.get("detail", 1))

    def pages_from_ycc(self, ycc_dev):
        """Device tensor ``uint8 [B,H,W,3]`` of libjpeg YCbCr triples (``decode_file_ycc``) -> ``(rgb_dev, gray_dev)``: the RGB pages and Y
        planes ``readtext_device`` takes, computed on the card by libjpeg's own integer colour conversion."""
        self._dev_u8(ycc_dev, "ycc", 4)
        B, H, W, ch = ycc_dev.shape
        if ch not in (3, 4):                                         # 4: Pillow's padded pixels (decode_file_ycc(padded=True))
            raise ValueError(f"ycc: last dimension must be 3 or 4, got {ch}")
        torch = self._torch
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=ycc_dev.device)
        gray = torch.empty((B, H, W), dtype=torch.uint8, device=ycc_dev.device)
        torch.cuda.current_stream(self.device_index).synchronize()       # the library runs on its own stream
        self._check(self._lib.bbocr_op_ycc_to_rgb(self._h, C.c_void_p(ycc_dev.data_ptr()), B * H * W, ch, C.c_void_p(rgb.data_ptr()),
                                                  C.c_void_p(gray.data_ptr())))
        return rgb, gray

    @staticmethod
    def _jpeg_files(pages):
        """The ``files`` and ``sizes`` arrays of a JPEG batch call (the pages keep their bytes alive)"""
        n = len(pages)
        return (C.c_void_p * n)(*[C.cast(C.c_char_p(p.data), C.c_void_p) for p in pages]), (C.c_size_t * n)(*[len(p.data) for p in pages])

    def decode_jpeg_batch(self, pages, padded=False, scale=1):
        """``JpegPage`` s of ONE shape -> ``(batch, status)``: the device tensor ``uint8 [n,H,W,3]`` (``padded``: ``[n,H,W,4]``) of libjpeg's
        YCbCr triples -- what ``pages_from_ycc`` takes -- or ``[n,H,W]`` for 1-component files, decoded by ONE ``bbocr_jpeg_decode`` call
        (only the files' bytes cross the link), and the per-file status list (0, or negative: that page of the batch is undefined).
        ``scale`` 2, 4 or 8: the decode at that fraction, Pillow's ``draft`` (``bbocr_jpeg_decode_scaled``): ``H`` and ``W`` are then
        ``ceil(. / scale)`` of the pages', and a 4:4:4, 4:2:2 or 4:4:0 file gets a negative status."""
        torch = self._torch
        pages = list(pages)
        if not pages or any(p.shape != pages[0].shape for p in pages):
            raise ValueError("decode_jpeg_batch: pages of one decoded shape")
        if scale not in JPEG_SCALES:
            raise ValueError(f"scale must be one of {JPEG_SCALES}")
        H, W, comps = pages[0].shape
        H, W = -(-H // scale), -(-W // scale)
        layout = _lib.PAGE_YCBCR4 if padded else _lib.PAGE_YCBCR3
        px = _lib.PAGE_PX_BYTES[_lib.PAGE_GRAY if comps == 1 else layout]
        t = torch.empty((len(pages), H, W) + ((px,) if comps == 3 else ()), dtype=torch.uint8, device=self.device)
        torch.cuda.current_stream(self.device_index).synchronize()
        n = len(pages)
        files, sizes = self._jpeg_files(pages)
        outs = (C.c_void_p * n)(*[t.data_ptr() + k * H * W * px for k in range(n)])
        pitches = (C.c_longlong * n)(*([W * px] * n))
        status = (C.c_int * n)()
        if any(p.progressive for p in pages):              # the call that takes every file of the others, and progressive ones
            out = _lib.bbocr_jpeg_output(scale, _lib.JPEG_FORM_YCBCR, outs, pitches)
            self._check(self._lib.bbocr_jpeg_decode_progressive(self._h, files, sizes, n, layout, C.byref(out), 1, status))
        elif scale == 1:
            self._check(self._lib.bbocr_jpeg_decode(self._h, files, sizes, n, layout, outs, pitches, status))
        else:
            self._check(self._lib.bbocr_jpeg_decode_scaled(self._h, files, sizes, n, layout, scale, outs, pitches, status))
        return t, list(status)

    def imread_jpeg_batch(self, pages):
        """``JpegPage`` s of any shapes -> ``(tensors, status)``: per page ``cv2.imread``'s BGR page ``uint8 [H',W',3]`` on the device -- the
        decode with the page's EXIF orientation applied (``H'``, ``W'`` swapped for orientations 5 .. 8), a grey file replicated -- by ONE
        ``bbocr_jpeg_imread`` call, and the per-file status list (non-zero: that tensor is undefined)."""
        torch = self._torch
        pages = list(pages)
        if not pages:
            raise ValueError("imread_jpeg_batch: no pages")
        outs = []
        for p in pages:
            H, W, _ = p.shape
            outs.append(torch.empty((W, H, 3) if p.orientation >= 5 else (H, W, 3), dtype=torch.uint8, device=self.device))
        torch.cuda.current_stream(self.device_index).synchronize()
        n = len(pages)
        files, sizes = self._jpeg_files(pages)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
        pitches = (C.c_longlong * n)(*[t.shape[1] * 3 for t in outs])
        status = (C.c_int * n)()
        if any(p.progressive for p in pages):
            out = _lib.bbocr_jpeg_output(1, _lib.JPEG_FORM_IMREAD, ptrs, pitches)
            self._check(self._lib.bbocr_jpeg_decode_progressive(self._h, files, sizes, n, _lib.PAGE_YCBCR4, C.byref(out), 1, status))
        else:
            self._check(self._lib.bbocr_jpeg_imread(self._h, files, sizes, n, ptrs, pitches, status))
        return outs, list(status)

    def pages_from_jpeg(self, batch):
        """The tensor of ``decode_jpeg_batch`` -> ``(rgb_dev, gray_dev)``: ``pages_from_ycc`` of the triples ``[n,H,W,3 or 4]``; for
        1-component files ``[n,H,W]`` the samples, replicated for RGB."""
        if batch.ndim == 4:
            return self.pages_from_ycc(batch)
        return batch[..., None].expand(-1, -1, -1, 3).contiguous(), batch

    def encode_jpeg(self, page_dev, layout=None, quality=85, components=None, comment=None):
        """A uint8 device page -> the bytes of the JPEG file Pillow saves for it (``Image.fromarray(...).save(buf, "JPEG", quality=quality)``),
        written on the card by ``bbocr_jpeg_encode`` (csrc/jpegenc.hip): baseline JFIF, 4:2:0, standard Huffman tables.  ``page_dev``:
        ``[H,W]`` or ``[H,W,C]`` rows of packed pixels of a ``PAGE_*`` ``layout`` (default: GRAY for ``[H,W]``, RGB for 3 bytes per pixel,
        YCBCR4 for 4); a strided row pitch (a crop of a larger page) is read in place.  ``components``: 3 = YCbCr (a gray page: what Pillow
        saves for its ``convert("RGB")``), 1 = one component (gray pages only, Pillow's ``"L"`` save); default 1 for a gray page, else 3.
        ``comment``: bytes of a COM segment (Pillow's ``info["comment"]``), at most 65533.  ``ValueError`` for anything else."""
        from .preprocess import _page_layout

        if layout is None:
            ch = page_dev.shape[2] if getattr(page_dev, "ndim", 0) == 3 else 1
            layout = {1: _lib.PAGE_GRAY, 3: _lib.PAGE_RGB, 4: _lib.PAGE_YCBCR4}.get(int(ch), _lib.PAGE_RGB)
        if layout not in _lib.PAGE_PX_BYTES:
            raise ValueError(f"unknown page layout {layout!r}")
        H, W, pitch, _ = _page_layout(self, page_dev, (layout,))
        if components is None:
            components = 1 if layout == _lib.PAGE_GRAY else 3
        if components not in (1, 3) or (components == 1 and layout != _lib.PAGE_GRAY):
            raise ValueError("components must be 3, or 1 for a gray page")
        if H > 65535 or W > 65535:
            raise ValueError("a JPEG file holds at most 65535 x 65535 pixels")
        if not isinstance(quality, int) or not 1 <= quality <= 100:
            raise ValueError("quality must be an int in 1 .. 100")
        if isinstance(comment, str):
            comment = comment.encode()
        comment = bytes(comment) if comment else b""
        if len(comment) > 65533:
            raise ValueError("a comment holds at most 65533 bytes")
        cap = int(self._lib.bbocr_jpeg_encode_bound(H, W, components))
        out = np.empty(cap, np.uint8)                                   # (untouched pages of it cost nothing)
        n = C.c_size_t()
        self._torch.cuda.current_stream(self.device_index).synchronize()      # the library runs on its own stream
        self._check(self._lib.bbocr_jpeg_encode(self._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, int(layout), int(components), int(quality),
                                                C.cast(C.c_char_p(comment), C.c_void_p) if comment else None, len(comment),
                                                C.c_void_p(out.ctypes.data), cap, C.byref(n)))
        return out[:n.value].tobytes()

    def encode_png(self, page_dev, layout=None, icc_profile=None):
        """A uint8 device page -> the bytes of a lossless 8-bit PNG file of it, written on the card by ``bbocr_png_encode``
        (csrc/pngenc.hip): adaptive filters, run matches, dynamic Huffman codes per 16 KiB chunk.  NOT the bytes Pillow writes: opened
        with Pillow the file has the mode (``L`` / ``RGB``), size, pixels and ``info["icc_profile"]`` of Pillow's file.  ``page_dev``:
        ``[H,W]`` or ``[H,W,3]`` rows of packed pixels of ``layout`` GRAY, RGB or BGR (default: GRAY for ``[H,W]``, RGB for ``[H,W,3]``); a
        strided row pitch (a crop of a larger page) is read in place.  ``icc_profile``: bytes of an iCCP chunk.  ``ValueError`` for
        anything else, 4-byte layouts included."""
        from .preprocess import _page_layout

        if layout is None:
            layout = _lib.PAGE_GRAY if getattr(page_dev, "ndim", 0) == 2 else _lib.PAGE_RGB
        if layout not in (_lib.PAGE_GRAY, _lib.PAGE_RGB, _lib.PAGE_BGR):
            raise ValueError(f"a PNG file is written from a GRAY, RGB or BGR page, not layout {layout!r}")
        H, W, pitch, _ = _page_layout(self, page_dev, (layout,))
        icc = bytes(icc_profile) if icc_profile else b""
        cap = int(self._lib.bbocr_png_encode_bound(H, W, _lib.PAGE_PX_BYTES[layout], len(icc)))
        if cap == 0:
            raise ValueError("the page or the profile is too large for a PNG file")
        out = np.empty(cap, np.uint8)                                   # (untouched pages of it cost nothing)
        n = C.c_size_t()
        self._torch.cuda.current_stream(self.device_index).synchronize()      # the library runs on its own stream
        self._check(self._lib.bbocr_png_encode(self._h, C.c_void_p(page_dev.data_ptr()), H, W, pitch, int(layout),
                                               C.cast(C.c_char_p(icc), C.c_void_p) if icc else None, len(icc), C.c_void_p(out.ctypes.data), cap,
                                               C.byref(n)))
        return out[:n.value].tobytes()

    def decode_png_batch(self, pages):
        """``PngPage`` s of ONE shape -> ``((rgb, gray), status)``: the device tensors ``uint8 [n,H,W,3]`` and ``[n,H,W]`` that ``decode_file``
        + upload would hold, written by ONE ``bbocr_png_decode`` call (only the files' IDAT payloads cross the link), and the per-file
        status list (0, or negative: that page of both tensors is undefined)."""
        torch = self._torch
        pages = list(pages)
        if not pages or any(p.shape != pages[0].shape for p in pages):
            raise ValueError("decode_png_batch: pages of one decoded shape")
        H, W, _ = pages[0].shape
        n = len(pages)
        rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
        gray = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        status = self._png_decode_into(pages, [rgb.data_ptr() + k * H * W * 3 for k in range(n)], [W * 3] * n,
                                       [gray.data_ptr() + k * H * W for k in range(n)], [W] * n)
        return (rgb, gray), status

    def _png_decode_into(self, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches):
        """``bbocr_png_decode`` of the pages into the given device addresses and row pitches -> the per-file status list"""
        n = len(pages)
        files, sizes = self._jpeg_files(pages)
        status = (C.c_int * n)()
        self._torch.cuda.current_stream(self.device_index).synchronize()      # the library runs on its own stream
        self._check(self._lib.bbocr_png_decode(self._h, files, sizes, n, (C.c_void_p * n)(*rgb_ptrs), (C.c_longlong * n)(*rgb_pitches),
                                               (C.c_void_p * n)(*gray_ptrs), (C.c_longlong * n)(*gray_pitches), status))
        return list(status)

    def decode_png_device(self, sources):
        """Paths or bytes objects -> per source ``(rgb_dev [H,W,3], gray_dev [H,W])`` as ``decode_file`` defines them, decoded on the card,
        or ``None`` for a file the plan refuses or whose data is damaged.  Files of one shape share one decode call."""
        pages = [png_page(s) for s in sources]
        out = [None] * len(pages)
        groups = {}
        for i, p in enumerate(pages):
            if p is not None:
                groups.setdefault(p.shape, []).append(i)
        for idxs in groups.values():
            (rgb, gray), status = self.decode_png_batch([pages[i] for i in idxs])
            for k, i in enumerate(idxs):
                if status[k] == 0:
                    out[i] = (rgb[k], gray[k])
        return out

    def png_decode_stage(self, source, stage):
        """``bbocr_op_png_decode_stage`` of one file (path or bytes) -> ``(array, file status)``: stage 0 the inflated stream ``uint8
        [H * (1 + row_bytes)]``, 1 the unfiltered scanlines (same size), 2 ``(rgb [H,W,3], gray [H,W])``"""
        torch = self._torch
        data = _file_bytes(source)
        plan = png_plan(data)
        if not plan.supported or stage not in (0, 1, 2):
            raise ValueError("png_decode_stage: a file the plan supports and stage 0, 1 or 2")
        H, W = int(plan.height), int(plan.width)
        nb = H * (1 + int(plan.row_bytes)) if stage < 2 else 4 * H * W
        out = torch.empty(nb, dtype=torch.uint8, device=self.device)
        st = C.c_int()
        torch.cuda.current_stream(self.device_index).synchronize()
        self._check(self._lib.bbocr_op_png_decode_stage(self._h, data, len(data), stage, C.c_void_p(out.data_ptr()), nb, C.byref(st)))
        a = out.cpu().numpy()
        if stage < 2:
            return a, st.value
        return (a[:3 * H * W].reshape(H, W, 3), a[3 * H * W:].reshape(H, W)), st.value

    def decode_tiff_batch(self, pages):
        """``TiffPage`` s of ONE shape -> ``((rgb, gray), status)``: the device tensors ``uint8 [n,H,W,3]`` and ``[n,H,W]`` that ``decode_file``
        + upload would hold, written by ONE ``bbocr_tiff_decode`` call (only the files' strips cross the link), and the per-file status list
        (0, or negative: that page of both tensors is undefined).  The files may differ in codec, strips, depth and interpretation."""
        torch = self._torch
        pages = list(pages)
        if not pages or any(p.shape != pages[0].shape for p in pages):
            raise ValueError("decode_tiff_batch: pages of one decoded shape")
        H, W, _ = pages[0].shape
        n = len(pages)
        rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
        gray = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        status = self._tiff_decode_into(pages, [rgb.data_ptr() + k * H * W * 3 for k in range(n)], [W * 3] * n,
                                        [gray.data_ptr() + k * H * W for k in range(n)], [W] * n)
        return (rgb, gray), status

    def decode_tiff_pages(self, pages):
        """``TiffPage`` s of ANY shapes -> ``([(rgb [H,W,3], gray [H,W])], status)``: ONE ``bbocr_tiff_decode`` call for all of them, each
        page into tensors of its own; a page of non-zero status holds undefined pixels"""
        torch = self._torch
        pages = list(pages)
        if not pages:
            raise ValueError("decode_tiff_pages: at least one page")
        out = [(torch.empty(p.shape, dtype=torch.uint8, device=self.device), torch.empty(p.shape[:2], dtype=torch.uint8, device=self.device))
               for p in pages]
        status = self._tiff_decode_into(pages, [a.data_ptr() for a, _ in out], [3 * p.shape[1] for p in pages],
                                        [g.data_ptr() for _, g in out], [p.shape[1] for p in pages])
        return out, status

    def _tiff_decode_into(self, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches):
        """``bbocr_tiff_decode`` of the pages -- ``bbocr_tiff_decode_fax`` when one of them is a CCITT page (``TiffPage.fax``) -- into the
        given device addresses and row pitches -> the per-file status list"""
        n = len(pages)
        files, sizes = self._jpeg_files(pages)
        status = (C.c_int * n)()
        self._torch.cuda.current_stream(self.device_index).synchronize()      # the library runs on its own stream
        call = self._lib.bbocr_tiff_decode_fax if any(getattr(p, "fax", False) for p in pages) else self._lib.bbocr_tiff_decode
        self._check(call(self._h, files, sizes, n, (C.c_void_p * n)(*rgb_ptrs), (C.c_longlong * n)(*rgb_pitches),
                   (C.c_void_p * n)(*gray_ptrs), (C.c_longlong * n)(*gray_pitches), status))
        return list(status)

    def decode_tiff_device(self, sources, fax=None):
        """Paths or bytes objects -> per source ``(rgb_dev [H,W,3], gray_dev [H,W])`` as ``decode_file`` defines them, decoded on the card,
        or ``None`` for a file the plan refuses or whose data is damaged.  All the files share one decode call.  ``fax`` (None: the
        Reader's ``tiff_decode`` is ``"fax"``): CCITT files as well."""
        fax = tiff_fax(getattr(self, "tiff_decode", False)) if fax is None else bool(fax)
        pages = [tiff_page(s, fax) for s in sources]
        out = [None] * len(pages)
        idxs = [i for i, p in enumerate(pages) if p is not None]
        if idxs:
            planes, status = self.decode_tiff_pages([pages[i] for i in idxs])
            for k, i in enumerate(idxs):
                if status[k] == 0:
                    out[i] = planes[k]
        return out

    def tiff_fax_decode_stage(self, source, stage):
        """``bbocr_op_tiff_fax_decode_stage``: ``tiff_decode_stage`` for the files ``tiff_fax_plan`` supports, CCITT files among them"""
        return self.tiff_decode_stage(source, stage, fax=True)

    def tiff_decode_stage(self, source, stage, fax=False):
        """``bbocr_op_tiff_decode_stage`` of one file (path or bytes) -> ``(array, file status)``: stage 0 the strips' decoded stream
        ``uint8 [H * row_bytes]``, 1 the same after the predictor, 2 ``(rgb [H,W,3], gray [H,W])``"""
        torch = self._torch
        data = _file_bytes(source)
        plan = tiff_fax_plan(data)[0] if fax else tiff_plan(data)
        if not plan.supported or stage not in (0, 1, 2):
            raise ValueError("tiff_decode_stage: a file the plan supports and stage 0, 1 or 2")
        H, W = int(plan.height), int(plan.width)
        nb = H * int(plan.row_bytes) if stage < 2 else 4 * H * W
        out = torch.empty(nb, dtype=torch.uint8, device=self.device)
        st = C.c_int()
        torch.cuda.current_stream(self.device_index).synchronize()
        call = self._lib.bbocr_op_tiff_fax_decode_stage if fax else self._lib.bbocr_op_tiff_decode_stage
        self._check(call(self._h, data, len(data), stage, C.c_void_p(out.data_ptr()), nb, C.byref(st)))
        a = out.cpu().numpy()
        if stage < 2:
            return a, st.value
        return (a[:3 * H * W].reshape(H, W, 3), a[3 * H * W:].reshape(H, W)), st.value

    def _decode_pages_into(self, call, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches):
        """``call`` (``bbocr_gif_decode``'s signature) of the pages into the given device addresses and row pitches -> the per-file status list"""
        n = len(pages)
        files, sizes = self._jpeg_files(pages)
        status = (C.c_int * n)()
        self._torch.cuda.current_stream(self.device_index).synchronize()      # the library runs on its own stream
        self._check(call(self._h, files, sizes, n, (C.c_void_p * n)(*rgb_ptrs), (C.c_longlong * n)(*rgb_pitches), (C.c_void_p * n)(*gray_ptrs),
                         (C.c_longlong * n)(*gray_pitches), status))
        return list(status)

    def _decode_pages(self, into, pages, name):
        torch = self._torch
        pages = list(pages)
        if not pages:
            raise ValueError(f"{name}: at least one page")
        out = [(torch.empty(p.shape, dtype=torch.uint8, device=self.device), torch.empty(p.shape[:2], dtype=torch.uint8, device=self.device))
               for p in pages]
        status = into(pages, [a.data_ptr() for a, _ in out], [3 * p.shape[1] for p in pages], [g.data_ptr() for _, g in out],
                      [p.shape[1] for p in pages])
        return out, status

    def _decode_sources(self, page_of, decode_pages, sources):
        pages = [page_of(s) for s in sources]
        out = [None] * len(pages)
        idxs = [i for i, p in enumerate(pages) if p is not None]
        if idxs:
            planes, status = decode_pages([pages[i] for i in idxs])
            for k, i in enumerate(idxs):
                if status[k] == 0:
                    out[i] = planes[k]
        return out

    def _gif_decode_into(self, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches):
        """``bbocr_gif_decode`` of the pages into the given device addresses and row pitches -> the per-file status list"""
        return self._decode_pages_into(self._lib.bbocr_gif_decode, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches)

    def decode_gif_pages(self, pages):
        """``GifPage`` s of ANY shapes -> ``([(rgb [H,W,3], gray [H,W])], status)``: ONE ``bbocr_gif_decode`` call for all of them (only the
        files' LZW payloads and tables cross the link), each page into tensors of its own; a page of non-zero status holds undefined pixels"""
        return self._decode_pages(self._gif_decode_into, pages, "decode_gif_pages")

    def decode_gif_device(self, sources):
        """Paths or bytes objects -> per source ``(rgb_dev [H,W,3], gray_dev [H,W])`` as ``decode_file`` defines them, decoded on the card,
        or ``None`` for a file the plan refuses or whose data is damaged.  All the files share one decode call."""
        return self._decode_sources(gif_page, self.decode_gif_pages, sources)

    def _bmp_decode_into(self, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches):
        """``bbocr_bmp_decode`` of the pages into the given device addresses and row pitches -> the per-file status list"""
        return self._decode_pages_into(self._lib.bbocr_bmp_decode, pages, rgb_ptrs, rgb_pitches, gray_ptrs, gray_pitches)

    def decode_bmp_pages(self, pages):
        """``BmpPage`` s of ANY shapes -> ``([(rgb [H,W,3], gray [H,W])], status)``: ONE ``bbocr_bmp_decode`` call -- one launch -- for all of
        them, each page into tensors of its own; a page of non-zero status (an argument error) holds undefined pixels"""
        return self._decode_pages(self._bmp_decode_into, pages, "decode_bmp_pages")

    def decode_bmp_device(self, sources):
        """Paths or bytes objects -> per source ``(rgb_dev [H,W,3], gray_dev [H,W])`` as ``decode_file`` defines them, decoded on the card,
        or ``None`` for a file the plan refuses.  All the files share one decode call."""
        return self._decode_sources(bmp_page, self.decode_bmp_pages, sources)

    def gif_decode_stage(self, source, stage):
        """``bbocr_op_gif_decode_stage`` of one file (path or bytes) -> ``(bytes, file status)``: stage 0 the piece table (a 16-byte head --
        count, the scan's error bits -- and 16 bytes per piece: first bit low / high, data codes, end), 1 ``uint32`` offsets per piece and
        the total, 2 the index stream in stored row order, ``width * height`` bytes"""
        torch = self._torch
        data = _file_bytes(source)
        plan = gif_plan(data)
        if not plan.supported or stage not in (0, 1, 2):
            raise ValueError("gif_decode_stage: a file the plan supports and stage 0, 1 or 2")
        room = int(self._lib.bbocr_gif_piece_room(int(plan.payload_bytes), int(plan.min_code)))
        st = C.c_int()

        def run(stage, nb):
            out = torch.empty(nb, dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device_index).synchronize()
            self._check(self._lib.bbocr_op_gif_decode_stage(self._h, data, len(data), stage, C.c_void_p(out.data_ptr()), nb, C.byref(st)))
            return out.cpu().numpy()

        if stage == 2:
            return run(2, int(plan.width) * int(plan.height)).tobytes(), st.value
        head = run(0, 16 + 16 * room)
        count = int(head[:4].view(np.uint32)[0])
        if stage == 0:
            return head[:16 + 16 * count].tobytes(), st.value
        return run(1, 4 * (room + 1))[:4 * (count + 1)].tobytes(), st.value

    def deflate_device(self, bytes_dev):
        """A contiguous 1-D uint8 device tensor -> the zlib stream ``bbocr_op_deflate`` makes of it (the PNG writer's chunks, run matches and
        dynamic Huffman codes); ``zlib.decompress`` gives the bytes back."""
        torch = self._torch
        if not isinstance(bytes_dev, torch.Tensor) or bytes_dev.dtype != torch.uint8 or bytes_dev.ndim != 1 or not bytes_dev.is_contiguous():
            raise ValueError("expected a contiguous 1-D uint8 device tensor")
        if not bytes_dev.is_cuda or bytes_dev.device.index != self.device_index:
            raise ValueError(f"expected a tensor on {self.device}")
        nb = int(bytes_dev.numel())
        cap = 2 + -(-nb // _lib.PNG_CHUNK) * 5 + nb + 6
        out = np.empty(cap, np.uint8)
        n = C.c_size_t()
        torch.cuda.current_stream(self.device_index).synchronize()
        self._check(self._lib.bbocr_op_deflate(self._h, C.c_void_p(bytes_dev.data_ptr()) if nb else None, nb, C.c_void_p(out.ctypes.data), cap,
                                               C.byref(n)))
        return out[:n.value].tobytes()

    @property
    def decode_option(self):
        """This Reader's ``device_decode`` as the functions of ``extractor_batch`` and ``preprocess`` take it: ``"progressive"``,
        ``"chroma"``, True or False"""
        return DECODE_PROGRESSIVE if self.jpeg_progressive else DECODE_CHROMA if self.jpeg_chroma else self.device_decode

    @staticmethod
    def jpeg_progressive_plan(source):
        """``jpeg_progressive_plan`` of a path or a bytes object: the plan of a multi-scan file, its script included (no GPU)"""
        return jpeg_progressive_plan(_file_bytes(source))

    def decode_jpeg_device(self, sources, chroma=None, scale=1, progressive=None):
        """Paths or bytes objects -> per source ``(rgb_dev [H,W,3], gray_dev [H,W])`` as ``decode_file`` defines them (libjpeg's RGB and its Y
        plane; a grey file: the samples, replicated for RGB), decoded on the card, or ``None`` for a file the plan refuses or whose
        entropy-coded data is damaged.  Files of one decoded shape share one decode call.  ``chroma`` (None: this Reader's
        ``jpeg_chroma``): 4:4:4, 4:2:2 and 4:4:0 files are decoded as well.  ``scale`` 2, 4 or 8: the decode at that fraction (Pillow's
        ``draft``: ``ceil(H / scale) x ceil(W / scale)``), of 4:2:0 and grey files only -- every other file is ``None``.  ``progressive``
        (None: this Reader's ``jpeg_progressive``): progressive files are decoded as well, of every sampling at every scale."""
        progressive = self.jpeg_progressive if progressive is None else bool(progressive)   # such files are decoded too, at every scale
        chroma = (self.jpeg_chroma if chroma is None else bool(chroma)) and scale == 1
        pages = [jpeg_page(s, chroma, progressive) for s in sources]
        out = [None] * len(pages)
        groups = {}
        for i, p in enumerate(pages):
            if p is not None:
                groups.setdefault(p.shape, []).append(i)
        for idxs in groups.values():
            t, status = self.decode_jpeg_batch([pages[i] for i in idxs], scale=scale)
            rgb, gray = self.pages_from_jpeg(t)
            for k, i in enumerate(idxs):
                if status[k] == 0:
                    out[i] = (rgb[k], gray[k])
        return out

    def jpeg_counters(self):
        """``bbocr_jpeg_counters``: this Reader's totals since it was made, per file of every JPEG batch -- ``{"files", "entropy_runs",
        "idct_passes", "output_passes"}``.  A ``decode_jpeg_scales`` call with two scales adds 1, 1, 2, 2 per file."""
        out = (C.c_longlong * 4)()
        self._check(self._lib.bbocr_jpeg_counters(self._h, out))
        return dict(zip(("files", "entropy_runs", "idct_passes", "output_passes"), (int(v) for v in out)))

    def decode_jpeg_scales_batch(self, pages, scales, imread=False):
        """``JpegPage`` s of any shapes -> ``(decodes, status)`` by ONE ``bbocr_jpeg_decode_scales`` call: the entropy stages run once per
        file, then one IDCT + output pass per scale.  ``decodes[k]`` maps each scale to the decoder's own device tensor -- ``uint8
        [oh,ow,4]`` Pillow's padded YCbCr pixels (``pages_from_ycc``'s input) or ``[oh,ow]`` for a 1-component file, ``oh, ow = ceil(. /
        scale)`` -- and, with ``imread``, scale 1 to ``cv2.imread``'s oriented BGR page (``imread_jpeg_batch``'s).  Files of a chroma class are
        decoded at every scale.  ``status[k]`` non-zero: that file's tensors are undefined."""
        torch = self._torch
        pages = list(pages)
        scales = tuple(int(s) for s in scales)
        if not pages or not scales or len(set(scales)) != len(scales) or any(s not in JPEG_SCALES for s in scales):
            raise ValueError(f"decode_jpeg_scales_batch: pages, and different scales out of {JPEG_SCALES}")
        if imread and 1 not in scales:
            raise ValueError("imread: the oriented page exists at scale 1 only")
        n = len(pages)
        outs = (_lib.bbocr_jpeg_output * len(scales))()
        decodes = [{} for _ in pages]
        keep = []
        for o, s in enumerate(scales):
            form = _lib.JPEG_FORM_IMREAD if imread and s == 1 else _lib.JPEG_FORM_YCBCR
            ts = []
            for p in pages:
                H, W, comps = p.shape
                if form == _lib.JPEG_FORM_IMREAD:
                    shape = (W, H, 3) if p.orientation >= 5 else (H, W, 3)
                else:
                    shape = (-(-H // s), -(-W // s)) + ((4,) if comps == 3 else ())
                ts.append(torch.empty(shape, dtype=torch.uint8, device=self.device))
            ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
            pitches = (C.c_longlong * n)(*[t.shape[1] * (t.shape[2] if t.ndim == 3 else 1) for t in ts])
            keep.append((ptrs, pitches))
            outs[o].scale, outs[o].form, outs[o].dev_out, outs[o].pitches = s, form, ptrs, pitches
            for k, t in enumerate(ts):
                decodes[k][s] = t
        torch.cuda.current_stream(self.device_index).synchronize()
        files, sizes = self._jpeg_files(pages)
        status = (C.c_int * n)()
        call = self._lib.bbocr_jpeg_decode_progressive if any(p.progressive for p in pages) else self._lib.bbocr_jpeg_decode_scales
        self._check(call(self._h, files, sizes, n, _lib.PAGE_YCBCR4, outs, len(scales), status))
        del keep
        return decodes, list(status)

    def decode_jpeg_scales(self, sources, scales=(1, 2), chroma=None, imread=False, progressive=None):
        """Paths or bytes objects -> per source ``{scale: pages}``, or ``None`` for a file the plan refuses or whose entropy-coded data is
        damaged -- all scales of all files from ONE device call that runs the entropy stages once per file (``decode_jpeg_device`` called
        once per scale runs them once per scale).  ``pages`` is ``(rgb_dev [oh,ow,3], gray_dev [oh,ow])`` as ``decode_jpeg_device`` defines
        them, ``oh, ow = ceil(. / scale)``; with ``imread`` the scale-1 entry is ``cv2.imread``'s page instead: BGR ``[H',W',3]``, EXIF
        orientation applied.  ``chroma`` (None: this Reader's ``jpeg_chroma``): 4:4:4, 4:2:2 and 4:4:0 files are decoded as well -- here at
        EVERY scale, where ``decode_jpeg_device(scale=2)`` leaves them to the host."""
        chroma = self.jpeg_chroma if chroma is None else bool(chroma)
        progressive = self.jpeg_progressive if progressive is None else bool(progressive)     # progressive files are decoded as well
        pages = [jpeg_page(s, chroma, progressive) for s in sources]
        out = [None] * len(pages)
        idxs = [i for i, p in enumerate(pages) if p is not None]
        if not idxs:
            return out
        decodes, status = self.decode_jpeg_scales_batch([pages[i] for i in idxs], scales, imread=imread)
        for k, i in enumerate(idxs):
            if status[k] != 0:
                continue
            out[i] = {}
            for s, t in decodes[k].items():
                out[i][s] = t if imread and s == 1 else tuple(x[0] for x in self.pages_from_jpeg(t[None]))
        return out

    def readtext_ycc_arrays(self, ycc, **kw):
        """Host array ``uint8 [B,H,W,3]`` of once-decoded JPEG pages (``decode_file_ycc``) -> per-page results, identical to
        ``readtext_arrays(rgb, gray)`` of the same files decoded twice."""
        if not isinstance(ycc, (list, tuple)):               # a list of [H,W,3] pages is uploaded page by page (Reader._to_dev)
            ycc = np.asarray(ycc)
            if ycc.dtype != np.uint8 or ycc.ndim != 4 or ycc.shape[3] not in (3, 4):
                raise ValueError("readtext_ycc_arrays expects uint8 [B,H,W,3] (or [B,H,W,4]: Pillow's padded pixels)")
        rgb, gray = self.pages_from_ycc(self._to_dev(ycc))
        return self.readtext_device(rgb, gray, **kw)

    def _stream(self, submit, batches, in_flight):
        """``submit(executor, batch) -> future`` for every batch, results IN ORDER, ``in_flight`` calls running and one batch queued behind
        them: the one loop of ``readtext_stream`` and ``readtext_pages_stream``.  A lazy producer (H2D copies) is drained no further
        ahead than that, so at most ``in_flight + 1`` batches are resident on the card, and each result is yielded as soon as it is next."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        in_flight = max(1, int(in_flight))
        with ThreadPoolExecutor(max_workers=in_flight, thread_name_prefix="bbocr-call") as ex:
            pending = deque()
            for b in batches:
                pending.append(submit(ex, b))
                if len(pending) > in_flight:                 # one batch queued behind the running ones: a worker never waits for the producer
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    def readtext_stream(self, batches, in_flight=2, **kw):
        """Device page batches in, per-batch results out, IN ORDER, with up to ``in_flight`` calls running on this Reader at once.

        The reference shares one Reader between ``ThreadPoolExecutor`` workers (batch_processor_enhanced.py:215, default 2); libbbocr gives
        each concurrent call its own call slot (``bbocr_config::call_slots``), so batch k+1's detector is on the card while batch k's host
        thread finishes box geometry, CTC read-back and result marshalling.  ``batches`` yields uint8 ``[B,H,W,3]`` device tensors or
        ``(rgb, gray)`` pairs (it may produce them lazily, e.g. H2D copies: it is drained one batch ahead of the workers).  Results are those
        of calling ``readtext_device`` batch by batch."""

        def submit(ex, b):
            rgb, gray = b if isinstance(b, tuple) else (b, None)
            return ex.submit(self.readtext_device, rgb, gray, **kw)

        return self._stream(submit, batches, in_flight)

    def readtext_pages_stream(self, batches, in_flight=2, **kw):
        """``readtext_stream`` for pages of mixed shapes: ``batches`` yields page LISTS as ``readtext_pages`` takes them (it may produce them
        lazily, drained one batch ahead of the workers, as there), each list is one ``readtext_pages`` call, and the results are those of
        calling it list by list, in order."""
        return self._stream(lambda ex, b: ex.submit(self.readtext_pages, b, **kw), batches, in_flight)

    def readtext(self, image, decoder="greedy", beamWidth=5, batch_size=1, workers=0, allowlist=None, blocklist=None, detail=1,
                 rotation_info=None, paragraph=False, min_size=20, contrast_ths=0.1, adjust_contrast=0.5, filter_ths=0.003,
                 text_threshold=0.7, low_text=0.4, link_threshold=0.4, canvas_size=2560, mag_ratio=1.0, slope_ths=0.1, ycenter_ths=0.5,
                 height_ths=0.5, width_ths=0.5, y_ths=0.5, x_ths=1.0, add_margin=0.1, threshold=0.2, bbox_min_score=0.2, bbox_min_size=3,
                 max_candidates=0, output_format="standard"):
        """``image -> [(bbox, text, confidence)]`` exactly as ``easyocr.Reader.readtext`` shapes it."""
        self._unsupported(decoder, allowlist, blocklist, rotation_info, paragraph, output_format)
        # one page per call is latency-bound: RGB and the Y plane decoded side by side on two threads (4.9 ms) beat the single YCbCr decode
        # (decode_file_ycc, ~5.6 ms on one core) that the throughput-bound callers (extractor_batch) take
        rgb_dev = None
        if self.device_decode and isinstance(image, (str, os.PathLike, bytes, bytearray)):
            dev = self.decode_jpeg_device([image])[0]          # None: refused or damaged -> the host decode below, unchanged
            if dev is not None:
                # a file given as bytes keeps upstream's rule for arrays (the gray plane derived from the colour image), as with the option off
                rgb_dev, gray_dev = dev[0][None], (None if isinstance(image, (bytes, bytearray)) else dev[1][None])
        if rgb_dev is None and self.png_decode and isinstance(image, (str, os.PathLike, bytes, bytearray)):
            dev = self.decode_png_device([image])[0]           # None: not a PNG, refused or damaged -> the host decode below, unchanged
            if dev is not None:
                rgb_dev, gray_dev = dev[0][None], (None if isinstance(image, (bytes, bytearray)) else dev[1][None])
        if rgb_dev is None and self.tiff_decode and isinstance(image, (str, os.PathLike, bytes, bytearray)):
            dev = self.decode_tiff_device([image])[0]          # None: not a TIFF, refused or damaged -> the host decode below, unchanged
            if dev is not None:
                rgb_dev, gray_dev = dev[0][None], (None if isinstance(image, (bytes, bytearray)) else dev[1][None])
        if rgb_dev is None and self.gif_decode and isinstance(image, (str, os.PathLike, bytes, bytearray)):
            dev = self.decode_gif_device([image])[0]           # None: not a GIF, refused or damaged -> the host decode below, unchanged
            if dev is not None:
                rgb_dev, gray_dev = dev[0][None], (None if isinstance(image, (bytes, bytearray)) else dev[1][None])
        if rgb_dev is None and self.bmp_decode and isinstance(image, (str, os.PathLike, bytes, bytearray)):
            dev = self.decode_bmp_device([image])[0]           # None: not a BMP or refused -> the host decode below, unchanged
            if dev is not None:
                rgb_dev, gray_dev = dev[0][None], (None if isinstance(image, (bytes, bytearray)) else dev[1][None])
        if rgb_dev is None:
            img, grey = reformat_input(image, device_gray=True, parallel_decode=True)
            rgb_dev, gray_dev = self._to_dev(img[None]), (self._to_dev(grey[None]) if grey is not None else None)
        kw = dict(min_size=min_size, contrast_ths=contrast_ths, adjust_contrast=adjust_contrast, text_threshold=text_threshold,
                  low_text=low_text, link_threshold=link_threshold, canvas_size=canvas_size, mag_ratio=mag_ratio, slope_ths=slope_ths,
                  ycenter_ths=ycenter_ths, height_ths=height_ths, width_ths=width_ths, add_margin=add_margin, detail=detail,
                  allowlist=allowlist, blocklist=blocklist, paragraph=paragraph, x_ths=x_ths, y_ths=y_ths, decoder=decoder,
                  beamWidth=beamWidth, rotation_info=rotation_info)
        result = self.readtext_device(rgb_dev, gray_dev, **kw)[0]
        return format_output(result, output_format, paragraph, detail)

    def readtext_batched(self, image, n_width=None, n_height=None, mixed=None, **kw):
        """List (or 4-D array) of pages -> list of per-page results.  Equal-size pages share one device batch.  ``mixed`` (None: the
        environment variable ``BBOCR_MIXED_BATCH``, off unless it is ``1``): pages of ANY sizes share device batches -- closed by page count
        and a pixel budget (``mixed_batches``), each read by one ``readtext_pages`` call, two calls in flight; same results."""
        self._unsupported(kw.get("decoder", "greedy"), kw.get("allowlist"), kw.get("blocklist"), kw.get("rotation_info"),
                          kw.get("paragraph", False), kw.get("output_format", "standard"))
        output_format = kw.pop("output_format", "standard")
        for k in ("batch_size", "workers", "filter_ths", "threshold", "bbox_min_score", "bbox_min_size", "max_candidates"):
            kw.pop(k, None)
        pages = [reformat_input(im) for im in image]
        if n_width is not None and n_height is not None:
            from PIL import Image

            pages = [(np.asarray(Image.fromarray(a).resize((n_width, n_height), Image.BILINEAR)),
                      np.asarray(Image.fromarray(g).resize((n_width, n_height), Image.BILINEAR))) for a, g in pages]
        out = [None] * len(pages)
        max_pages = int(os.environ.get("BBOCR_MAX_DEVICE_BATCH", "64"))     # pages per device batch; larger groups stream, two batches in flight
        if mixed_batch_enabled(mixed):
            chunks = mixed_batches([a.shape[0] * a.shape[1] for a, _ in pages], max_pages)
            feed = ([(self._to_dev(pages[i][0]), self._to_dev(pages[i][1])) for i in ch] for ch in chunks)
            for ch, res in zip(chunks, self.readtext_pages_stream(feed, **kw)):
                for i, r in zip(ch, res):
                    out[i] = format_output(r, output_format, kw.get("paragraph", False), kw.get("detail", 1))
            return out
        by_shape = {}
        for i, (a, g) in enumerate(pages):
            by_shape.setdefault(a.shape, []).append(i)
        for _, idxs in by_shape.items():
            chunks = [idxs[k:k + max_pages] for k in range(0, len(idxs), max_pages)]
            # (lists: the pages reach the card in one upload call per batch, without a host-side np.stack)
            feed = ((self._to_dev([pages[i][0] for i in ch]), self._to_dev([pages[i][1] for i in ch])) for ch in chunks)
            for ch, res in zip(chunks, self.readtext_stream(feed, **kw)):
                for i, r in zip(ch, res):
                    out[i] = format_output(r, output_format, kw.get("paragraph", False), kw.get("detail", 1))
        return out

    def readtext_files(self, paths, max_batch=64, decode_workers=None, **kw):
        """Image FILES in, ``Reader.readtext(path)``'s result per file out (same order), through the decode pool / upload stage / two device
        batches in flight of ``extractor_batch.read_files``: JPEG files are decoded once (YCbCr triples), pages of one size share device
        batches -- with ``mixed=True`` (None: ``BBOCR_MIXED_BATCH``) pages of any sizes do.  A file that cannot be decoded or read maps to ``[]``."""
        from .extractor_batch import read_files

        paths = list(paths)
        kw.setdefault("device_decode", self.decode_option)
        res = read_files(self, paths, None, max_batch, decode_workers, **kw)
        return [res[i] for i in range(len(paths))]

    def readtext_arrays(self, rgb, gray=None, **kw):
        """Host arrays ``uint8 [B,H,W,3]`` (+ optional ``[B,H,W]`` gray planes, else derived on device) -> per-page results."""
        if isinstance(rgb, (list, tuple)):                   # lists of [H,W,3] (+ [H,W]) pages: uploaded page by page (Reader._to_dev)
            if gray is not None and len(gray) != len(rgb):
                raise ValueError("readtext_arrays: one gray plane per page")
            return self.readtext_device(self._to_dev(rgb), self._to_dev(gray) if gray is not None else None, **kw)
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3:
            raise ValueError("readtext_arrays expects uint8 [B,H,W,3]")
        if gray is not None and (np.asarray(gray).dtype != np.uint8 or np.asarray(gray).shape != rgb.shape[:3]):
            raise ValueError("readtext_arrays: gray must be uint8 [B,H,W] matching rgb")
        return self.readtext_device(self._to_dev(rgb), self._to_dev(np.asarray(gray)) if gray is not None else None, **kw)

    def detect(self, img, min_size=20, text_threshold=0.7, low_text=0.4, link_threshold=0.4, canvas_size=2560, mag_ratio=1.0,
               slope_ths=0.1, ycenter_ths=0.5, height_ths=0.5, width_ths=0.5, add_margin=0.1, reformat=True, **_ignored):
        """``Reader.detect`` -> (horizontal_list_agg, free_list_agg) for one page."""
        if reformat:
            img, _ = reformat_input(img)
        kw = dict(min_size=min_size, text_threshold=text_threshold, low_text=low_text, link_threshold=link_threshold,
                  canvas_size=canvas_size, mag_ratio=mag_ratio, slope_ths=slope_ths, ycenter_ths=ycenter_ths, height_ths=height_ths,
                  width_ths=width_ths, add_margin=add_margin)
        heat, ratio = self.heatmap_device(self._to_dev(img[None]), **kw)
        h, f, _ = self.boxes_from_heatmap(heat, ratio, **kw)
        return [h[0]], [f[0]]

    def recognize(self, img_cv_grey, horizontal_list=None, free_list=None, decoder="greedy", beamWidth=5, detail=1, paragraph=False,
                  contrast_ths=0.1, adjust_contrast=0.5, reformat=True, rotation_info=None, allowlist=None, blocklist=None, y_ths=0.5, x_ths=1.0,
                  output_format="standard", **_ignored):
        """``Reader.recognize`` for explicit boxes of one gray page (``paragraph=True``: ``get_paragraph`` on the result, like upstream)."""
        self._unsupported(decoder, None, None, None, False, output_format)
        if paragraph:
            raw = self.recognize(img_cv_grey, horizontal_list, free_list, decoder=decoder, beamWidth=beamWidth, detail=1, paragraph=False,
                                 contrast_ths=contrast_ths, adjust_contrast=adjust_contrast, reformat=reformat, rotation_info=rotation_info,
                                 allowlist=allowlist, blocklist=blocklist)
            para = get_paragraph(raw, x_ths=x_ths, y_ths=y_ths, mode="ltr")
            return [item[1] for item in para] if detail == 0 else format_output(para, output_format, True, detail)
        if reformat:
            _, img_cv_grey = reformat_input(img_cv_grey)
        H, W = img_cv_grey.shape
        if horizontal_list is None and free_list is None:
            horizontal_list, free_list = [[0, W, 0, H]], []
        res = self.recognize_device(self._to_dev(img_cv_grey[None]), [horizontal_list or []], [free_list or []],
                                    contrast_ths=contrast_ths, adjust_contrast=adjust_contrast, detail=detail, decoder=decoder,
                                    beamWidth=beamWidth, rotation_info=rotation_info, allowlist=allowlist, blocklist=blocklist)[0]
        return format_output(res, output_format, False, detail)

    # -- stage-level entry points (tests, bench) --------------------------------------------
    def detect_dims(self, H, W, canvas_size=2560, mag_ratio=1.0):
        v = [C.c_int() for _ in range(4)]
        ratio = C.c_double()
        rc = self._lib.bbocr_detect_dims(H, W, canvas_size, float(mag_ratio), *[C.byref(x) for x in v], C.byref(ratio))
        if rc != 0:
            raise ValueError("bad page size")
        return v[0].value, v[1].value, v[2].value, v[3].value, ratio.value

    def heatmap_device(self, rgb_dev, **kw):
        """uint8 [B,H,W,3] device tensor -> (fp32 [B,h,w,2] device tensor, ratio)."""
        self._dev_u8(rgb_dev, "rgb", 4)
        B, H, W, ch = rgb_dev.shape
        if ch != 3:
            raise ValueError(f"rgb: last dimension must be 3, got {ch}")
        _, _, h, w, ratio = self.detect_dims(H, W, kw.get("canvas_size", 2560), kw.get("mag_ratio", 1.0))
        heat = self._torch.empty((B, h, w, 2), dtype=self._torch.float32, device=self.device)
        p = self._params(kw)
        self._check(self._lib.bbocr_detect(self._h, C.c_void_p(rgb_dev.data_ptr()), B, H, W, C.byref(p), C.c_void_p(heat.data_ptr())))
        return heat, ratio

    def boxes_from_heatmap(self, heat_dev, ratio, **kw):
        """fp32 [B,h,w,2] device tensor -> (horizontal lists, free lists, polys) per page."""
        torch = self._torch
        if (not isinstance(heat_dev, torch.Tensor) or not heat_dev.is_cuda or heat_dev.device.index != self.device_index
                or heat_dev.dtype != torch.float32 or heat_dev.ndim != 4 or heat_dev.shape[3] != 2 or not heat_dev.is_contiguous()):
            raise ValueError(f"heat-map: expected a contiguous float32 [B,h,w,2] tensor on {self.device}")
        B, h, w, _ = heat_dev.shape
        p = self._params(kw)
        bl = C.POINTER(_lib.bbocr_boxlist)()
        self._check(self._lib.bbocr_boxes(self._h, C.c_void_p(heat_dev.data_ptr()), B, h, w, float(ratio), C.byref(p), C.byref(bl)))
        try:
            b = bl.contents
            hori = [[[b.hori[i * 4 + k] for k in range(4)] for i in range(b.hori_off[n], b.hori_off[n + 1])] for n in range(B)]
            free = [[[[b.free_q[i * 8 + 2 * k], b.free_q[i * 8 + 2 * k + 1]] for k in range(4)]
                     for i in range(b.free_off[n], b.free_off[n + 1])] for n in range(B)]
            polys = [[[b.polys[i * 8 + k] for k in range(8)] for i in range(b.poly_off[n], b.poly_off[n + 1])] for n in range(B)]
        finally:
            self._lib.bbocr_free_boxlist(bl)
        return hori, free, polys

    def ctc_beam_device(self, probs_dev, seqs, beam_width, C=97):
        """The device beam search alone (bbocr_op_ctc_beam): fp32 [rows, cs] device tensor of probabilities, seqs = [(first row, T)], width
        <= _lib.BEAM_DEVICE_MAX -> one list of class indices per sequence (ctcBeamSearch's text, blank and repeats dropped).  C <= 128: the
        kernel keeps labels as bytes; a wider model's beam search runs on the host, or through ctc_beam_wide_device's kernels (beam_wide)."""
        import ctypes as ct             # the argument C (classes, as in bbocr.h) hides the module's alias here

        if int(C) > 128:
            raise ValueError("the device beam search takes at most 128 classes")

        torch = self._torch
        if (not isinstance(probs_dev, torch.Tensor) or not probs_dev.is_cuda or probs_dev.device.index != self.device_index
                or probs_dev.dtype != torch.float32 or probs_dev.ndim != 2 or not probs_dev.is_contiguous()):
            raise ValueError(f"probabilities: expected a contiguous float32 [rows,cs] tensor on {self.device}")
        flat = [int(v) for s in seqs for v in s]
        n = len(flat) // 2
        tab = (ct.c_int * max(len(flat), 1))(*flat)
        off = (ct.c_int * (n + 1))()
        idx = (ct.c_int * max(1, sum(max(t, 0) for t in flat[1::2])))()
        self._check(self._lib.bbocr_op_ctc_beam(self._h, ct.c_void_p(probs_dev.data_ptr()), probs_dev.shape[0], tab, n, int(C),
                                                probs_dev.shape[1], int(beam_width), off, idx))
        return [idx[off[i]:off[i + 1]] for i in range(n)]

    def ctc_wordbeam_device(self, probs_dev, seqs, beam_width, C=97):
        """The device word beam search alone (bbocr_op_ctc_wordbeam) over this Reader's dictionary: arguments and result as
        ctc_beam_device's; the text equals bbocr_host_ctc_wordbeam's on the same rows."""
        import ctypes as ct

        torch = self._torch
        if (not isinstance(probs_dev, torch.Tensor) or not probs_dev.is_cuda or probs_dev.device.index != self.device_index
                or probs_dev.dtype != torch.float32 or probs_dev.ndim != 2 or not probs_dev.is_contiguous()):
            raise ValueError(f"probabilities: expected a contiguous float32 [rows,cs] tensor on {self.device}")
        flat = [int(v) for s in seqs for v in s]
        n = len(flat) // 2
        tab = (ct.c_int * max(len(flat), 1))(*flat)
        off = (ct.c_int * (n + 1))()
        idx = (ct.c_int * max(1, sum(max(t, 0) for t in flat[1::2])))()
        self._check(self._lib.bbocr_op_ctc_wordbeam(self._h, ct.c_void_p(probs_dev.data_ptr()), probs_dev.shape[0], tab, n, int(C),
                                                    probs_dev.shape[1], int(beam_width), off, idx))
        return [idx[off[i]:off[i + 1]] for i in range(n)]

    def word_segments_device(self, idx_dev, seqs, space):
        """The word-group kernel alone (bbocr_op_word_segments): int32 [rows] device tensor of arg-max classes, seqs = [(first row, T)] ->
        per sequence the list of its groups ``(first row, T)``."""
        torch = self._torch
        if (not isinstance(idx_dev, torch.Tensor) or not idx_dev.is_cuda or idx_dev.device.index != self.device_index
                or idx_dev.dtype != torch.int32 or idx_dev.ndim != 1 or not idx_dev.is_contiguous()):
            raise ValueError(f"arg-max rows: expected a contiguous int32 [rows] tensor on {self.device}")
        flat = [int(v) for s in seqs for v in s]
        n = len(flat) // 2
        tab = (C.c_int * max(len(flat), 1))(*flat)
        off = (C.c_int * (n + 1))()
        segs = (C.c_int * max(2, 2 * sum((max(t, 0) + 1) // 2 for t in flat[1::2])))()
        self._check(self._lib.bbocr_op_word_segments(self._h, C.c_void_p(idx_dev.data_ptr()), idx_dev.shape[0], tab, n, int(space), off, segs))
        return [[(segs[2 * k], segs[2 * k + 1]) for k in range(off[i], off[i + 1])] for i in range(n)]

    def dict_lookup_device(self, queries, words=None, n_slots=0):
        """The dictionary lookup alone (bbocr_op_dict_lookup): queries / words = lists of class-index strings -> ([0 / 1 per query], the
        table's longest probe run).  words None: this Reader's dictionary as uploaded; else a table built for the call with n_slots slots
        (0: the default size)."""
        def flat(strings):
            off = np.concatenate([[0], np.cumsum([len(w) for w in strings])]).astype(np.int32)
            sym = np.array([v for w in strings for v in w] or [0], dtype=np.uint16)
            return sym, off

        qs, qo = flat(queries)
        ws, wo = flat(words or [])
        found, probe = (C.c_int * max(1, len(queries)))(), C.c_int(0)
        u16, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int)
        self._check(self._lib.bbocr_op_dict_lookup(self._h, ws.ctypes.data_as(u16), wo.ctypes.data_as(i32), len(words or []), int(n_slots),
                                                   qs.ctypes.data_as(u16), qo.ctypes.data_as(i32), len(queries), found, C.byref(probe)))
        return list(found)[:len(queries)], probe.value

    def ctc_beam_wide_device(self, probs_dev, seqs, beam_width, C):
        """The device beam search over more than 128 classes alone (bbocr_op_ctc_beam_wide), on a Reader of such a model: arguments as
        ctc_beam_device's, 128 < C <= _lib.REC_CLASSES_MAX -> (texts, n_host): one list of class indices per sequence, and the number of
        sequences that had a row of more than 128 candidate classes and were searched on the host."""
        import ctypes as ct             # the argument C (classes, as in bbocr.h) hides the module's alias here

        torch = self._torch
        if (not isinstance(probs_dev, torch.Tensor) or not probs_dev.is_cuda or probs_dev.device.index != self.device_index
                or probs_dev.dtype != torch.float32 or probs_dev.ndim != 2 or not probs_dev.is_contiguous()):
            raise ValueError(f"probabilities: expected a contiguous float32 [rows,cs] tensor on {self.device}")
        flat = [int(v) for s in seqs for v in s]
        n = len(flat) // 2
        tab = (ct.c_int * max(len(flat), 1))(*flat)
        off = (ct.c_int * (n + 1))()
        idx = (ct.c_int * max(1, sum(max(t, 0) for t in flat[1::2])))()
        n_host = ct.c_int(-1)
        self._check(self._lib.bbocr_op_ctc_beam_wide(self._h, ct.c_void_p(probs_dev.data_ptr()), probs_dev.shape[0], tab, n, int(C),
                                                     probs_dev.shape[1], int(beam_width), off, idx, ct.byref(n_host)))
        return [idx[off[i]:off[i + 1]] for i in range(n)], n_host.value

    def recognize_device(self, gray_dev, horizontal_lists, free_lists, **kw):
        self._dev_u8(gray_dev, "gray", 3)
        B, H, W = gray_dev.shape
        if len(horizontal_lists) != B or len(free_lists) != B:
            raise ValueError("one horizontal list and one free list per page")
        n_h = [len(x) for x in horizontal_lists]
        n_f = [len(x) for x in free_lists]
        hoff = (C.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(n_h)]).astype(int).tolist())
        foff = (C.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(n_f)]).astype(int).tolist())
        poff = (C.c_int * (B + 1))()
        hflat = [int(v) for page in horizontal_lists for box in page for v in box]
        fflat = [float(v) for page in free_lists for box in page for pt in box for v in pt]
        harr = (C.c_int * max(1, len(hflat)))(*hflat)
        farr = (C.c_double * max(1, len(fflat)))(*fflat)
        parr = (C.c_int * 8)()
        bl = _lib.bbocr_boxlist(n_images=B, poly_off=poff, polys=parr, hori_off=hoff, hori=harr, free_off=foff, free_q=farr)
        p = self._params(kw)
        res = C.POINTER(_lib.bbocr_result)()
        self._check(self._lib.bbocr_recognize(self._h, C.c_void_p(gray_dev.data_ptr()), B, H, W, C.byref(bl), C.byref(p), C.byref(res)))
        return self._collect(res, kw.get("detail", 1))

    def _unsupported(self, decoder, allowlist, blocklist, rotation_info, paragraph, output_format):
        if decoder not in ("greedy", "beamsearch") and not (decoder == "wordbeamsearch" and self._dictionary is not None):
            raise NotImplementedError("decoder='wordbeamsearch' needs easyocr's dictionary files, which are not available offline; "
                                      "'greedy' (the reference's call) and 'beamsearch' are implemented")
        if output_format not in ("standard", "dict", "json"):
            raise NotImplementedError("output_format 'free_merge' is not implemented "
                                      "(the reference calls readtext(path, paragraph=False, batch_size=1, workers=0))")
