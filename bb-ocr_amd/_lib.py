"""ctypes binding of libbbocr.so (include/bbocr.h) -- the stub a BB-OCR maintainer would add.

There is no fallback: if the shared library (hand-written HIP kernels for gfx950) is not
built, importing this module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C bb-ocr_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BBOCR_LIB_PATH") or os.path.join(_HERE, "libbbocr.so")   # override: A/B runs of two builds on one box


class bbocr_config(C.Structure):
    _fields_ = [("device", C.c_int), ("det_sub_batch", C.c_int), ("rec_max_cols", C.c_int), ("precision", C.c_int), ("call_slots", C.c_int),
                ("host_threads", C.c_int), ("rec_quant", C.c_int), ("rec_classes", C.c_int)]


class bbocr_config_v2(C.Structure):
    """bbocr.h bbocr_config_v2: bbocr_config (whose 32 bytes stand) with the later fields appended; what bbocr_create_v2 takes"""
    _fields_ = bbocr_config._fields_ + [("beam_wide", C.c_int)]


PRECISIONS = {"bf16": 0, "fp16": 1, "exact": 2, "mixed": 3, "exact_rec": 4}
REC_CLASSES_MAX = 8192                                                           # bbocr.h BBOCR_REC_CLASSES_MAX
BEAM_DEVICE_MAX = 32                                                             # bbocr.h BBOCR_BEAM_DEVICE_MAX
PAGE_GRAY, PAGE_BGR, PAGE_RGB, PAGE_YCBCR4, PAGE_YCBCR3 = 0, 1, 2, 3, 4          # bbocr.h BBOCR_PAGE_*: layouts of a device page
PNG_CHUNK = 16384                                                                # bbocr.h BBOCR_PNG_CHUNK
PAGE_PX_BYTES = {PAGE_GRAY: 1, PAGE_BGR: 3, PAGE_RGB: 3, PAGE_YCBCR4: 4, PAGE_YCBCR3: 3}    # bytes per pixel (csrc/kernels.h page_px_bytes)


class bbocr_tensor_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4), ("data", C.POINTER(C.c_float))]


class bbocr_params(C.Structure):
    _fields_ = [
        ("text_threshold", C.c_double), ("low_text", C.c_double), ("link_threshold", C.c_double), ("mag_ratio", C.c_double),
        ("slope_ths", C.c_double), ("ycenter_ths", C.c_double), ("height_ths", C.c_double), ("width_ths", C.c_double),
        ("add_margin", C.c_double), ("contrast_ths", C.c_double), ("adjust_contrast", C.c_double),
        ("canvas_size", C.c_int), ("min_size", C.c_int), ("ignore_mask", C.c_uint * 4), ("decoder", C.c_int), ("beam_width", C.c_int), ("rotation_info", C.c_int * 4),
    ]


class bbocr_preproc_params(C.Structure):
    _fields_ = [("scale", C.c_double), ("blur_sigma", C.c_double), ("contrast", C.c_double), ("brightness", C.c_double),
                ("clahe_clip", C.c_double), ("unsharp_radius", C.c_double), ("unsharp_percent", C.c_int), ("unsharp_threshold", C.c_int),
                ("reserved", C.c_int * 4)]


class bbocr_jpeg_plan(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("sampling", (C.c_int * 2) * 3), ("restart_interval", C.c_int),
                ("mcu_cols", C.c_int), ("mcu_rows", C.c_int), ("segments", C.c_int), ("scan_offset", C.c_longlong), ("scan_bytes", C.c_longlong),
                ("supported", C.c_int), ("reason", C.c_int), ("orientation", C.c_int), ("reserved", C.c_int * 2),
                ("chroma", C.c_int)]                             # 1 = 4:4:4, 2 = 4:2:2, 3 = 4:4:0: decodable although `supported` is 0


JPEG_MAX_SCANS = 64                                                              # bbocr.h BBOCR_JPEG_MAX_SCANS
JPEG_NOT_JPEG, JPEG_SOF, JPEG_SCRIPT, JPEG_SCANS = 1, 4, 12, 13                   # bbocr.h BBOCR_JPEG_*: no SOI, "not SOF2", and the reasons the progressive plan adds


class bbocr_jpeg_scan(C.Structure):
    _fields_ = [("components", C.c_int), ("component", C.c_int * 3), ("dc_table", C.c_int * 3), ("ac_table", C.c_int * 3), ("ss", C.c_int),
                ("se", C.c_int), ("ah", C.c_int), ("al", C.c_int), ("restart_interval", C.c_int), ("segments", C.c_int), ("offset", C.c_longlong),
                ("bytes", C.c_longlong)]


class bbocr_jpeg_progressive_plan(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("sampling", (C.c_int * 2) * 3), ("mcu_cols", C.c_int),
                ("mcu_rows", C.c_int), ("chroma", C.c_int), ("orientation", C.c_int), ("supported", C.c_int), ("reason", C.c_int),
                ("n_scans", C.c_int), ("reserved", C.c_int), ("scans", bbocr_jpeg_scan * JPEG_MAX_SCANS)]


JPEG_FORM_YCBCR, JPEG_FORM_IMREAD = 0, 1                                         # bbocr.h BBOCR_JPEG_FORM_*
JPEG_UP_NONE, JPEG_UP_H2V1_FANCY, JPEG_UP_H1V2_FANCY, JPEG_UP_H2V2_NOT_NEEDED, JPEG_UP_REPLICATE = range(5)    # bbocr.h BBOCR_JPEG_UP_*


class bbocr_jpeg_output(C.Structure):
    _fields_ = [("scale", C.c_int), ("form", C.c_int), ("dev_out", C.POINTER(C.c_void_p)), ("pitches", C.POINTER(C.c_longlong))]


class bbocr_jpeg_scaled_comp(C.Structure):
    _fields_ = [("block", C.c_int), ("plane_rows", C.c_int), ("plane_cols", C.c_int), ("valid_rows", C.c_int), ("valid_cols", C.c_int),
                ("upsample", C.c_int)]


class bbocr_png_plan(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("color_type", C.c_int), ("channels", C.c_int), ("bpp", C.c_int),
                ("row_bytes", C.c_longlong), ("palette_entries", C.c_int), ("idat_chunks", C.c_int), ("idat_bytes", C.c_longlong),
                ("supported", C.c_int), ("reason", C.c_int), ("reserved", C.c_int * 2)]


# bbocr.h BBOCR_PNG_*: why bbocr_host_png_plan refuses a file
(PNG_OK, PNG_NOT_PNG, PNG_TRUNCATED, PNG_CRC, PNG_DIMENSIONS, PNG_DEPTH, PNG_INTERLACE, PNG_PALETTE, PNG_IDAT_ORDER, PNG_APNG, PNG_ZLIB,
 PNG_HEADER) = range(12)


class bbocr_tiff_plan(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bits", C.c_int), ("samples", C.c_int), ("photometric", C.c_int),
                ("compression", C.c_int), ("predictor", C.c_int), ("big_endian", C.c_int), ("rows_per_strip", C.c_longlong), ("strips", C.c_int),
                ("extra_sample", C.c_int), ("row_bytes", C.c_longlong), ("strip_bytes", C.c_longlong), ("supported", C.c_int), ("reason", C.c_int),
                ("reserved", C.c_int * 2)]


# bbocr.h BBOCR_TIFF_*: why bbocr_host_tiff_plan refuses a file
(TIFF_OK, TIFF_NOT_TIFF, TIFF_BIGTIFF, TIFF_TRUNCATED, TIFF_HEADER, TIFF_DIMENSIONS, TIFF_TILES, TIFF_PLANAR, TIFF_FILL_ORDER, TIFF_DEPTH,
 TIFF_SUBBYTE, TIFF_GRAY_ALPHA, TIFF_ASSOC_ALPHA, TIFF_PHOTOMETRIC, TIFF_SAMPLES, TIFF_JPEG, TIFF_CCITT, TIFF_COMPRESSION, TIFF_PREDICTOR,
 TIFF_OLD_LZW, TIFF_STRIPS, TIFF_PALETTE) = range(22)


class bbocr_tiff_fax(C.Structure):
    _fields_ = [("scheme", C.c_int), ("t4_options", C.c_int), ("fill_order", C.c_int), ("reason", C.c_int), ("reserved", C.c_int * 4)]


# bbocr.h BBOCR_FAX_*: why bbocr_host_tiff_fax_plan refuses a file, and the widest row the CCITT decoder takes
(FAX_OK, FAX_PLAIN, FAX_FILL_ORDER, FAX_DEPTH, FAX_OPTIONS, FAX_WIDTH) = range(6)
FAX_MAX_WIDTH = 10240


CONV_ROUTE_IDS = ("NONE", "GEN64_P4", "GEN64_P8", "GEN64_P16", "GEN128_P4", "GEN128_P8", "GEN128_P16", "DMA64_FUSE1", "DMA64_POSTW", "RESW_POOL64",
                  "RESW_1CH", "RESW_2CH", "DMA64_324_NF2", "DMA64_324", "DMA64_384", "DMA64_448", "DMA128_384", "DMA128_448", "DMA2X2_64",
                  "DMA2X2_128", "DMA1X1_64", "DMA1X1_128", "DMA1X1_256", "DMA1X1_ADDUP")       # include/bbocr.h BBOCR_ROUTE_*, in order
CONV_ROUTE_FIELDS = ("id", "status", "el", "wm", "wn", "mf", "piter", "npb", "ring", "nps", "fuse1", "nf", "epi", "ks", "addup", "resw", "OH", "OW",
                     "TH", "TW", "PH", "PW", "NP", "sub", "stack", "tiles_x", "tiles_y", "ntiles_n", "nchunks", "ntaps", "lean", "grid", "threads",
                     "persistent", "lds_bytes", "tail", "split_off")


class bbocr_conv_route(C.Structure):
    _fields_ = [(k, C.c_int) for k in CONV_ROUTE_FIELDS]

    def as_dict(self):
        d = {k: getattr(self, k) for k in CONV_ROUTE_FIELDS}
        d["id"] = CONV_ROUTE_IDS[d["id"]]
        return d


PP_ROUTE_IDS = ("GAUSS_X4", "GAUSS_BYTE", "HIST_X4", "HIST_BYTE", "APPLY_CELL_2", "APPLY_CELL_8", "APPLY_CELL_32", "APPLY_VEC", "APPLY_BYTE",
                "BOX0_X4", "BOX_BYTE", "UNSHARP_FUSED", "UNSHARP_PASSES_VEC", "UNSHARP_PASSES_BYTE", "RESIZE_TILED32", "RESIZE_TILED16",
                "RESIZE_PIXEL")                                                  # include/bbocr.h BBOCR_PP_*, in order
# which of them each bbocr_host_pp_<key>_route may return
PP_ROUTES_OF = {"gauss": ("GAUSS_X4", "GAUSS_BYTE"), "clahe_hist": ("HIST_X4", "HIST_BYTE"),
                "clahe_apply": ("APPLY_CELL_2", "APPLY_CELL_8", "APPLY_CELL_32", "APPLY_VEC", "APPLY_BYTE"), "box": ("BOX0_X4", "BOX_BYTE"),
                "unsharp": ("UNSHARP_FUSED", "UNSHARP_PASSES_VEC", "UNSHARP_PASSES_BYTE"),
                "resize": ("RESIZE_TILED32", "RESIZE_TILED16", "RESIZE_PIXEL")}


class bbocr_page(C.Structure):
    _fields_ = [("dev_rgb", C.c_void_p), ("dev_gray", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("rgb_pitch", C.c_longlong),
                ("gray_pitch", C.c_longlong)]


class bbocr_boxlist(C.Structure):
    _fields_ = [
        ("n_images", C.c_int), ("poly_off", C.POINTER(C.c_int)), ("polys", C.POINTER(C.c_int)),
        ("hori_off", C.POINTER(C.c_int)), ("hori", C.POINTER(C.c_int)),
        ("free_off", C.POINTER(C.c_int)), ("free_q", C.POINTER(C.c_double)),
    ]


class bbocr_result(C.Structure):
    _fields_ = [
        ("n_images", C.c_int), ("box_off", C.POINTER(C.c_int)), ("quads", C.POINTER(C.c_double)),
        ("is_free", C.POINTER(C.c_int)), ("text_off", C.POINTER(C.c_int)), ("text_idx", C.POINTER(C.c_int)),
        ("conf", C.POINTER(C.c_double)),
    ]


# every symbol include/bbocr.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
PROTOTYPES = {
    "bbocr_create": (C.c_int, [C.POINTER(bbocr_config), C.POINTER(_vp)]),
    "bbocr_create_v2": (C.c_int, [C.POINTER(bbocr_config_v2), C.POINTER(_vp)]),
    "bbocr_destroy": (None, [_vp]),
    "bbocr_last_error": (C.c_char_p, [_vp]),
    "bbocr_default_params": (None, [C.POINTER(bbocr_params)]),
    "bbocr_load_weights": (C.c_int, [_vp, C.c_int, C.POINTER(bbocr_tensor_desc), C.c_int]),
    "bbocr_alloc_weights": (C.c_int, [_vp, C.c_int]),
    "bbocr_weights_blob_size": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "bbocr_weights_export": (C.c_int, [_vp, _vp, C.c_size_t]),
    "bbocr_weights_import": (C.c_int, [_vp, _vp, C.c_size_t]),
    "bbocr_dist_unique_id": (C.c_int, [_vp]),
    "bbocr_dist_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "bbocr_dist_finalize": (C.c_int, [_vp]),
    "bbocr_bcast_weights": (C.c_int, [_vp, C.c_int]),
    "bbocr_scatter_images": (C.c_int, [_vp, _vp, C.c_longlong, C.c_size_t, C.c_int, _vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "bbocr_gather_results": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "bbocr_result_pack": (C.c_int, [C.POINTER(bbocr_result), C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "bbocr_result_unpack": (C.c_int, [_vp, C.c_size_t, C.POINTER(C.POINTER(bbocr_result))]),
    "bbocr_free_bytes": (None, [_vp]),
    "bbocr_detect_dims": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "bbocr_detect": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(bbocr_params), _vp]),
    "bbocr_boxes": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(bbocr_params), C.POINTER(C.POINTER(bbocr_boxlist))]),
    "bbocr_recognize": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(bbocr_boxlist), C.POINTER(bbocr_params),
                                  C.POINTER(C.POINTER(bbocr_result))]),
    "bbocr_readtext_batch": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(bbocr_params), C.POINTER(C.POINTER(bbocr_result))]),
    "bbocr_readtext_pages": (C.c_int, [_vp, C.POINTER(bbocr_page), C.c_int, C.POINTER(bbocr_params), C.POINTER(C.POINTER(bbocr_result))]),
    "bbocr_host_pages_plan": (C.c_int, [C.POINTER(bbocr_page), C.c_int, C.POINTER(bbocr_params), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "bbocr_op_pack_pages": (C.c_int, [_vp, C.POINTER(bbocr_page), C.c_int, _vp, _vp]),
    "bbocr_op_crops_pages": (C.c_int, [_vp, C.POINTER(bbocr_page), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int), C.c_int, C.c_float, _vp, C.POINTER(C.c_int), C.c_int]),
    "bbocr_free_boxlist": (None, [C.POINTER(bbocr_boxlist)]),
    "bbocr_free_result": (None, [C.POINTER(bbocr_result)]),
    "bbocr_stage_times": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int]),
    "bbocr_last_ctc_route": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "bbocr_last_ctc_host_sequences": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "bbocr_set_class_mask": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_int]),
    "bbocr_set_profiling": (C.c_int, [_vp, C.c_int]),
    "bbocr_conv_profile": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "bbocr_host_cpu_share": (C.c_int, []),
    "bbocr_host_component_polys": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]),
    "bbocr_host_group_boxes": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(bbocr_params), C.POINTER(C.POINTER(bbocr_boxlist))]),
    "bbocr_host_ctc_beam": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_host_crop_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "bbocr_op_conv2d": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    "bbocr_host_conv_route": (C.c_int, [C.c_int] * 16 + [C.POINTER(bbocr_conv_route)]),
    "bbocr_op_conv2d_route": (C.c_int, [_vp, C.POINTER(bbocr_conv_route)]),
    "bbocr_crnn_logits": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    "bbocr_op_qlinear": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, _vp, _vp, C.POINTER(C.c_float)]),
    "bbocr_op_qlstm": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "bbocr_op_ctc": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                               C.POINTER(C.c_uint), C.c_int]),
    "bbocr_op_ctc_probs": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_uint), _vp]),
    "bbocr_op_ctc_rows": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "bbocr_op_pred": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "bbocr_op_pred_ctc": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_int, _vp, _vp]),
    "bbocr_op_ctc_beam": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int)]),
    "bbocr_op_ctc_beam_wide": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_host_ctc_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "bbocr_host_ctc_wordbeam": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16),
                                          C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_host_wordbeam_route": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "bbocr_set_dictionary": (C.c_int, [_vp, C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.c_int, C.c_int]),
    "bbocr_dictionary_stats": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_op_word_segments": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_op_dict_lookup": (C.c_int, [_vp, C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_int),
                                       C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_op_ctc_wordbeam": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "bbocr_op_resize_u8": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int]),
    "bbocr_op_ycc_to_rgb": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, _vp]),
    "bbocr_upload_pages": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, _vp]),
    "bbocr_op_crops": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_float,
                                 _vp, C.POINTER(C.c_int), C.c_int]),
    "bbocr_preprocess_book_cover": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_preproc_defaults": (None, [C.POINTER(bbocr_preproc_params), C.c_int]),
    "bbocr_preprocess_chain": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(bbocr_preproc_params), _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_op_preprocess_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_double]),
    "bbocr_host_pp_resize_route": (C.c_int, [C.c_int] * 4),
    "bbocr_host_pp_resize_dword_rows": (C.c_int, [C.c_int] * 2),
    "bbocr_host_pp_gauss_route": (C.c_int, [C.c_int] * 4),
    "bbocr_host_pp_clahe_hist_route": (C.c_int, [C.c_int] * 3),
    "bbocr_host_pp_clahe_apply_route": (C.c_int, [C.c_int] * 4),
    "bbocr_host_pp_box_route": (C.c_int, [C.c_int] * 5),
    "bbocr_host_pp_unsharp_route": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]),
    "bbocr_host_pp_unsharp_box_radius": (C.c_int, [C.c_double]),
    "bbocr_auto_crop": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "bbocr_op_autocrop_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, _vp]),
    "bbocr_op_autocrop_mask_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_longlong, _vp, C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(C.c_int)]),
    "bbocr_ocr_thumbnail": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "bbocr_op_thumbnail_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_thumbnail_dims": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_host_thumbnail_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "bbocr_host_resample_coeffs": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                             C.POINTER(C.c_int)]),
    "bbocr_host_jpeg_qtables": (C.c_int, [C.c_int, C.POINTER(C.c_uint16)]),
    "bbocr_host_jpeg_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_jpeg_plan)]),
    "bbocr_jpeg_decode": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bbocr_jpeg_imread": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                    C.POINTER(C.c_int)]),
    "bbocr_page_orient": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, _vp, C.c_longlong, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int)]),
    "bbocr_op_jpeg_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_jpeg_decode_scaled": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bbocr_jpeg_scaled_dims": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bbocr_op_jpeg_scaled_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_jpeg_decode_scales": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(bbocr_jpeg_output), C.c_int,
                                           C.POINTER(C.c_int)]),
    "bbocr_jpeg_counters": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bbocr_host_jpeg_progressive_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_jpeg_progressive_plan)]),
    "bbocr_jpeg_decode_progressive": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(bbocr_jpeg_output),
                                                C.c_int, C.POINTER(C.c_int)]),
    "bbocr_op_jpeg_progressive_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_int, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_host_jpeg_scaled_geometry": (C.c_int, [C.POINTER(bbocr_jpeg_plan), C.c_int, C.POINTER(bbocr_jpeg_scaled_comp)]),
    "bbocr_op_jpeg_scaled_class_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_thumbnail_box": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "bbocr_host_resize_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "bbocr_jpeg_encode_bound": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bbocr_host_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bbocr_jpeg_encode": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "bbocr_op_jpeg_encode_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "bbocr_png_encode_bound": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "bbocr_png_encode": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bbocr_op_deflate": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bbocr_op_png_stage": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_size_t, _vp, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "bbocr_host_png_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_png_plan)]),
    "bbocr_png_decode": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bbocr_op_png_decode_stage": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_host_tiff_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_tiff_plan)]),
    "bbocr_tiff_decode": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bbocr_op_tiff_decode_stage": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_host_tiff_fax_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_tiff_plan), C.POINTER(bbocr_tiff_fax)]),
    "bbocr_tiff_decode_fax": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "bbocr_op_tiff_fax_decode_stage": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
}

class bbocr_gif_plan(C.Structure):
    _fields_ = [("screen_w", C.c_int), ("screen_h", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("canvas_w", C.c_int), ("canvas_h", C.c_int), ("interlace", C.c_int), ("table_len", C.c_int), ("local_table", C.c_int),
                ("transparency", C.c_int), ("min_code", C.c_int), ("mode_l", C.c_int), ("payload_bytes", C.c_longlong), ("supported", C.c_int),
                ("reason", C.c_int), ("reserved", C.c_int * 2), ("table", C.c_uint8 * 768)]


# bbocr.h BBOCR_GIF_*: why bbocr_host_gif_plan refuses a file
(GIF_OK, GIF_NOT_GIF, GIF_TRUNCATED, GIF_NO_IMAGE, GIF_EMPTY, GIF_PIXELS, GIF_CODE_SIZE) = range(7)

class bbocr_bmp_plan(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bits", C.c_int), ("compression", C.c_int), ("header_size", C.c_int),
                ("top_down", C.c_int), ("colors", C.c_int), ("mode", C.c_int), ("r_at", C.c_int), ("g_at", C.c_int), ("b_at", C.c_int),
                ("six_bit_green", C.c_int), ("table_offset", C.c_longlong), ("table_entry", C.c_int), ("supported", C.c_int),
                ("row_stride", C.c_longlong), ("data_offset", C.c_longlong), ("reason", C.c_int), ("reserved", C.c_int * 3)]


# bbocr.h BBOCR_BMP_*: why bbocr_host_bmp_plan refuses a file
(BMP_OK, BMP_NOT_BMP, BMP_TRUNCATED, BMP_HEADER, BMP_DIMENSIONS, BMP_PIXELS, BMP_DEPTH, BMP_RLE, BMP_COMPRESSION, BMP_MASKS, BMP_PALETTE,
 BMP_GRAY_TABLE) = range(12)

_FILE_DECODE = (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                          C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.POINTER(C.c_int)])
PROTOTYPES.update({
    "bbocr_host_gif_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_gif_plan)]),
    "bbocr_gif_decode": _FILE_DECODE,
    "bbocr_gif_decode_timed": (_FILE_DECODE[0], _FILE_DECODE[1] + [C.POINTER(C.c_float)]),
    "bbocr_op_gif_decode_stage": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int)]),
    "bbocr_gif_piece_room": (C.c_size_t, [C.c_longlong, C.c_int]),
    "bbocr_host_bmp_plan": (C.c_int, [_vp, C.c_size_t, C.POINTER(bbocr_bmp_plan)]),
    "bbocr_bmp_decode": _FILE_DECODE,
})

_lib = None


def load():
    """Load libbbocr.so and attach prototypes.  Raises RuntimeError if it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X backend has no CPU fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
    # torch wheels bundle their own libamdhip64; libbbocr.so needs the same SONAME.  Whichever is loaded first serves both, and a
    # process with TWO HIP runtimes cannot create streams (bbocr_create fails): load torch's first so that there is only one.
    try:
        import torch  # noqa: F401
    except Exception:       # a torch-free host still gets the ABI (system ROCm runtime)
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libbbocr.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
