/* libbbocr -- C ABI of the MI355X-native OCR backend (detector + recogniser) for BB-OCR.
 *
 * Drop-in boundary: the L3 -> L1 edge of the reference, i.e. what
 *     easyocr.Reader(["en"], gpu=...)                     pipeline_demo/extractor/enhanced_extractor.py:153
 *     reader.readtext(path, paragraph=False, batch_size=1, workers=0)      ...enhanced_extractor.py:520
 * compute.  The reference has no FFI of its own (it is pure Python on the third-party easyocr==1.7.2,
 * pipeline_demo/requirements.txt:7); the Python binding a maintainer adds is the ctypes stub shown in
 * INTEGRATION.md and shipped as bb_ocr_amd/_lib.py.
 *
 * Conventions: every entry point returns 0 on success and a negative bbocr_status on failure, never throws and
 * never aborts (the reference relies on catching exceptions: enhanced_extractor.py:529-531, i2j_ui/app/main.py:631-644);
 * bbocr_last_error() gives the message.  Image / heat-map pointers are DEVICE pointers (HBM); weight descriptors and
 * results are HOST memory.  All work of one call is ordered on the context's own HIP stream and the call returns after
 * its own work has finished.  One context may be used from several threads: up to bbocr_config::call_slots (default 2) pipeline
 * calls run at once, each in its own call slot (work buffers, side stream), sharing the weights and the compute stream; further
 * callers wait for a free slot; weight loading / export / import wait for every slot.  bbocr_stage_times and bbocr_last_error
 * answer for the calling thread.  ctypes releases the GIL around each call.
 */
#ifndef BBOCR_H
#define BBOCR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbocr_ctx bbocr_ctx;

enum bbocr_status {
    BBOCR_OK = 0,
    BBOCR_ERR_ARG = -1,      /* bad argument / shape */
    BBOCR_ERR_HIP = -2,      /* a HIP runtime call failed */
    BBOCR_ERR_WEIGHTS = -3,  /* missing or mis-shaped tensor in a state-dict */
    BBOCR_ERR_STATE = -4,    /* weights not loaded, context destroyed, ... */
    BBOCR_ERR_OVERFLOW = -5, /* a device work buffer was too small (reported, never silent) */
    BBOCR_ERR_INTERNAL = -6,
    BBOCR_ERR_DATA = -7      /* per-file status of bbocr_jpeg_decode: the entropy-coded data is not what the headers promise */
};

/* Streams: every context owns non-blocking HIP streams.  On entry each call waits for the legacy default stream (where torch
 * queues its copies and fills by default); device buffers produced on OTHER streams must be complete before they are passed in.
 * Every call returns with its own work finished (results are host-visible / device buffers final). */
typedef struct bbocr_config {
    int device;         /* HIP device ordinal */
    int det_sub_batch;  /* pages per detector pass; 0 = auto (<= 64 pages / 96 GB of activations, short last pass) */
    int rec_max_cols;   /* pixel columns (4 per pooled time step) whose sequence stage runs as one pass; 0 = default (6,000,000) */
    int precision;      /* arithmetic of the two networks (fixed per context: the weights are packed for it at bbocr_load_weights):
                         *   BBOCR_PREC_BF16  (0) bf16 MFMA operands and stored activations, fp32 accumulation;
                         *   BBOCR_PREC_FP16  (1) the same kernels on IEEE fp16 operands (v_mfma_f32_16x16x32_f16): 8x finer rounding,
                         *                        range 6e-8 .. 65504 -- BASELINE.json configs[4] ("fp16 MFMA conv path"), and what the Python host
                         *                        (bb_ocr_amd.Reader) selects unless told otherwise: boxes and strings equal to the fp32 CPU path's
                         *                        on every input class measured;
                         *   BBOCR_PREC_EXACT (2) BOTH networks in split fp16: every activation and weight is a pair hi + lo of fp16 values
                         *                        (22 significand bits) and every product runs as the three MFMA terms hi*hi + lo*hi + hi*lo
                         *                        accumulated in fp32, LSTM state and gates in fp32 -- threshold decisions and boxes follow the
                         *                        fp32 CPU path on arbitrary heat-maps, CONFIDENCES to 1e-5 (3x the MFMA work: ~0.3x FP16's rate);
                         *   BBOCR_PREC_MIXED (3) detector as BF16, recogniser as FP16: 1.6 % faster than FP16 and as exact on binary-ink pages
                         *                        (2,051 of 2,051 boxes and strings of the 1280x960 workload equal the fp32 CPU path's,
                         *                        profiles/r03_text_parity.json): bf16 keeps the detector's clock (fp16 operands
                         *                        toggle more bits under the power limit); on continuous-tone images its bf16
                         *                        heat-map flips a few threshold decisions (3 of 110 boxes on the reference's images).
                         *   BBOCR_PREC_EXACT_REC (4) detector as FP16, recogniser as in EXACT: the fp32 path's confidences (1e-5) -- what upstream's
                         *                        contrast-retry decision and "keep the better pass" read -- at ~0.65x FP16's rate; boxes as FP16's.
                         * Any other value: bbocr_create returns BBOCR_ERR_ARG. */
    int call_slots;     /* calls that may be IN FLIGHT on this context at once: 0 = default (2), 1 = calls serialise (rounds 1-3), 2.
                         * The reference shares one Reader between ThreadPoolExecutor workers (batch_processor_enhanced.py:215, default 2).
                         * A call that arrives while another is running takes the second slot: own work buffers (allocated on first use,
                         * i.e. only if two calls ever overlap), same weights, same compute stream -- its detector runs on the card while the
                         * first call's host thread finishes box geometry, CTC read-back and result export.  Results are those of the
                         * serial path bit for bit (tests/test_gpu_pipeline.py::test_two_calls_in_flight_equal_the_serial_path). */
    int host_threads;   /* host worker threads per call slot (box geometry of a detector pass, beam search): 0 = auto = min(16, the CPUs this
                         * PROCESS may use: scheduler affinity mask and cgroup CPU quota -- not the machine's core count, which every one of
                         * the 8 ranks of a node would claim for itself).  Ranks that are not pinned pass their share (the Python host:
                         * share / LOCAL_WORLD_SIZE).  The pool is created once per slot and kept; no thread is spawned per call. */
    int rec_quant;      /* 0 (default): the recogniser as `precision` says.  1: its SEQUENCE half -- both BiLSTMs, the two Linear layers behind them
                         * and Prediction -- in the arithmetic easyocr's quantize=True default runs on a CPU device: torch's x86 / fbgemm DYNAMIC
                         * int8 quantisation (symmetric qint8 weights per tensor, 7-bit activation codes whose scale and zero point are taken per
                         * crop and, for the recurrent product, per direction and time step; int32 accumulation on v_mfma_i32_16x16x64_i8), every
                         * crop on its own as readtext(batch_size=1) runs it.  The conv stack, the 3-row mean and CTC are unchanged.  Allowed with
                         * BBOCR_PREC_EXACT and BBOCR_PREC_EXACT_REC only (what is quantised are the fp32 path's features, which those modes deliver
                         * to 1e-5); any other precision or value: bbocr_create returns BBOCR_ERR_ARG, and so it does with rec_classes
                         * other than 97 (0): the int8 Prediction is built for english_g2's 97 classes alone.  The weight blob carries the flag: a blob of
                         * the other kind is refused (BBOCR_ERR_WEIGHTS).  DESIGN.md section 4 states the arithmetic. */
    int rec_classes;    /* classes of the recogniser's Prediction layer, the CTC blank (class 0) included: 0 (default) = 97, english_g2.  Every
                         * generation-2 model of easyocr shares the CRNN and differs in this number alone (latin_g2 352, zh_sim_g2 6,719).  Valid:
                         * 2 .. BBOCR_REC_CLASSES_MAX; bbocr_load_weights then wants Prediction.weight [rec_classes, 256] and Prediction.bias
                         * [rec_classes] (BBOCR_ERR_WEIGHTS otherwise), the weight blob carries the count (a blob of another count:
                         * BBOCR_ERR_WEIGHTS) and bbocr_result::text_idx holds 1 .. rec_classes - 1.  Up to 128 classes nothing else changes.
                         * Above 128 the class mask comes from bbocr_set_class_mask, decoder == BEAMSEARCH is searched on the host (on the device
                         * with bbocr_config_v2::beam_wide == 1, below), and greedy
                         * passes of the 16-bit precisions run Prediction + softmax + arg-max as ONE kernel that never stores the logits
                         * (pred_ctc.hip).  rec_quant == 1 with any count but 97, or a count outside the range: bbocr_create
                         * returns BBOCR_ERR_ARG. */
} bbocr_config;
/* bbocr_config with the fields added since its layout was fixed, appended behind it: what bbocr_create_v2 takes.  bbocr_config itself keeps
 * its 32 bytes, so a caller built against an earlier header (or the earlier ctypes structure) that hands bbocr_create a 32-byte block is
 * still read correctly; bbocr_create means every field below at its default. */
typedef struct bbocr_config_v2 {
    bbocr_config base;  /* the fields above, unchanged */
    int beam_wide;      /* 0 (default): decoder == BEAMSEARCH over more than 128 classes is searched on the host, which reads the probabilities
                         * back.  1: widths up to BBOCR_BEAM_DEVICE_MAX are searched on the device (ctc_beam_wide.hip: a candidate list per row,
                         * then one wave per sequence; only text and lengths are read back, the text is the host search's exactly).  A sequence
                         * with a row of more than 128 candidate classes (p >= 0.5 / rec_classes) alone is searched on the host, from its own
                         * rows.  On a context of at most 128 classes the field changes nothing.  Any other value: bbocr_create_v2
                         * returns BBOCR_ERR_ARG. */
} bbocr_config_v2;
#define BBOCR_REC_CLASSES_MAX 8192
enum { BBOCR_PREC_BF16 = 0, BBOCR_PREC_FP16 = 1, BBOCR_PREC_EXACT = 2, BBOCR_PREC_MIXED = 3, BBOCR_PREC_EXACT_REC = 4 };

/* One tensor of an upstream state-dict (easyocr/craft.py::CRAFT or easyocr/model/vgg_model.py::Model key names,
 * optional "module." prefix), fp32, host memory, C-contiguous.  Replaces torch.load + load_state_dict in
 * easyocr/detection.py::get_detector and easyocr/recognition.py::get_recognizer. */
typedef struct bbocr_tensor_desc {
    const char* name;
    int ndim;
    int64_t shape[4];
    const float* data;
} bbocr_tensor_desc;

/* keyword arguments of easyocr.Reader.readtext that affect this path (same names, same defaults) */
enum { BBOCR_DECODER_GREEDY = 0, BBOCR_DECODER_BEAMSEARCH = 1, BBOCR_DECODER_WORDBEAMSEARCH = 2 };
/* Widest beam the device search takes.  The kernel keeps one sequence's whole search in the LDS of one workgroup (64 KB): the step's entry
 * table, beam_width * (1 + C) floats, plus the live labellings as bytes, 2 * beam_width * T (double-buffered), plus under 3 KB of row and
 * beam state.  At width 32 and C = 128 that is 32 * 129 * 4 = 16,512 B of entries and 64 B per time step: T up to 708, above the 639 steps
 * of a crop as wide as the default canvas (2560 / 4 - 1).  Width 64 would halve that to T <= 250.
 * The search over more than 128 classes (bbocr_config_v2::beam_wide) keeps the same table over at most 128 candidates per step and the
 * labellings as 16-bit symbols, 4 * beam_width * T bytes: at width 32 that is 19,856 B of tables and state and 128 B per time step, T up
 * to 356; at width 5, T up to 3,076.  A longer sequence sends its pass to the host search. */
#define BBOCR_BEAM_DEVICE_MAX 32
/* decoder == BBOCR_DECODER_WORDBEAMSEARCH (easyocr's decode_wordbeamsearch for a model without separator characters, over the words of
 * bbocr_set_dictionary; BBOCR_ERR_ARG on a context without a dictionary): the final candidates of a word group that are tested against the
 * dictionary -- upstream's wordsearch(classes, ignore_idx, 20, dict_list).  beam_width is used as for BEAMSEARCH.  csrc/ctc_wordbeam.cpp
 * states the decoder; widths up to BBOCR_BEAM_DEVICE_MAX at up to 128 classes run on the device, everything else on the host, with the
 * same text. */
#define BBOCR_WORD_CANDIDATES 20

typedef struct bbocr_params {
    double text_threshold; /* 0.7 */
    double low_text;       /* 0.4 */
    double link_threshold; /* 0.4 */
    double mag_ratio;      /* 1.0 */
    double slope_ths;      /* 0.1 */
    double ycenter_ths;    /* 0.5 */
    double height_ths;     /* 0.5 */
    double width_ths;      /* 0.5 */
    double add_margin;     /* 0.1 */
    double contrast_ths;   /* 0.1 */
    double adjust_contrast;/* 0.5 */
    int canvas_size;       /* 2560 */
    int min_size;          /* 20 */
    unsigned int ignore_mask[4]; /* recognizer_predict's ignore_idx as a bit mask over class indices 0..127 (allowlist / blocklist):
                                  * those classes are zeroed and the rest renormalised before the arg-max; 0 = none (english_g2 default) */
    int decoder;           /* BBOCR_DECODER_GREEDY (0, readtext's default, the reference's call) or BBOCR_DECODER_BEAMSEARCH (1):
                            * easyocr/utils.py::ctcBeamSearch without a language model over the device's probabilities.  Widths up to
                            * BBOCR_BEAM_DEVICE_MAX are searched on the device (one wave per sequence; only the text is read back);
                            * wider beams, and sequences too long for the kernel's LDS block, are searched on the host, which reads the
                            * probabilities back.  Both give the same text.  The confidence is the greedy path's custom_mean for every
                            * decoder, as upstream computes it */
    int beam_width;        /* 5 (readtext's beamWidth); used when decoder == BBOCR_DECODER_BEAMSEARCH */
    int rotation_info[4];  /* readtext's rotation_info: up to three angles out of {90, 180, 270}, zero-terminated (all 0 = None, the
                            * reference's call).  Non-empty: Reader.recognize's batched branch -- every crop of a page padded to the page's
                            * max_width, each also recognised as np.rot90(crop, angle/90), the most confident variant reported, results
                            * sorted by the boxes' top y */
} bbocr_params;

/* output of detection (easyocr.Reader.detect): per image horizontal_list / free_list, plus the ungrouped polygons */
typedef struct bbocr_boxlist {
    int n_images;
    int* poly_off;   /* [n_images+1] */
    int* polys;      /* [poly_off[n]][8]  int32 x,y x4 (detection.get_textbox output, image coordinates) */
    int* hori_off;   /* [n_images+1] */
    int* hori;       /* [hori_off[n]][4]  xmin, xmax, ymin, ymax */
    int* free_off;   /* [n_images+1] */
    double* free_q;  /* [free_off[n]][8]  x,y x4 */
} bbocr_boxlist;

/* output of readtext: boxes in upstream order (horizontal boxes, then free boxes), per image */
typedef struct bbocr_result {
    int n_images;
    int* box_off;     /* [n_images+1] */
    double* quads;    /* [n_boxes][8]; horizontal boxes are the clamped integer corners */
    int* is_free;     /* [n_boxes] */
    int* text_off;    /* [n_boxes+1] into text_idx */
    int* text_idx;    /* class indices 1..96: position in the english_g2 character list (0 = CTC blank, never emitted) */
    double* conf;     /* [n_boxes] custom_mean confidence */
} bbocr_result;

int bbocr_create(const bbocr_config* cfg, bbocr_ctx** out);
/* bbocr_create with bbocr_config_v2's appended field, beam_wide; bbocr_create of cfg is bbocr_create_v2 of {*cfg, 0} */
int bbocr_create_v2(const bbocr_config_v2* cfg, bbocr_ctx** out);
void bbocr_destroy(bbocr_ctx* ctx);
const char* bbocr_last_error(bbocr_ctx* ctx);
void bbocr_default_params(bbocr_params* p);

/* which: 0 = CRAFT detector (craft_mlt_25k layout), 1 = CRNN recogniser (english_g2 layout).  BatchNorm is folded,
 * weights are packed to the MFMA fragment layout in bf16 and uploaded. */
int bbocr_load_weights(bbocr_ctx* ctx, int which, const bbocr_tensor_desc* descs, int n);

/* ---- multi-GPU: the packed weights as one device blob ("RCCL broadcast of detector/recognizer weights") ----
 * What easyocr does per forward under nn.DataParallel (broadcast_coalesced of every parameter, easyocr.py::get_detector /
 * get_recognizer) happens ONCE here, on the tensors as the kernels read them: rank 0 loads the state-dicts
 * (bbocr_load_weights), exports the BN-folded, element-type-rounded, MFMA-packed images as ONE contiguous DEVICE buffer
 * (bbocr_weights_export; ~49 MB in bf16) and broadcasts it device-to-device (ncclBroadcast over xGMI; torch.distributed.broadcast
 * in the Python host); every other rank lays its plans out with bbocr_alloc_weights (no values) and fills them with
 * bbocr_weights_import.  Size and layout depend only on bbocr_config::precision and on which networks are present; a blob from a
 * context with another precision is refused (BBOCR_ERR_WEIGHTS). */
int bbocr_alloc_weights(bbocr_ctx* ctx, int which /* 0 = detector, 1 = recogniser */);
int bbocr_weights_blob_size(bbocr_ctx* ctx, size_t* bytes);
int bbocr_weights_export(bbocr_ctx* ctx, void* dev_blob, size_t bytes);
int bbocr_weights_import(bbocr_ctx* ctx, const void* dev_blob, size_t bytes);

/* ---- multi-GPU for hosts without torch.distributed: one process per GPU, RCCL over xGMI ----
 * The Python host reaches RCCL through torch.distributed (bb-ocr_amd/dist.py); these entry points do the same exchanges from C.  RCCL is
 * loaded with dlopen("librccl.so.1") at the first call, so single-GPU users need no RCCL.  Rank 0 makes the 128-byte id
 * (bbocr_dist_unique_id = ncclGetUniqueId) and hands it to the other ranks out of band (environment, file, socket); every rank then
 * calls bbocr_dist_init (ncclCommInitRank: collective).  All of them are collective over the ranks of the communicator and wait for every
 * call slot of the context.  There is no collective inside the OCR path itself: pages are independent.
 *   bbocr_bcast_weights   ONE ncclBroadcast of the packed weight blob (root: bbocr_load_weights; others: bbocr_alloc_weights, same
 *                         precision) -- replaces nn.DataParallel's per-forward broadcast_coalesced (easyocr.py::get_detector / get_recognizer);
 *   bbocr_scatter_images  the loader rank's units (pages of unit_bytes = H*W*3) -> each rank's contiguous block [first, first + count)
 *                         (block partition, uneven / empty blocks allowed) as one grouped batch of ncclSend: the root's links carry all
 *                         blocks at once; dev_local holds ceil(n_units / world) units;
 *   bbocr_gather_results  per-rank host bytes (bbocr_result_pack of the rank's results) -> on root one malloc'd concatenation in rank
 *                         order (*all, free with bbocr_free_bytes) + sizes[world]; bbocr_result_unpack rebuilds each bbocr_result. */
int bbocr_dist_unique_id(void* id128);
int bbocr_dist_init(bbocr_ctx* ctx, int rank, int world, const void* id128);
int bbocr_dist_finalize(bbocr_ctx* ctx);
int bbocr_bcast_weights(bbocr_ctx* ctx, int root);
int bbocr_scatter_images(bbocr_ctx* ctx, const uint8_t* dev_all, long long n_units, size_t unit_bytes, int root, uint8_t* dev_local, long long* first,
                         long long* count);
int bbocr_gather_results(bbocr_ctx* ctx, const void* local, size_t local_bytes, int root, void** all, size_t* sizes);
int bbocr_result_pack(const bbocr_result* r, void** bytes, size_t* n);       /* free *bytes with bbocr_free_bytes */
int bbocr_result_unpack(const void* bytes, size_t n, bbocr_result** out);    /* free *out with bbocr_free_result */
void bbocr_free_bytes(void* p);

/* geometry of the detector for an H x W page: network input H32 x W32 (after canvas_size scaling, padded to x32),
 * heat-map h x w = H32/2 x W32/2, ratio as returned by resize_aspect_ratio */
int bbocr_detect_dims(int H, int W, int canvas_size, double mag_ratio, int* H32, int* W32, int* rh, int* rw, double* ratio);

/* S2+S3: uint8 RGB pages [B,H,W,3] (device) -> region/affinity heat-map fp32 [B,h,w,2] (device).
 * Replaces detection.test_net's resize_aspect_ratio + normalizeMeanVariance + CRAFT.forward. */
int bbocr_detect(bbocr_ctx* ctx, const uint8_t* dev_rgb, int B, int H, int W, const bbocr_params* p, float* dev_heat_out);

/* S4+S5: heat-map -> boxes.  Replaces craft_utils.getDetBoxes + adjustResultCoordinates + get_textbox +
 * utils.group_text_box + the min_size filter of Reader.detect.  ratio is the one bbocr_detect_dims returned. */
int bbocr_boxes(bbocr_ctx* ctx, const float* dev_heat, int B, int h, int w, double ratio, const bbocr_params* p, bbocr_boxlist** out);

/* S6-S10: gray pages [B,H,W] uint8 (device) + boxes -> text.  Replaces Reader.recognize (per-box branch:
 * get_image_list, AlignCollate, CRNN forward, softmax, greedy CTC, contrast retry). */
int bbocr_recognize(bbocr_ctx* ctx, const uint8_t* dev_gray, int B, int H, int W, const bbocr_boxlist* boxes, const bbocr_params* p,
                    bbocr_result** out);

/* all stages in one call (== Reader.readtext_batched for equally sized pages).  dev_gray may be NULL: it is then
 * derived from dev_rgb with cv2's BGR2GRAY fixed-point formula, as upstream does for ndarray input. */
int bbocr_readtext_batch(bbocr_ctx* ctx, const uint8_t* dev_rgb, const uint8_t* dev_gray, int B, int H, int W, const bbocr_params* p,
                         bbocr_result** out);

/* ---- pages of mixed shapes in one call ----
 * One page of bbocr_readtext_pages: uint8 RGB in device memory, rows rgb_pitch bytes apart, and optionally its gray plane.  A strided
 * view -- a crop of a larger device page -- is a pointer + pitch and is read in place; no byte outside the H rows of W pixels is read
 * (the padding of a view may belong to another tensor).  Pages may start at any byte and have any pitch >= the row. */
typedef struct bbocr_page {
    const uint8_t* dev_rgb;   /* [H][W][3] uint8, device */
    const uint8_t* dev_gray;  /* [H][W] uint8, device, or NULL: derived from dev_rgb as bbocr_readtext_batch derives it */
    int H, W;
    long long rgb_pitch, gray_pitch;   /* bytes per row; 0 = tight (3 * W, W) */
} bbocr_page;
/* all stages in one call for n pages of individually given shapes: the result is what n one-page bbocr_readtext_batch calls return, bit
 * for bit, n_images == n in the caller's order.  One launch (csrc/pages.hip) packs the pages shape group by shape group -- two pages are
 * in one group when their (H, W) are equal -- the detector runs group after group with no host wait in between, box extraction of a
 * pass overlaps the next pass, and ONE recognition pass reads the crops of all pages, whatever page they came from.  Every work buffer
 * is sized before the first pass is queued.  bbocr_stage_times: [0] is the detector's GPU span over all groups.  BBOCR_ERR_ARG before
 * anything is queued: n <= 0 or n > 65535, a null dev_rgb, H or W <= 0 or H * W >= 2^30, a pitch smaller than the row, a page that
 * collapses to zero size under canvas_size / mag_ratio. */
int bbocr_readtext_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, const bbocr_params* p, bbocr_result** out);
/* host only, no GPU: the plan bbocr_readtext_pages makes of a page list (it runs this very function); the pointers of the pages are only
 * compared with NULL.  group_of_page [n]: groups are numbered by first appearance; slot_in_group [n]: position among the group's pages, in
 * the caller's order; rgb_off / gray_off [n]: byte offset of the page's tight copy in the RGB / gray staging buffer -- a group's pages
 * stand back to back in slot order, [nb][H][W][3] and [nb][H][W], groups in number order, every group's block at a multiple of 256;
 * *n_groups; staging_bytes [2]: size of the RGB and of the gray staging buffer.  Any output pointer may be NULL.  p NULL: the defaults. */
int bbocr_host_pages_plan(const bbocr_page* pages, int n, const bbocr_params* p, int* group_of_page, int* slot_in_group, long long* rgb_off,
                          long long* gray_off, int* n_groups, long long* staging_bytes);
/* the pack launch alone (parity tests): the pages into caller-owned staging buffers of bbocr_host_pages_plan's sizes (default
 * parameters), laid out as it says.  The staging buffers may start at any byte: a page is moved with 16-byte accesses where its source
 * pointer, its pitch and the ADDRESS of its staging copy (base + offset) are multiples of 16, byte by byte otherwise */
int bbocr_op_pack_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, uint8_t* dev_rgb_staging, uint8_t* dev_gray_staging);

void bbocr_free_boxlist(bbocr_boxlist* b);
void bbocr_free_result(bbocr_result* r);

/* milliseconds spent in the last readtext/detect/boxes/recognize call OF THE CALLING THREAD on this context, per stage:
 * [0] detector net (S2+S3), [1] CCL kernels (S4 device), [2] box geometry + grouping (S4/S5 host),
 * [3] crops (S6/S7), [4] recogniser net (S8), [5] CTC decode (S9), [6] contrast retry pass, [7] total */
int bbocr_stage_times(bbocr_ctx* ctx, float* ms, int n);

/* recognizer_predict's ignore_idx for a context of MORE than 128 classes (bbocr_config::rec_classes), whose classes bbocr_params::ignore_mask
 * cannot name: bit c of words[c >> 5] removes class c; n_words <= ceil(rec_classes / 32), the words behind them count as 0; n_words = 0
 * clears the mask.  Bits at or behind rec_classes, and bit 0 (the CTC blank), are BBOCR_ERR_ARG.  A thread holds ONE mask, for ONE context:
 * setting a mask on another context drops the one it held (that context's calls from this thread then run without a mask), so a thread
 * that alternates between wide contexts sets the mask before each call, as the Python Reader does.  bbocr_destroy called from the thread
 * drops its mask for that context; a mask another thread still holds for a destroyed context must be cleared by that thread (n_words = 0 on
 * any live context, or a new mask) before it uses a context created later.  The mask is kept FOR THE CALLING THREAD (as
 * bbocr_last_error and bbocr_stage_times are) and read by that thread's later recognise / readtext calls on this context, so two calls in
 * flight never see each other's mask.  On a context of at most 128 classes: BBOCR_ERR_ARG, and bbocr_params::ignore_mask rules as before
 * (on a wider context its four words are not read, the blank's bit excepted, which stays an argument error). */
int bbocr_set_class_mask(bbocr_ctx* ctx, const uint32_t* words, int n_words);
/* where the text of the LAST sequence pass of the calling thread's last recognise / readtext call on this context came from: 0 greedy
 * (Prediction launch + row kernel + collapse), 1 beam search on the host, 2 beam search on the device, 3 greedy with Prediction inside the CTC
 * kernel (more than 128 classes, 16-bit precisions: no logits stored), 4 beam search on the device over more than 128 classes
 * (bbocr_config_v2::beam_wide; sequences whose rows overflow the candidate list are searched on the host within the same pass); -1: no such pass (no call, a call without boxes, or the thread's
 * last call was on another context: like bbocr_stage_times this is the record of the calling thread's LAST call) */
/* 5: word beam search (BBOCR_DECODER_WORDBEAMSEARCH) on the host, 6: word beam search on the device */
int bbocr_last_ctc_route(bbocr_ctx* ctx, int* route);
/* The word list of BBOCR_DECODER_WORDBEAMSEARCH, as class-index strings: word i = symbols[word_off[i] .. word_off[i + 1]) (word_off[0] = 0),
 * space_class the class of ' ' (it separates word groups and joins the words).  Every word is checked first -- symbols in 1 .. C - 1, none
 * the space class, length 1 .. 1024 -- and a bad table is BBOCR_ERR_ARG with nothing changed.  Duplicates are kept once.  The table is built
 * (an open-addressing set, csrc/word_dict.h), uploaded once (contexts of at most 128 classes) and kept on the host for the host route.
 * n_words == 0 clears it.  Waits for the context's call slots, as bbocr_load_weights does. */
int bbocr_set_dictionary(bbocr_ctx* ctx, const uint16_t* symbols, const int* word_off, int n_words, int space_class);
/* the context's dictionary (any pointer may be null): words kept, slots of the table, its longest probe run, and the words with two adjacent
 * equal symbols (the collapse of a labelling removes adjacent repeats: "book" is matched only through a labelling that holds a blank symbol
 * between the two letters).  All 0
 * without a dictionary */
int bbocr_dictionary_stats(bbocr_ctx* ctx, int* words, int* slots, int* longest_probe, int* unmatchable);
/* the sequences of the calling thread's last recognise / readtext call on this context that route 4 left to the host search (a row of more
 * than 128 candidate classes), summed over the call's sequence passes; 0 on every other route.  On trained models it stays 0 or near it: a
 * count that does not says that the candidate list is too short for the model's rows */
int bbocr_last_ctc_host_sequences(bbocr_ctx* ctx, int* n);

/* Per-launch timing of the dominant kernel (conv_mfma) with HIP events recorded on the context's stream.
 * group 0 = detector convs, 1 = recogniser convs/GEMMs.  on = 1 times group 0 only (54 launches per 64-page step: the roofline
 * leg of bench.py), on = 2 both groups (about ten times as many events: ~1.5 % of a step), 0 = off.  Totals accumulate from the call on:
 * ms = sum of launch durations, flops = sum of ALGORITHMIC flops (2*N*OH*OW*Cout*Cin*KH*KW, unpadded). */
int bbocr_set_profiling(bbocr_ctx* ctx, int on);
int bbocr_conv_profile(bbocr_ctx* ctx, int group, double* ms, double* flops, long long* launches);

/* ---- host-only halves of S4/S5 (no device work; callable without a GPU, used by the CPU test-suite) ----
 * comps: [n][7] = root, left, top, right, bottom, area, row_off (heat-map coordinates); rowext: per component row the
 * min/max x of TEXT pixels ([row_off + y - top][2], max < 0 = none) -- exactly what the CCL kernels emit.
 * Writes n polygons [n][8] (craft_utils.getDetBoxes_core tail + adjustResultCoordinates + get_textbox). */
/* CPUs this PROCESS may use (scheduler affinity mask, cgroup v2 cpu.max / v1 cfs quota): what bbocr_config::host_threads = 0 sizes the
 * per-slot host pools from (capped at 16) -- never the machine's core count */
int bbocr_host_cpu_share(void);
int bbocr_host_component_polys(const int* comps, const int* rowext, int n, int w, int h, double ratio, int* polys_out);
/* utils.group_text_box + Reader.detect's min_size filter on n polygons of one image */
int bbocr_host_group_boxes(const int* polys, int n, const bbocr_params* p, bbocr_boxlist** out);
/* easyocr/utils.py::ctcBeamSearch (CTCLabelConverter.decode_beamsearch, no language model) on host probabilities fp32 [n,T,cs]
 * (C <= cs classes, class 0 = blank): text_off [n+1], text_idx (<= n*T).  The definition of bbocr_params::decoder == BEAMSEARCH, the path of
 * beams wider than BBOCR_BEAM_DEVICE_MAX, and the yardstick of bbocr_op_ctc_beam */
int bbocr_host_ctc_beam(const float* probs, int n, int T, int C, int cs, int beam_width, int* text_off, int* text_idx);
/* CTCLabelConverter.decode_wordbeamsearch for a model without separator characters on host probabilities fp32 [n,T,cs], as
 * csrc/ctc_wordbeam.cpp states it, over the words symbols / word_off / n_words (as bbocr_set_dictionary takes them; n_words == 0: no word,
 * every group decodes as BEAMSEARCH decodes its rows): text_off [n+1], text_idx (<= n*T).  Needs no context and no device.  The definition of
 * bbocr_params::decoder == WORDBEAMSEARCH and the yardstick of bbocr_op_ctc_wordbeam */
int bbocr_host_ctc_wordbeam(const float* probs, int n, int T, int C, int cs, int beam_width, int space_class, const uint16_t* symbols,
                            const int* word_off, int n_words, int* text_off, int* text_idx);
/* the rule by which a WORDBEAMSEARCH pass picks its route (values 5 / 6 of bbocr_last_ctc_route): the host for more than 128 classes, a width
 * above BBOCR_BEAM_DEVICE_MAX, or a longest SEQUENCE (which bounds every word group) whose LDS block would not fit */
int bbocr_host_wordbeam_route(int beam_width, int C, const int* seqs, int nseq);
/* the crop plan of explicit boxes of ONE H x W gray page, as bbocr_op_crops and a recognition pass make it (utils.get_image_list's clamp /
 * four_point_transform geometry and resize target, AlignCollate's content width): hori [n_hori][4] = x_min, x_max, y_min, y_max, free_q
 * [n_free][4][2].  Box k (the horizontal boxes, then the free ones): taken[k] = 0 for a box the pass skips (empty after clamping, a quad
 * with a side shorter than a pixel; its other outputs are zero), else 1 with geom[k][9] = source rectangle sx0, sy0, sw, sh (free box: 0, 0
 * and the warp's maxWidth x maxHeight), cv2.resize target rw x rh, content width fw, own padded width imgW, warp (1 = free box) and minv[k][9]
 * = the inverted perspective matrix warpPerspective samples with (free boxes; zero otherwise) */
int bbocr_host_crop_plan(int H, int W, const int* hori, int n_hori, const double* free_q, int n_free, int* taken, int* geom, double* minv);

/* ---- single-operator entry points (used by the parity tests; same kernels the pipeline runs) ---- */
/* conv2d on device tensors: in bf16 NHWC [N,H,W,Cin] (as uint16 bits), weights fp32 OIHW on the host (+bias or NULL),
 * out bf16 (out_f32 = 0) or fp32 NHWC [N,OH,OW,Cout_store]; Cin % 32 == 0; Cout_store = roundup16(Cout).  With
 * bbocr_config::precision FP16 / EXACT "bf16" reads "fp16" throughout (the DETECTOR's element type of the context; MIXED: bf16).
 * pool_mode 1/2 fuses MaxPool2d(2,2) / MaxPool2d((2,1),(2,1)) (optionally after ReLU: pool_relu) into the epilogue and
 * writes bf16 [N,OH/2,OW/2 or OW,Cout_store] to dev_pool_out; dev_out may then be NULL (pooled output only). */
int bbocr_op_conv2d(bbocr_ctx* ctx, const uint16_t* dev_in, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                    int KH, int KW, int pad, int dil, int relu_in, int relu_out, int out_f32, void* dev_out, int pool_mode, int pool_relu,
                    uint16_t* dev_pool_out);
/* Which conv kernel a bbocr_op_conv2d call takes.  The library's launch code picks one of about thirty kernel instantiations from the
 * layer's shape; the terminal it reaches writes this report (one id per terminal, its template numbers, the geometry it settled). */
enum {
    BBOCR_ROUTE_NONE = 0,    /* nothing launched: the shape was refused, `status` has the HIP error code */
    /* conv_mfma_kernel, the register-staged generic kernel: 64 / 128 couts per tile, PITER 4 / 8 / 16 */
    BBOCR_ROUTE_GEN64_P4, BBOCR_ROUTE_GEN64_P8, BBOCR_ROUTE_GEN64_P16, BBOCR_ROUTE_GEN128_P4, BBOCR_ROUTE_GEN128_P8, BBOCR_ROUTE_GEN128_P16,
    /* conv3x3_dma_kernel, 64 couts: conv1_1 fused in / a 1x1 behind the layer (the networks' own launches only) */
    BBOCR_ROUTE_DMA64_FUSE1, BBOCR_ROUTE_DMA64_POSTW,
    /* conv3x3_resw_kernel (resident weights, persistent tile loop): 64 couts pooled / one input chunk / two */
    BBOCR_ROUTE_RESW_POOL64, BBOCR_ROUTE_RESW_1CH, BBOCR_ROUTE_RESW_2CH,
    /* conv3x3_dma_kernel, 64 couts: 324-slot patch with 2 / 4 cout fragments per wave, 384 slots, 448 slots */
    BBOCR_ROUTE_DMA64_324_NF2, BBOCR_ROUTE_DMA64_324, BBOCR_ROUTE_DMA64_384, BBOCR_ROUTE_DMA64_448,
    /* conv3x3_dma_kernel, 128 couts: 384 slots (4-deep weight ring), 448 slots (3-deep) */
    BBOCR_ROUTE_DMA128_384, BBOCR_ROUTE_DMA128_448,
    /* conv3x3_dma_kernel as the 2x2 / padding 0 conv */
    BBOCR_ROUTE_DMA2X2_64, BBOCR_ROUTE_DMA2X2_128,
    /* conv1x1_dma_kernel: 64 / 128 / 256 couts per tile; with an addend in the epilogue, see `addup` (the networks' own launches only) */
    BBOCR_ROUTE_DMA1X1_64, BBOCR_ROUTE_DMA1X1_128, BBOCR_ROUTE_DMA1X1_256, BBOCR_ROUTE_DMA1X1_ADDUP,
    BBOCR_ROUTE_COUNT
};
typedef struct bbocr_conv_route {
    int id;                  /* BBOCR_ROUTE_* */
    int status;              /* HIP error code of the launch (0: launched, or -- dry run -- would have been) */
    int el, wm, wn, mf;      /* template numbers of the kernel; 0 where its family has none: element type (0 bf16, 1 fp16), waves along pixels /
                              * couts, 16-pixel fragments per wave */
    int piter;               /* conv_mfma_kernel: 16-pixel patch pieces a wave stages per chunk */
    int npb, ring, nps, fuse1, nf, epi, ks;   /* conv3x3_dma_kernel: 64-pixel patch blocks, weight ring depth, patch slots, conv1_1 fused, cout
                                               * fragments per wave, epilogue, kernel size (conv1x1_dma_kernel: ring, ks = 1) */
    int addup;               /* conv1x1_dma_kernel, BBOCR_ROUTE_DMA1X1_ADDUP: 1 = the up-sampling epilogue, 2 = a tensor of the output's own
                              * resolution added in the epilogue (the folded fc6 / fc7 / upconv1 stage) */
    int resw;                /* conv3x3_resw_kernel: 1 = 64 couts pooled, 2 = one chunk, 3 = two chunks */
    int OH, OW, TH, TW, PH, PW, NP, sub, stack, tiles_x, tiles_y, ntiles_n, nchunks, ntaps, lean;   /* geometry: output, tile, patch, patch
                              * slots, dilation phases (> 1: the sub-lattice route) and rows of one phase image, tile counts, 32-channel input
                              * chunks, taps, epilogue of conv3x3_dma_kernel (0 shared, 1 plain lean, 3 pooled lean) */
    int grid, threads;       /* workgroups, threads per workgroup */
    int persistent;          /* > 0: the launch caps the grid at persistent x compute units and loops over tiles; a dry run, which asks no
                              * device, reports the tile count as grid */
    int lds_bytes;           /* dynamic LDS */
    int tail, split_off;     /* epilogue switches that select no kernel (the networks' own launches only) */
} bbocr_conv_route;
/* pure host, no context, usable without a GPU: the route bbocr_op_conv2d would take for these arguments on a context of element type el
 * (0 bf16, 1 fp16), from a dry run of the launch code itself (the same dispatch, returning before the first HIP call).  store_full: with
 * pool_mode, whether dev_out is given too.  BBOCR_ERR_HIP with out->id = BBOCR_ROUTE_NONE and out->status set: the shape is refused, as
 * bbocr_op_conv2d would refuse it. */
int bbocr_host_conv_route(int el, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int dil, int relu_in, int relu_out,
                          int out_f32, int pool_mode, int pool_relu, int store_full, bbocr_conv_route* out);
/* the route the last bbocr_op_conv2d call on this context launched, recorded by the launch itself (id BBOCR_ROUTE_NONE: none yet, or refused) */
int bbocr_op_conv2d_route(bbocr_ctx* ctx, bbocr_conv_route* out);
/* recogniser network only: crops [n,64,imgW] (device, 16-bit elements of the context's RECOGNISER type: bf16 (BF16) / fp16 (FP16, MIXED) values already
 * normalised to [-1, 1]; BBOCR_PREC_EXACT: CODES, 0 = padding zero, 1 + grey level otherwise, from which the first layer rebuilds the
 * fp32 input ((g/255 - 0.5)/0.5) exactly) -> logits fp32 [n,T,cs] (device), T = imgW/4-1, cs = rec_classes rounded up to 16 (112 for the
 * 97 classes of english_g2; the columns behind the classes hold 0).  More than 128 classes: always through the unfused Prediction launch */
int bbocr_crnn_logits(bbocr_ctx* ctx, const uint16_t* dev_crops, int n, int imgW, float* dev_logits);
/* rec_quant contexts only: ONE dynamically quantised matrix product of the sequence half.  dev_x fp32 [rows, K] (device), seqs (host): nseq
 * pairs {first row, T} that tile [0, rows) in order -- one set of activation parameters per pair (crop).  layer: 0 / 1 = the input
 * projection of BiLSTM 0 / 1 (K 256 -> N 2048: column dir * 1024 + gate * 256 + unit, bias b_ih), 2 / 3 = the Linear behind BiLSTM 0 / 1
 * (512 -> 256), 4 = Prediction (256 -> 112: 97 classes, the rest 0).  Outputs: dev_out fp32 [rows, N], dev_codes uint8 [rows, K] (the 7-bit
 * codes, device), seg_params (host) [nseq][2] = {scale, zero point}. */
int bbocr_op_qlinear(bbocr_ctx* ctx, const float* dev_x, int rows, const int* seqs, int nseq, int layer, float* dev_out, uint8_t* dev_codes,
                     float* seg_params);
/* rec_quant contexts only: the recurrence of BiLSTM `layer` (0 / 1), both directions.  dev_g fp32 [rows, 2048]: the input projection as
 * bbocr_op_qlinear writes it; seqs as there (sequences of any mix of lengths; 16 share a workgroup).  Outputs (device, row = first row + t):
 * dev_h, dev_c fp32 [rows, 512] (forward | backward) = h and c AFTER step t; dev_hcodes uint8 [rows, 512] and dev_hparams fp32 [rows][2][2] =
 * the codes and {scale, zero point} of the h that ENTERED step t of each direction (h of t - 1 forward, of t + 1 backward, zeros at a
 * direction's first step). */
int bbocr_op_qlstm(bbocr_ctx* ctx, const float* dev_g, int rows, const int* seqs, int nseq, int layer, float* dev_h, float* dev_c, uint8_t* dev_hcodes,
                   float* dev_hparams);
/* CTC decode of logits fp32 [n,T,cs]: host outputs text_off [n+1], text_idx (<= n*T), conf [n]; ignore_mask (host): the class mask, 4 words
 * for C <= 128 (bbocr_params::ignore_mask), ceil(C / 32) words for a wider C (the wide rows kernel, one wavefront per row), or NULL;
 * beam_width <= 0: greedy, > 0: ctcBeamSearch with that width (bbocr_params::decoder; C > 128: on the host, or on the device on a context with beam_wide).  C > 128 is taken on a context
 * created with rec_classes > 128 (then up to BBOCR_REC_CLASSES_MAX) and is BBOCR_ERR_ARG on any other, here and in the two entry points below */
int bbocr_op_ctc(bbocr_ctx* ctx, const float* dev_logits, int n, int T, int C, int cs, int* text_off, int* text_idx, double* conf,
                 const unsigned int* ignore_mask, int beam_width);
/* the probabilities alone, as the CTC stage's row kernel writes them: softmax of logits fp32 [rows,cs] over C classes (C <= 128: ctc_rows_kernel,
 * wider: ctc_rows_wide_kernel), the classes of ignore_mask (host words as in bbocr_op_ctc, or NULL) zeroed, the rest renormalised ->
 * dev_probs_out fp32 [rows,cs] (device; columns >= C are neither read nor written) */
int bbocr_op_ctc_probs(bbocr_ctx* ctx, const float* dev_logits, size_t rows, int C, int cs, const unsigned int* ignore_mask,
                       float* dev_probs_out);
/* the same with arg-max, collapse and confidence product kept: dev_probs_out may be NULL; idx, pmax [rows], out_idx [rows] and ctc_out
 * [nseq][4] = {len, cnt, prod bits, 0} are DEVICE tensors the caller owns (what a recognition pass reads back); seqs (host) = {first row, T} */
int bbocr_op_ctc_rows(bbocr_ctx* ctx, const float* dev_logits, size_t rows, int C, int cs, const unsigned int* ignore_mask, const int* seqs,
                      int nseq, float* dev_probs_out, int* dev_idx, float* dev_pmax, int* dev_out_idx, int* dev_ctc_out);
/* Prediction alone, as a sequence pass of a 16-bit precision launches it on the unfused route (the conv plan over rows padded to whole
 * 256-row tiles): dev_x [rows, 256] elements of the recogniser type -> dev_logits fp32 [rows, cs], cs = rec_classes rounded up to 16 */
int bbocr_op_pred(bbocr_ctx* ctx, const uint16_t* dev_x, size_t rows, float* dev_logits);
/* contexts of more than 128 classes in a 16-bit precision: Prediction + softmax + mask + arg-max of a recognition pass's greedy route as the
 * ONE kernel that stores no logits (pred_ctc.hip), alone, with the context's Prediction weights.  dev_x: [rows, 256] elements of the
 * recogniser type (the second BiLSTM stage's output); dev_mask_words: n_words (<= ceil(rec_classes / 32)) DEVICE words or NULL; outputs
 * (device): dev_idx int32 [rows] = the unmasked class of the largest logit (lowest index among equals), dev_pmax fp32 [rows] = its
 * renormalised probability (e_best / sum_all) / (sum_unmasked / sum_all) */
int bbocr_op_pred_ctc(bbocr_ctx* ctx, const uint16_t* dev_x, size_t rows, const uint32_t* dev_mask_words, int n_words, int* dev_idx,
                      float* dev_pmax);
/* the device beam search alone (the kernel behind decoder == BEAMSEARCH for widths <= BBOCR_BEAM_DEVICE_MAX): dev_probs fp32 [rows,cs]
 * (device), seqs (host) = {first row, T} per sequence, ragged, T = 0 allowed -> text_off [nseq+1], text_idx (<= the sum of T), both host.
 * The text equals bbocr_host_ctc_beam's on the same rows, exactly.  BBOCR_ERR_ARG before anything is queued: a null pointer, cs < C,
 * C > 128, beam_width < 1 or > BBOCR_BEAM_DEVICE_MAX, a sequence outside [0, rows), a T too long for the kernel's LDS block at this width
 * (see BBOCR_BEAM_DEVICE_MAX) */
int bbocr_op_ctc_beam(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width,
                      int* text_off, int* text_idx);
/* the stages of decoder == WORDBEAMSEARCH on the device alone (csrc/ctc_wordbeam.hip).  All arguments are checked before anything is queued;
 * BBOCR_ERR_ARG leaves every output untouched.
 * bbocr_op_word_segments: dev_idx int32 [rows] (arg-max rows), seqs {first row, T} -> the word groups of sequence i as {first row, T} pairs
 * segs[2 * seg_off[i] .. 2 * seg_off[i + 1]) (host arrays: seg_off [nseq + 1], segs with room for sum((T + 1) / 2) pairs).
 * bbocr_op_dict_lookup: n_q class-index strings (q_symbols / q_off) -> found[q] = 0 / 1 through a DEVICE table: the context's dictionary when
 * n_words == 0, else a table built for this call from symbols / word_off / n_words (symbols 1 .. 127) with n_slots slots (0: the default,
 * else a power of two above n_words -- a small one forces long probe runs); *longest_probe (may be null) reports the table's.
 * bbocr_op_ctc_wordbeam: as bbocr_op_ctc_beam, with the context's dictionary (BBOCR_ERR_ARG without one); the text equals
 * bbocr_host_ctc_wordbeam's on the same rows, exactly. */
int bbocr_op_word_segments(bbocr_ctx* ctx, const int* dev_idx, size_t rows, const int* seqs, int nseq, int space_class, int* seg_off, int* segs);
int bbocr_op_dict_lookup(bbocr_ctx* ctx, const uint16_t* symbols, const int* word_off, int n_words, int n_slots, const uint16_t* q_symbols,
                         const int* q_off, int n_q, int* found, int* longest_probe);
int bbocr_op_ctc_wordbeam(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width, int* text_off,
                          int* text_idx);
/* the device beam search over more than 128 classes alone (the kernels behind decoder == BEAMSEARCH on a context with beam_wide): arguments
 * and outputs as bbocr_op_ctc_beam's, for 128 < C <= BBOCR_REC_CLASSES_MAX on a context created with rec_classes > 128 (beam_wide need not be
 * set).  *n_host (may be NULL): the sequences that had a row of more than 128 candidates and were searched on the host.  The text equals
 * bbocr_host_ctc_beam's on the same rows, exactly.  BBOCR_ERR_ARG before anything is queued, with nothing written: a null pointer, cs < C, C
 * outside that range or a narrower context, beam_width < 1 or > BBOCR_BEAM_DEVICE_MAX, a sequence outside [0, rows), a T too long for the
 * kernel's LDS block at this width (see BBOCR_BEAM_DEVICE_MAX) */
int bbocr_op_ctc_beam_wide(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width,
                           int* text_off, int* text_idx, int* n_host);
/* ctc_route, the rule by which a sequence pass picks its CTC route (the values of bbocr_last_ctc_route), on the host alone: beam_wide as in
 * bbocr_config, beam_width <= 0 for greedy, C classes, seqs = {first row, T} per sequence.  No context, no device. */
int bbocr_host_ctc_route(int beam_wide, int beam_width, int C, const int* seqs, int nseq);
/* cv2.resize(INTER_LINEAR) on uint8 [N,sh,sw,C] -> [N,dh,dw,C] (device) */
int bbocr_op_resize_u8(bbocr_ctx* ctx, const uint8_t* dev_src, int N, int sh, int sw, int C, uint8_t* dev_dst, int dh, int dw);
/* JPEG pages decoded ONCE on the host into libjpeg's YCbCr triples (out_color_space = JCS_YCbCr; PIL: draft("YCbCr")): uint8 [npix,3]
 * (device) -> the RGB image libjpeg's own ycc_rgb_convert yields (what skimage / cv2.imread hand easyocr.utils.reformat_input,
 * reader.readtext at enhanced_extractor.py:520) and, when dev_gray is not NULL, the Y plane = cv2.imread(IMREAD_GRAYSCALE)'s
 * plane; both bit for bit (tests/test_oracle_cpu.py pins the formula against the decoder) */
int bbocr_op_ycc_to_rgb(bbocr_ctx* ctx, const uint8_t* dev_ycc, size_t npix, int pixel_stride, uint8_t* dev_rgb, uint8_t* dev_gray);
/* n separately allocated host pages of bytes_each bytes (the arrays a decode pool returns) -> one device buffer [n][bytes_each], copied
 * inside ONE call: a Python host releases its interpreter lock once per batch instead of once per page, and needs no host-side
 * concatenation of the pages (236 MB for 64 pages of 1280x960).  pixel_stride above: 3 = tight triples, 4 = Pillow's own 4-byte pixel
 * storage (Y Cb Cr x) uploaded as it is.  Every page pointer is checked before the first copy is queued: a call refused with
 * BBOCR_ERR_ARG has written nothing to dev_dst. */
int bbocr_upload_pages(bbocr_ctx* ctx, const void* const* host_pages, int n, size_t bytes_each, void* dev_dst);
/* recogniser inputs for explicit boxes of ONE gray page: fills crops [n,64,imgW] (in box order) of 16-bit elements of the context's
 * RECOGNISER type, as bbocr_crnn_logits reads them (bf16 / fp16 values normalised to [-1, 1]; BBOCR_PREC_EXACT: codes 1 + grey level, the
 * pad columns carry the last content column's code); returns their count in *n_out.  contrast != 0 applies adjust_contrast_grey first.
 * mode 0: the boxes whose own padded width is imgW (Reader.recognize's per-box branch); mode 1..4: EVERY box at the forced width imgW, rotated by np.rot90(crop, mode - 1) (the batched branch rotation_info takes) */
int bbocr_op_crops(bbocr_ctx* ctx, const uint8_t* dev_gray, int H, int W, const int* hori, int n_hori, const double* free_q, int n_free,
                   int imgW, float contrast, uint16_t* dev_out, int* n_out, int mode);
/* the same for explicit boxes of n gray pages of their own shapes (the page-table variant of the crop kernels, what bbocr_readtext_pages
 * launches): pages[k].dev_gray / gray_pitch / H / W are read (in place; dev_rgb is ignored), page k's boxes are hori [hori_off[k],
 * hori_off[k+1]) and free_q [free_off[k], free_off[k+1]).  dev_out receives the crops page after page, per page in bbocr_op_crops' order:
 * what n bbocr_op_crops calls write, back to back. */
int bbocr_op_crops_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, const int* hori, const int* hori_off, const double* free_q,
                         const int* free_off, int imgW, float contrast, uint16_t* dev_out, int* n_out, int mode);

/* ---- OCR pre-processing chain of the reference ----
 * pipeline_demo/ocr_testing/preprocessing/image_preprocessor.py::preprocess_for_book_cover (:147-160) on ONE decoded page:
 * dev_bgr uint8 [H,W,3] in cv2.imread's channel order -> dev_out uint8 [int(H*1.5), int(W*1.5)] (gray): BGR2GRAY, x1.5
 * INTER_CUBIC, GaussianBlur 3x3 sigma 3, PIL Contrast 1.9, PIL Brightness 1.2, CLAHE (clip 2.5, 8x8 tiles),
 * PIL UnsharpMask(radius 1, 30 %, threshold 3).  out_h / out_w receive the output size (pass dev_out = NULL to query it). */
int bbocr_preprocess_book_cover(bbocr_ctx* ctx, const uint8_t* dev_bgr, int H, int W, uint8_t* dev_out, int* out_h, int* out_w);
/* The same ImagePreprocessor stage sequence with its parameters spelled out (a stage whose parameter is 0 is skipped).
 * bbocr_preproc_defaults(p, 0) = the pipeline_demo chain above; (p, 1) = the LEGACY chain of
 * pipeline_components/img_to_json/ocr_testing/preprocessing/image_preprocessor.py:221-252 (sigma 5, contrast 1.3, no brightness
 * step, CLAHE 2.0, unsharp 20 %) -- the one whose stored outputs (results/images/book*_preprocessed.png) pin the stages. */
typedef struct bbocr_preproc_params {
    double scale;           /* resize(scale_factor): new size int(H*s) x int(W*s), cv2.INTER_CUBIC */
    double blur_sigma;      /* denoise(strength): cv2.GaussianBlur 3x3, sigma */
    double contrast;        /* increase_contrast(factor): PIL ImageEnhance.Contrast */
    double brightness;      /* increase_brightness(factor): PIL ImageEnhance.Brightness */
    double clahe_clip;      /* clahe(clip_limit), 8x8 tiles */
    double unsharp_radius;  /* sharpen: PIL UnsharpMask radius (1.0) */
    int unsharp_percent;    /* int(amount * 100) */
    int unsharp_threshold;  /* 3 */
    int reserved[4];
} bbocr_preproc_params;
void bbocr_preproc_defaults(bbocr_preproc_params* p, int legacy);
int bbocr_preprocess_chain(bbocr_ctx* ctx, const uint8_t* dev_bgr, int H, int W, const bbocr_preproc_params* p, uint8_t* dev_out, int* out_h,
                           int* out_w);
/* the chain's stages one by one (parity tests): stage 0 = resize cubic of a gray plane to (dh, dw), 1 = GaussianBlur 3x3
 * sigma `param`, 2 = PIL Contrast `param`, 3 = PIL Brightness `param`, 4 = CLAHE clip `param` 8x8, 5 = PIL UnsharpMask
 * (radius `param`, 30 %, threshold 3), 6 = cv2 BGR2GRAY of an interleaved [H,W,3] plane (the gray plane reformat_input derives from
 * arrays), 7 = PIL UnsharpMask (radius 1, `param` %, threshold 3).  Stages 1-7 keep the size (dh = H, dw = W). */
int bbocr_op_preprocess_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, uint8_t* dev_dst, int dh, int dw, double param);
/* Which kernel a launch of the chain takes.  Every launcher picks between a dword kernel and a byte-wise one (or between tile sizes) from
 * the plane's size and from the low two bits of its source and destination pointers; each choice is one host function, which the launcher
 * itself switches on and which the bbocr_host_pp_*_route calls below report. */
enum {
    BBOCR_PP_GAUSS_X4 = 0,          /* pp_gauss3_x4_kernel: W % 4 == 0, W >= 8, both pointers 4-byte aligned */
    BBOCR_PP_GAUSS_BYTE,            /* pp_gauss3_kernel */
    BBOCR_PP_HIST_X4,               /* pp_clahe_hist_x4_kernel: W % 4 == 0, source aligned */
    BBOCR_PP_HIST_BYTE,             /* pp_clahe_hist_kernel */
    BBOCR_PP_APPLY_CELL_2,          /* pp_clahe_apply_cell_kernel (W % 4 == 0, aligned, H * W >= 1 << 14), 2 row chunks per cell */
    BBOCR_PP_APPLY_CELL_8,          /* the same, 8 chunks: tile height >= 64 */
    BBOCR_PP_APPLY_CELL_32,         /* the same, 32 chunks: tile height >= 512 */
    BBOCR_PP_APPLY_VEC,             /* pp_clahe_apply_kernel with dword loads / stores: a smaller W % 4 == 0, aligned plane */
    BBOCR_PP_APPLY_BYTE,            /* pp_clahe_apply_kernel byte-wise */
    BBOCR_PP_BOX0_X4,               /* pp_box0_x4_kernel: one box pass of radius 0, W % 4 == 0, aligned */
    BBOCR_PP_BOX_BYTE,              /* pp_box_pass_kernel */
    BBOCR_PP_UNSHARP_FUSED,         /* pp_box0_h3_kernel + pp_box0_v3_unsharp_kernel: box radius 0, W % 4 == 0, every plane aligned */
    BBOCR_PP_UNSHARP_PASSES_VEC,    /* six box passes (each BOX0_X4 or BOX_BYTE), then pp_unsharp_kernel over dwords with a byte tail: aligned */
    BBOCR_PP_UNSHARP_PASSES_BYTE,   /* six box passes, then pp_unsharp_kernel byte-wise: a misaligned source or destination */
    BBOCR_PP_RESIZE_TILED32,        /* pp_resize_cubic_tiled_kernel, 64 x 32 output tiles */
    BBOCR_PP_RESIZE_TILED16,        /* the same, 64 x 16 tiles */
    BBOCR_PP_RESIZE_PIXEL,          /* pp_resize_cubic_kernel: the source window of a tile does not fit */
    BBOCR_PP_ROUTE_COUNT
};
/* pure host, no context, usable without a GPU: the BBOCR_PP_* route bbocr_op_preprocess_stage takes for an H x W plane whose source and
 * destination pointers have the low two bits src_bits / dst_bits (0..3); the stage's own scratch planes are aligned.  resize: stage 0;
 * gauss: stage 1, and stage 2's pixel sum (destination: a scratch plane, dst_bits 0); clahe_hist / clahe_apply: the two plane passes of
 * stage 4, BBOCR_ERR_ARG for a plane smaller than the tile grid's padding, which the stage refuses; unsharp: stages 5 and 7 (radius 1);
 * box: one of the six box passes behind BBOCR_PP_UNSHARP_PASSES_* (r = bbocr_host_pp_unsharp_box_radius(radius); the first pass reads the
 * stage's source, all six write scratch planes).  Any other bad argument: BBOCR_ERR_ARG. */
int bbocr_host_pp_resize_route(int H, int W, int dh, int dw);
/* 1: the tiled resize kernels store their full 64-column tiles as whole dwords (dw % 4 == 0, destination aligned), 0: byte-wise.  The
 * launcher passes this very value to the kernel */
int bbocr_host_pp_resize_dword_rows(int dw, int dst_bits);
int bbocr_host_pp_gauss_route(int H, int W, int src_bits, int dst_bits);
int bbocr_host_pp_clahe_hist_route(int H, int W, int src_bits);
int bbocr_host_pp_clahe_apply_route(int H, int W, int src_bits, int dst_bits);
int bbocr_host_pp_box_route(int H, int W, int r, int src_bits, int dst_bits);
int bbocr_host_pp_unsharp_route(int H, int W, double radius, int src_bits, int dst_bits);
int bbocr_host_pp_unsharp_box_radius(double radius);

/* ---- text-region auto-crop (enhanced_extractor.py::_auto_crop_text_region, the extractor's `crop_for_ocr`) of one u8 page on the
 * device: gray [H,W] (channels 1) or BGR [H,W,3] (channels 3), rows `pitch` bytes apart (a crop of a larger plane is passed as a
 * pointer + pitch).  box = (x0, y0, x1, y1) of the crop with `margin` applied, *found = 0 when the reference returns None (then box is
 * zeros).  comp_boxes receives min(*n_comps, max_comps) kept component boxes (x, y, w, h), sorted by (y, x); comp_boxes may be null
 * when max_comps is 0.  A pipeline call: runs in a call slot next to readtext calls, returns with its work finished.  BBOCR_ERR_ARG,
 * before anything is queued: null pointers, H or W < 1, pitch < W * channels, channels not 1 or 3, margin < 0, a page smaller than
 * the 8x8 CLAHE grid allows. */
int bbocr_auto_crop(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int channels, int margin, int box[4], int* found,
                    int* comp_boxes, int max_comps, int* n_comps);
/* its intermediates as u8 [H,W] in dev_dst (parity tests): stage 0 = CLAHE output, 1 = composite threshold mask (0/255), 2 = merged
 * morphology mask, 3 = pixels of the external (RETR_EXTERNAL) components of the merged mask */
int bbocr_op_autocrop_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int channels, uint8_t* dev_dst);
/* the same morphology and component code on a mask the caller designs (parity tests): dev_mask is a byte plane [H,W], nonzero = set, rows
 * `pitch` bytes apart; dev_dst receives u8 [H,W] of 0 / 255.  MERGED: the merged morphology mask of dev_mask.  EXTERNAL: the pixels of
 * the external components of that merged mask.  COMPONENTS: the pixels of the external components of dev_mask itself, no morphology.
 * The last two report every external component's bounding box before any area filter: *n_boxes of them, the first
 * min(*n_boxes, max_boxes) as (x, y, w, h) in `boxes`, in no particular order (boxes may be null when max_boxes is 0); MERGED sets
 * *n_boxes = 0.  Any H, W >= 1: the CLAHE grid rule of the page entries does not apply.  BBOCR_ERR_ARG before anything is queued:
 * null pointers, H or W < 1, pitch < W, an unknown mode, max_boxes < 0. */
enum { BBOCR_AC_MASK_MERGED = 0, BBOCR_AC_MASK_EXTERNAL = 1, BBOCR_AC_MASK_COMPONENTS = 2 };
int bbocr_op_autocrop_mask_stage(bbocr_ctx* ctx, int mode, const uint8_t* dev_mask, int H, int W, long long pitch, uint8_t* dev_dst, int* boxes,
                                 int max_boxes, int* n_boxes);

/* ---- OCR-input thumbnail (enhanced_extractor.py:486-512, the step between the crops and readtext) of one u8 page on the device: a page
 * whose longer side exceeds max_dim becomes Image.thumbnail((max_dim, max_dim)) in RGB (Pillow 12: reduce by int(size / out / 2) when that
 * is > 1, then bicubic with 22-bit fixed-point weights) and goes through the lossy half of a baseline 4:2:0 ISLOW JPEG file of the given
 * quality (libjpeg-turbo: colour conversion, edge replication, downsampling, DCT, quantisation, IDCT, fancy upsampling).  dev_rgb
 * [out_h,out_w,3] and dev_gray [out_h,out_w] receive what easyocr reads from that file: the RGB decode and libjpeg's Y plane, to the bit.
 * A page at or below max_dim is passed on as the reference reads it: gray -> replicated RGB + itself, RGB / BGR -> RGB + libpng's gray
 * (9797 R + 19234 G + 3737 B) >> 15, YCbCr -> libjpeg's RGB + Y.  quality <= 0: no JPEG (the resized page, gray by the same rules).
 * Pages: rows `pitch` bytes apart (a crop of a larger plane is a pointer + pitch), layout BBOCR_PAGE_*; YCBCR4 is Pillow's padded
 * decode (decode_file_ycc(padded=True)).  A pipeline call: runs in a call slot next to readtext calls, scratch from the slot, returns
 * with its work finished.  BBOCR_ERR_ARG before anything is queued: null pointers, H or W < 1, an unknown layout, pitch shorter than
 * a row, max_dim < 1, quality > 100. */
enum { BBOCR_PAGE_GRAY = 0, BBOCR_PAGE_BGR = 1, BBOCR_PAGE_RGB = 2, BBOCR_PAGE_YCBCR4 = 3, BBOCR_PAGE_YCBCR3 = 4 };
int bbocr_ocr_thumbnail(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int max_dim, int quality, uint8_t* dev_rgb,
                        uint8_t* dev_gray, int* out_h, int* out_w);
/* ---- EXIF orientation + channel order of one u8 page on the device (csrc/orient.hip): what cv2.imread does behind its decoder.  Source:
 * [H,W] pixels of any BBOCR_PAGE_* layout, rows `pitch` bytes apart.  Destination: [H',W',c] in dst_layout, rows dst_pitch apart, (H', W') =
 * (H, W) for orientations 1 .. 4 and (W, H) for 5 .. 8; BBOCR_PAGE_BGR or BBOCR_PAGE_RGB from every source (GRAY replicated, YCbCr through
 * libjpeg's integer conversion), BBOCR_PAGE_GRAY from GRAY.  Geometry = PIL.ImageOps.exif_transpose = OpenCV's ExifTransform:
 *   1 as it is, 2 mirror columns, 3 rotate 180, 4 mirror rows, 5 transpose, 6 rotate 90 clockwise, 7 transverse, 8 rotate 90 counter-clockwise.
 * out_h / out_w receive (H', W'); dev_dst = NULL is a size query.  Source and destination must not overlap.  Bytes of a destination row
 * behind W' * c are left as they are.  A pipeline call: runs in a call slot, returns with its work finished.  BBOCR_ERR_ARG before anything
 * is queued: null pointers, H or W < 1, an unknown layout or layout pair, orientation outside 1 .. 8, a pitch shorter than a row. */
int bbocr_page_orient(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int orientation, int dst_layout,
                      uint8_t* dev_dst, long long dst_pitch, int* out_h, int* out_w);
/* its parts (parity tests): stage 0 = the thumbnail alone (reduce + resize) as RGB [out_h,out_w,3] in dev_dst (a page at or below
 * max_dim: the page as RGB); stage 1 = the JPEG round trip alone of a gray or RGB page, RGB -> dev_dst [H,W,3], Y -> dev_gray [H,W];
 * stage 2 = the upsampled YCbCr triple of that round trip, before the colour conversion, in dev_dst [H,W,3].  Stages 1 and 2 need
 * 1 <= quality <= 100; dev_gray is only read by stage 1. */
int bbocr_op_thumbnail_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int max_dim, int quality,
                             uint8_t* dev_dst, uint8_t* dev_gray, int* out_h, int* out_w);
/* host only: Image.thumbnail's output size ((H, W) when no thumbnail is taken) */
int bbocr_thumbnail_dims(int H, int W, int max_dim, int* out_h, int* out_w);
/* host only: the plan of that thumbnail -- output size, reduce factors (x, y), the reduced region (x0, y0, x1, y1) and the float box
 * (x0, y0, x1, y1) handed to the bicubic resample in the reduced image */
int bbocr_host_thumbnail_plan(int H, int W, int max_dim, int* out_h, int* out_w, int factors[2], int reduce_box[4], float resize_box[4]);
/* ---- the resize Image.thumbnail runs after a JPEG draft: Image.resize((out_w, out_h), BICUBIC, box=(0, 0, box_w, box_h),
 * reducing_gap=2.0) of an H x W page for a float box that ends inside the last pixel (W - 1 < box_w <= W, H - 1 < box_h <= H; the draft's
 * box is the original size over the draft scale, e.g. 535.5 rows of a 536-row decode).  The reduce factors are int(box / out / 2) or 1,
 * the reduce step covers the whole page, and the bicubic resample gets the box (0, 0, box_w / fx, box_h / fy) as C floats.  dev_dst
 * receives RGB [out_h,out_w,3] (YCbCr pages: libjpeg's RGB), or the samples [out_h,out_w] of a BBOCR_PAGE_GRAY page; any layout, rows
 * `pitch` bytes apart.  A pipeline call like bbocr_ocr_thumbnail; any other box: BBOCR_ERR_ARG.  bbocr_host_resize_plan: host only, the
 * factors (x, y) and the box handed to the resample. */
int bbocr_thumbnail_box(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int out_h, int out_w, double box_w,
                        double box_h, uint8_t* dev_dst);
int bbocr_host_resize_plan(int H, int W, int out_h, int out_w, double box_w, double box_h, int factors[2], float resize_box[4]);
/* host only: Pillow's bicubic coefficients of one axis (precompute_coeffs + normalize_coeffs_8bpc): bounds [out][2] = (first, count),
 * coeffs [out][max_ksize] (22-bit fixed point).  *ksize is always set; bounds = coeffs = NULL is a size query. */
int bbocr_host_resample_coeffs(int in_size, float in0, float in1, int out_size, int* bounds, int* coeffs, int max_ksize, int* ksize);
/* host only: jpeg_set_quality(quality, TRUE)'s luminance (0..63) and chrominance (64..127) tables, natural order */
int bbocr_host_jpeg_qtables(int quality, uint16_t* out);


/* ---- baseline JPEG files decoded on the device (csrc/jpegdec.hip), to the bit of libjpeg-turbo / Pillow: only the file's bytes cross the
 * link.  Taken: SOF0, 8 bit, Huffman, ONE interleaved scan, 3 components YCbCr 4:2:0 (JFIF, or Adobe transform 1: decode_file_ycc's
 * rule) or 1 component, any DQT / DHT / DRI, any size.  Everything else is refused by the plan, and the caller keeps its host path.
 * Opt-in beside that scope: 3 components sampled 4:4:4, 4:2:2 or 4:4:0 that are otherwise inside it.  The plan still reports them as
 * refused (supported 0, reason BBOCR_JPEG_SAMPLING) and names their class in `chroma`; bbocr_jpeg_decode / bbocr_jpeg_imread take a file
 * whose `chroma` is not 0, so a caller that asks for them hands such a file over and every other caller behaves as before.
 * bbocr_jpeg_decode ignores the EXIF orientation, as the host path of readtext ignores it; the plan reports it, and bbocr_jpeg_imread
 * applies it: cv2.imread's page, which the extractor's crop settings read. */
enum {
    BBOCR_JPEG_OK = 0,
    BBOCR_JPEG_NOT_JPEG = 1,    /* no SOI: another container */
    BBOCR_JPEG_TRUNCATED = 2,   /* the headers end before SOS (a marker segment cut short, EOI before any scan) */
    BBOCR_JPEG_NO_EOI = 3,      /* the entropy-coded data runs to the end of the file */
    BBOCR_JPEG_SOF = 4,         /* extended, progressive, lossless or arithmetic-coded frame; no or a second frame header */
    BBOCR_JPEG_PRECISION = 5,   /* 12-bit samples, 16-bit quantisation table */
    BBOCR_JPEG_COMPONENTS = 6,  /* CMYK / YCCK / two components */
    BBOCR_JPEG_SAMPLING = 7,    /* any sampling but 4:2:0; 4:4:4, 4:2:2 and 4:4:0 files are decodable all the same when plan.chroma != 0 */
    BBOCR_JPEG_COLORSPACE = 8,  /* three components without JFIF or Adobe transform 1: may be RGB-coded */
    BBOCR_JPEG_MULTISCAN = 9,   /* a scan that does not hold every component, or more after the first */
    BBOCR_JPEG_TABLES = 10,     /* a table the scan names is missing or malformed */
    BBOCR_JPEG_RESTART = 11,    /* restart markers out of sequence, or not one per interval */
    BBOCR_JPEG_SCRIPT = 12,     /* bbocr_host_jpeg_progressive_plan only: the progression is invalid (T.81 G.1.1) or incomplete */
    BBOCR_JPEG_SCANS = 13       /* bbocr_host_jpeg_progressive_plan only: more than BBOCR_JPEG_MAX_SCANS scans */
};
enum { BBOCR_JPEG_CHROMA_444 = 1, BBOCR_JPEG_CHROMA_422 = 2, BBOCR_JPEG_CHROMA_440 = 3 };   /* bbocr_jpeg_plan::chroma */
/* A file of a chroma class (chroma != 0) has supported == 0 and reason == BBOCR_JPEG_SAMPLING like every other file outside 4:2:0, and
 * every other field filled exactly as for a supported file: mcu_cols / mcu_rows count MCUs of 8 h x 8 v pixels, (h, v) = sampling[0],
 * and segments, scan_offset, scan_bytes describe its scan.  Such a file passed every check behind the sampling test (colour space, one
 * interleaved scan, tables, restart sequence, EOI); one that fails any of them has chroma == 0 and those fields 0. */
typedef struct bbocr_jpeg_plan {
    int width, height, components;
    int sampling[3][2];         /* (h, v) per component */
    int restart_interval;       /* MCUs, 0 = none */
    int mcu_cols, mcu_rows;
    int segments;               /* restart segments = entry points known without decoding */
    long long scan_offset;      /* first entropy-coded byte */
    long long scan_bytes;       /* up to the marker that ends the scan (stuffing and restart markers included) */
    int supported;              /* 1: bbocr_jpeg_decode takes the file (it also takes one whose `chroma` is not 0) */
    int reason;                 /* BBOCR_JPEG_* */
    int orientation;            /* EXIF orientation 1 .. 8 as cv2.imread applies it, 1 = none: the first APP1 "Exif\0\0" segment before SOS, TIFF header
                                 * of either byte order, IFD0 only, tag 0x0112 as ONE SHORT or LONG of value 1 .. 8.  Everything else is 1: no such
                                 * segment or tag, a tag only in IFD1, another type or count, value 0 / 9 / 65535, an IFD offset or entry count that
                                 * leaves the segment.  Filled for every file that starts with SOI, refused ones included; malformed EXIF changes no
                                 * other field.  XMP's tiff:Orientation is not read (OpenCV does not read it; Pillow's exif_transpose does, when the
                                 * EXIF block has no tag: the one difference to preprocess._imread_bgr). */
    int reserved[2];
    int chroma;                 /* 0: inside today's scope, or refused for another reason; BBOCR_JPEG_CHROMA_444 (luma sampled 1x1), _422 (2x1) or
                                 * _440 (1x2) over 1x1 chroma: bbocr_jpeg_decode / bbocr_jpeg_imread take the file although `supported` is 0 */
} bbocr_jpeg_plan;
/* host only, no GPU: one linear pass over the file (markers, then the scan's FF bytes); no entropy bit is decoded.  Fields a refused
 * file's headers did not reach stay 0. */
int bbocr_host_jpeg_plan(const uint8_t* file, size_t bytes, bbocr_jpeg_plan* plan);
/* n files (HOST bytes) -> pixels in DEVICE memory, one call per batch: dev_out[k] receives file k's libjpeg YCbCr triples (out_color_space
 * JCS_YCbCr, what decode_file_ycc holds), rows pitches[k] bytes apart, 3 (layout BBOCR_PAGE_YCBCR3) or 4 (BBOCR_PAGE_YCBCR4, fourth byte
 * 255) bytes per pixel -- bbocr_op_ycc_to_rgb's two inputs -- or, for a 1-component file, the samples themselves, one byte per pixel.
 * status[k]: 0, BBOCR_ERR_ARG (null pointer, pitch shorter than a row, a file the plan refuses and gives no chroma class) or BBOCR_ERR_DATA (the entropy-coded
 * data decodes to another block count than the headers promise, or holds a bit pattern without a code: dev_out[k] is then undefined);
 * the other files of the batch are decoded all the same and the context stays usable.  Runs on a stream of its own outside the call
 * slots, one batch at a time per context (bbocr_upload_pages' contract): a batch decodes while two pipeline calls are in flight.  Work
 * buffers belong to the context and grow on demand.  Returns with its work finished, also when it fails. */
int bbocr_jpeg_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, uint8_t* const* dev_out,
                      const long long* pitches, int* status);
/* cv2.imread(path) of n files on the device: bbocr_jpeg_decode followed by the orientation the plan reports, written as BGR (a
 * 1-component file replicated).  dev_out[k]: uint8 [H',W',3], rows pitches[k] >= 3 * W' bytes apart, (H', W') = the plan's (height, width),
 * swapped for orientations 5 .. 8.  Same stream, same one-batch-at-a-time contract and same per-file status as bbocr_jpeg_decode (a
 * pitch shorter than the ORIENTED row: BBOCR_ERR_ARG).  The un-oriented decode lives in a buffer of the context that grows on demand. */
int bbocr_jpeg_imread(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dev_out, const long long* pitches,
                      int* status);
/* its intermediates of ONE file (parity tests), cut into subsequences of subseq_bits bits (0 = the decoder's 1024; a multiple of 8 in
 * 32 .. 65536): stage 0 = the exact entry state of every subsequence, int32 [subsequences][4] = (bit in the unstuffed scan, block in the
 * MCU, zig-zag position, first output block); 1 = quantised coefficients int16 [blocks][64] in natural order, blocks in MCU order, DC
 * terms summed; 2 = the component planes before upsampling, Y [mcu_rows * 16][mcu_cols * 16] then Cb, Cr at half that (1 component:
 * [mcu_rows * 8][mcu_cols * 8]; a file of a chroma class: Y [mcu_rows * 8 v][mcu_cols * 8 h], then Cb and Cr, each
 * [mcu_rows * 8][mcu_cols * 8]); 3 = the pixels, tight; 4 = the status word the write pass raised for the file, int32 [1]: 0, or the sum
 * of 1 (a subsequence entered in another state than its left neighbour left), 2 (a bit pattern without a code) and 4 (another block count
 * than the headers promise, or a restart segment that ends inside a block).  *file_status as status[k] above. */
int bbocr_op_jpeg_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int subseq_bits, void* dev_dst, size_t dst_bytes,
                        int* file_status);
/* ---- the decode at reduced scale: what Pillow's draft (decoderconfig == (scale, 0)) and hence Image.thumbnail of an unloaded JPEG file get
 * from libjpeg-turbo, to the bit.  bbocr_jpeg_decode_scaled is bbocr_jpeg_decode -- same arguments, stream, contract and status codes --
 * with one `scale` per batch: 1 (bbocr_jpeg_decode itself), 2, 4 or 8.  At scale s > 1 file k comes out ceil(height / s) rows of
 * ceil(width / s) pixels (bbocr_jpeg_scaled_dims; pitches[k] at least such a row): luma blocks through jidctred.c's n x n IDCT, n = 8 / s,
 * the chroma blocks of a 4:2:0 file through the 2n x 2n one (jdmaster.c's per-component DCT_scaled_size), so that nothing is upsampled; the
 * entropy stages are those of the full-scale decode.  Only the files inside the plan's own scope (supported == 1: 4:2:0 or one component)
 * are decoded at s > 1: a file of a chroma class (4:4:4, 4:2:2, 4:4:0), like every file the plan refuses, gets status[k] = BBOCR_ERR_ARG,
 * the rest of the batch is decoded, and the caller keeps its host path for it -- or hands it to bbocr_jpeg_decode_scales below, which
 * decodes those classes at every scale. */
int bbocr_jpeg_decode_scaled(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, int scale,
                             uint8_t* const* dev_out, const long long* pitches, int* status);
/* host only: (ceil(H / scale), ceil(W / scale)); scale 1, 2, 4 or 8 */
int bbocr_jpeg_scaled_dims(int H, int W, int scale, int* out_h, int* out_w);
/* intermediates of ONE file's decode at scale 2, 4 or 8 (parity tests), numbered like bbocr_op_jpeg_stage's: stage 2 = the component
 * planes, each [mcu_rows * e][mcu_cols * e] with e = 16 / scale for a 4:2:0 file (Y, then Cb, then Cr: all of the output's size) and
 * e = 8 / scale for a 1-component file (Y alone); 3 = the pixels, tight.  A file outside the scaled decode's scope: BBOCR_ERR_ARG. */
int bbocr_op_jpeg_scaled_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int scale, void* dev_dst, size_t dst_bytes,
                               int* file_status);
/* ---- several decodes of a batch from ONE entropy pass, every chroma class at every scale.  bbocr_jpeg_decode_scales plans each file,
 * removes the stuffing and runs the entropy stages once, then runs one IDCT + output pass per entry of outputs[0 .. n_outputs) over the
 * shared coefficients.  An output names a scale (1, 2, 4 or 8; each at most once), a form and per-file destinations:
 *   BBOCR_JPEG_FORM_YCBCR   what bbocr_jpeg_decode (scale 1) / bbocr_jpeg_decode_scaled (2, 4, 8) write for the file: YCbCr triples in
 *                           `layout` (BBOCR_PAGE_YCBCR3 or _YCBCR4) or a 1-component file's samples, ceil(height / scale) rows of
 *                           ceil(width / scale) pixels, rows pitches[k] bytes apart;
 *   BBOCR_JPEG_FORM_IMREAD  scale 1 only: bbocr_jpeg_imread's oriented BGR page and its pitch rule.
 * It takes every file bbocr_jpeg_decode takes (supported, or chroma != 0), at EVERY scale: a 4:4:4, 4:2:2 or 4:4:0 file at scale s > 1
 * comes out as libjpeg-turbo / Pillow's draft decode it -- every block through the n x n reduced IDCT, n = 8 / s (jdmaster.c doubles a
 * component's block only when both directions allow it), the chroma planes, ceil(OH / v) x ceil(OW / h) valid samples for luma sampling
 * (h, v), upsampled at the reduced size by h2v1_fancy_upsample / h1v2_fancy_upsample at s = 2 and 4 and by replication at s = 8
 * (jdsample.c turns fancy upsampling off when min_DCT_scaled_size is 1).  Each output equals what the single-purpose call writes for the
 * file, bit for bit.  status[k] (one per file, for all of its outputs): as bbocr_jpeg_decode's; a null destination or a short pitch in any
 * output refuses the file (BBOCR_ERR_ARG).  n_outputs outside 1 .. 4, a repeated scale, an unknown form, the imread form at scale > 1, a
 * null array: BBOCR_ERR_ARG before anything is queued.  Stream, one-batch-at-a-time contract and work buffers: bbocr_jpeg_decode's; the
 * component planes are sized per output, the coefficient buffer is shared by the outputs. */
enum { BBOCR_JPEG_FORM_YCBCR = 0, BBOCR_JPEG_FORM_IMREAD = 1 };
typedef struct bbocr_jpeg_output {
    int scale;                   /* 1, 2, 4 or 8 */
    int form;                    /* BBOCR_JPEG_FORM_* */
    uint8_t* const* dev_out;     /* [n] DEVICE destinations, one per file */
    const long long* pitches;    /* [n] bytes between rows */
} bbocr_jpeg_output;
int bbocr_jpeg_decode_scales(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, const bbocr_jpeg_output* outputs,
                             int n_outputs, int* status);
/* read-only totals of this context's JPEG lane since bbocr_create, per file of every batch: out[0] = files decoded, out[1] = runs of the
 * entropy stages, out[2] = IDCT passes, out[3] = output passes.  A two-output bbocr_jpeg_decode_scales call of one file adds 1, 1, 2, 2. */
int bbocr_jpeg_counters(bbocr_ctx* ctx, long long* out);
/* ---- progressive JPEG files (SOF2) decoded on the device (csrc/jpegprog.hip), opt-in beside everything above: bbocr_host_jpeg_plan keeps
 * refusing them (reason BBOCR_JPEG_SOF) and every call above keeps answering BBOCR_ERR_ARG for them.  A plan of their own describes the
 * scan script; bbocr_jpeg_decode_progressive takes the files it supports.  Taken: SOF2, 8 bit, Huffman, 1 component or 3 components under
 * bbocr_host_jpeg_plan's colour rule, sampled 4:2:0, 4:4:4, 4:2:2 or 4:4:0, at most BBOCR_JPEG_MAX_SCANS scans whose script is valid by
 * T.81 G.1.1 -- a DC scan has Ss = Se = 0 and may interleave, an AC scan holds one component with 1 <= Ss <= Se <= 63 behind that
 * component's first DC scan, a coefficient's first scan has Ah = 0, a refinement has Ah = the Al before it and Al = Ah - 1 -- and COMPLETE:
 * every coefficient 0 .. 63 of every component reaches Al = 0 (libjpeg-turbo smooths between the blocks of a file whose script is not,
 * so its pixels are not what the coefficients alone give).  Reasons: the ones above, where BBOCR_JPEG_SOF now means "not SOF2" -- a
 * baseline file is refused by THIS plan, it has bbocr_host_jpeg_plan -- and BBOCR_JPEG_MULTISCAN means a DQT behind the first SOS or a scan
 * header that names a component the frame does not have (or one twice, or out of frame order); BBOCR_JPEG_SCRIPT; BBOCR_JPEG_SCANS.
 * A non-interleaved scan walks its component's own block raster, ceil(ceil(width * h / hmax) / 8) blocks a row, and its restart
 * interval counts those blocks; an interleaved one counts MCUs. */
#define BBOCR_JPEG_MAX_SCANS 64
typedef struct bbocr_jpeg_scan {
    int components;              /* 1 .. 3 components in this scan; more than one: interleaved (DC scans only) */
    int component[3];            /* their indices in the frame, ascending */
    int dc_table[3], ac_table[3]; /* per scan component: the table ids (0 .. 3) its header names; the decoder keeps the tables' contents as they
                                  * stand at this SOS, since a DHT between scans may redefine an id */
    int ss, se, ah, al;
    int restart_interval;        /* in force at this SOS (a DRI may sit between scans): MCUs or blocks, 0 = none */
    int segments;                /* restart segments of this scan */
    long long offset;            /* first entropy-coded byte */
    long long bytes;             /* up to the marker that ends the scan (stuffing and restart markers included) */
} bbocr_jpeg_scan;
typedef struct bbocr_jpeg_progressive_plan {
    int width, height, components;
    int sampling[3][2];          /* (h, v) per component */
    int mcu_cols, mcu_rows;
    int chroma;                  /* 0: 4:2:0 or one component; BBOCR_JPEG_CHROMA_* otherwise */
    int orientation;             /* bbocr_jpeg_plan's rule */
    int supported;               /* 1: bbocr_jpeg_decode_progressive takes the file */
    int reason;                  /* BBOCR_JPEG_* */
    int n_scans;                 /* scans described below: all of a supported file's, those read before the refusal otherwise */
    int reserved;
    bbocr_jpeg_scan scans[BBOCR_JPEG_MAX_SCANS];
} bbocr_jpeg_progressive_plan;
/* host only, no GPU: one linear pass over the markers and the scans' FF bytes; no entropy bit is decoded */
int bbocr_host_jpeg_progressive_plan(const uint8_t* file, size_t bytes, bbocr_jpeg_progressive_plan* plan);
/* bbocr_jpeg_decode_scales -- same arguments, stream, one-batch-at-a-time contract, status codes and outputs -- that takes every file that
 * call takes AND the progressive files the plan above supports, so a mixed batch is one call.  A progressive file's scans run into the
 * zeroed coefficient buffer in file order wherever one builds on another: a scan waits for the earlier scans that hold one of its
 * components and overlap its band, the others of the whole batch share a set of launches (libjpeg's ten-scan script: three).  DC first
 * and AC first scans are cut into subsequences and decoded speculatively with self-synchronisation, like a baseline scan (an
 * end-of-band run counts its blocks at its symbol); a DC refinement is a parallel pass over its blocks; an AC refinement cannot be entered
 * in the middle and is decoded by one wavefront per (file, scan, restart segment), the corrections of a block applied by its lanes.  So a
 * batch fills the card, and one file without restart markers, a few serial wavefronts in its refinement scans, is slower than on the
 * host.  status[k] = BBOCR_ERR_DATA: in some scan a bit pattern without a code, a
 * refinement symbol of another size than 1, a segment that ends before or behind the blocks it promises, or an end-of-band run that
 * leaves it.  The IDCT and output stages are those of every other file. */
int bbocr_jpeg_decode_progressive(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout,
                                  const bbocr_jpeg_output* outputs, int n_outputs, int* status);
/* intermediates of ONE file that bbocr_jpeg_decode_progressive takes (parity tests), numbered like bbocr_op_jpeg_stage's: stage 1 = the
 * quantised coefficients after the first n_scans scans (0 = all; a baseline file has one), int16 [blocks][64] in natural order, blocks
 * in MCU order -- a block outside its component's raster holds what the interleaved scans gave it; 2 = the component planes; 3 = the pixels,
 * tight.  subseq_bits as there: it cuts the scan of a baseline file and the DC first and AC first scans of a progressive one. */
int bbocr_op_jpeg_progressive_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int n_scans, int subseq_bits, void* dev_dst,
                                    size_t dst_bytes, int* file_status);
/* host only: the planes of a decode at scale 2, 4 or 8 of a file the decoder takes (plan->supported or plan->chroma), per component
 * comps[0 .. components): the block's edge, the plane in whole MCUs as the device keeps it, the valid extent inside it (what libjpeg
 * calls downsampled_height x downsampled_width) and how the output stage brings the component to the output's size.  comps[components .. 3)
 * are zeroed.  Another scale, a refused plan: BBOCR_ERR_ARG.  These are the values the decoder itself runs on: the same table sizes its
 * planes and is what its IDCT and output stages read from their descriptors. */
enum {
    BBOCR_JPEG_UP_NONE = 0,            /* the plane has the output's sampling */
    BBOCR_JPEG_UP_H2V1_FANCY = 1,      /* 4:2:2 at scale 2 and 4: h2v1_fancy_upsample (h2v1_upsample when at most 2 samples wide) */
    BBOCR_JPEG_UP_H1V2_FANCY = 2,      /* 4:4:0 at scale 2 and 4: h1v2_fancy_upsample */
    BBOCR_JPEG_UP_H2V2_NOT_NEEDED = 3, /* 4:2:0 chroma: blocks of twice the edge, already the output's size */
    BBOCR_JPEG_UP_REPLICATE = 4        /* 4:2:2 and 4:4:0 at scale 8: out[x] = c[x / h], out[y] = c[y / v] */
};
typedef struct bbocr_jpeg_scaled_comp {
    int block;                   /* edge of one block's samples */
    int plane_rows, plane_cols;
    int valid_rows, valid_cols;
    int upsample;                /* BBOCR_JPEG_UP_* */
} bbocr_jpeg_scaled_comp;
int bbocr_host_jpeg_scaled_geometry(const bbocr_jpeg_plan* plan, int scale, bbocr_jpeg_scaled_comp* comps);
/* bbocr_op_jpeg_scaled_stage for ONE file of a chroma class (plan.chroma != 0; every other file: BBOCR_ERR_ARG): stage 2 = the component
 * planes in bbocr_host_jpeg_scaled_geometry's sizes, Y [mcu_rows * n * v][mcu_cols * n * h], then Cb, then Cr, each
 * [mcu_rows * n][mcu_cols * n], n = 8 / scale; 3 = the pixels, tight YCbCr triples. */
int bbocr_op_jpeg_scaled_class_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int scale, void* dev_dst, size_t dst_bytes,
                                     int* file_status);

/* ---- the extractor's model-input JPEG (enhanced_extractor.py:399-411, _encode_image_for_model's img.save(format="JPEG", quality=q)) written
 * on the device (csrc/jpegenc.hip): one u8 page in device memory -- any BBOCR_PAGE_* layout, rows `pitch` bytes apart, a crop of a larger
 * plane is a pointer + pitch -- becomes the file Pillow 12 / libjpeg-turbo saves for the page's RGB pixels (YCbCr pages: libjpeg's RGB),
 * byte for byte: baseline JFIF, SOF0, 8 bit, one interleaved scan, no restart interval, the standard Huffman tables,
 * jpeg_set_quality(quality, TRUE), ISLOW; components 3 = YCbCr 4:2:0 (a gray page: all-zero chroma blocks), components 1 = one component
 * (gray pages only, Pillow's "L" save).  The header -- SOI, APP0 JFIF 1.01 (units 0, density 1:1), COM when comment_bytes > 0, DQT per
 * table, SOF0, DHT per table, SOS -- and EOI are written on the host; only the bytes the scan produced cross the link.
 *
 * bbocr_jpeg_encode_bound: host only; a capacity that always suffices, 0 for H or W outside 1 .. 65535 or components not 1 or 3:
 *     66160 + 2 * ceil(blocks * (22 + 63 * 26) / 8) + 2,   blocks = 6 * ceil(H/16) * ceil(W/16)  (components 1: ceil(H/8) * ceil(W/8))
 * -- the longest header (a 65533-byte comment), a block of at most 22 bits for its DC term and 26 for each of its 63 AC terms, every scan
 * byte stuffed, EOI.
 * bbocr_host_jpeg_header: host only; everything up to and including SOS into out[capacity], *bytes = its length (also set when the
 * capacity is too small, which is BBOCR_ERR_ARG).
 * bbocr_jpeg_encode: the complete file into host_out[capacity], *bytes = its length.  A pipeline call: runs in a call slot next to
 * readtext calls, scratch from the slot, returns with its work finished.  BBOCR_ERR_ARG before anything is queued: a null pointer, H or
 * W outside 1 .. 65535, an unknown layout, a pitch shorter than a row, quality outside 1 .. 100, components not 1 or 3 or 1 with a
 * colour layout, a comment longer than 65533 bytes, a capacity below the bound. */
size_t bbocr_jpeg_encode_bound(int H, int W, int components);
int bbocr_host_jpeg_header(int H, int W, int components, int quality, const uint8_t* comment, int comment_bytes, uint8_t* out, size_t capacity,
                           size_t* bytes);
int bbocr_jpeg_encode(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int components, int quality,
                      const uint8_t* comment, int comment_bytes, uint8_t* host_out, size_t capacity, size_t* bytes);
/* its intermediates in DEVICE memory dev_dst[dst_bytes] (parity tests), *bytes = what was written: stage 0 = the quantised coefficients,
 * int16 [blocks][64] in zig-zag order, blocks in MCU order (Y00 Y01 Y10 Y11 Cb Cr; one component: raster order), dummy Y blocks as
 * libjpeg fills them; 1 = int64 [blocks + 1], every block's bit offset in the unstuffed scan, then the total; 2 = the unstuffed scan, its
 * last byte filled with 1-bits (dst_bytes >= ceil(blocks * (22 + 63 * 26) / 8)). */
int bbocr_op_jpeg_encode_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int components,
                               int quality, void* dev_dst, size_t dst_bytes, size_t* bytes);

/* ---- the trace previews' PNG file (enhanced_extractor.py:184-199, _image_to_data_url's img.save(format="PNG")) written on the device
 * (csrc/pngenc.hip): one u8 page in device memory -- BBOCR_PAGE_GRAY (colour type 0), BBOCR_PAGE_RGB or BBOCR_PAGE_BGR (colour type 2, BGR
 * swapped on read), rows `pitch` bytes apart -- becomes an 8-bit, non-interlaced PNG file.  The file is LOSSLESS but NOT the bytes Pillow
 * writes (zlib's serial match search cannot be reproduced faster on a GPU): opened with Pillow it has the mode (L or RGB), the size, the
 * pixels and the info["icc_profile"] of the file Pillow would have written.  The call is opt-in everywhere; its bytes are reproducible from
 * call to call and are defined by tests/png_ref.py:
 *   filter   per row the PNG filter (None, Sub, Up, Average, Paeth) with the smallest sum of |(int8) x|, ties to the lowest number;
 *   tokens   the filtered stream, H * (1 + W * channels) bytes, is cut into chunks of BBOCR_PNG_CHUNK bytes, each one deflate block of its
 *            own; a maximal run of L equal bytes inside a chunk is its first byte as a literal, then while R >= 3 (R = L - 1 at first) a
 *            match of min(R, 258) at distance 1, then the last 0 .. 2 bytes as literals;
 *   codes    per chunk a dynamic block: length-limited Huffman codes (15 bits; 7 for the code-length code) that are a pure integer
 *            function of the chunk's histogram, one distance code of length 1 when the chunk has matches;
 *   emit     header + tokens + end of block + an empty stored block (000, pad, 00 00 FF FF), so that every chunk's output is whole
 *            bytes; when that is not shorter than a stored block (5 + n bytes) the chunk is stored instead; no block is final;
 *   file     signature, IHDR, iCCP when icc_bytes > 0 (name "ICC Profile", the profile in stored deflate blocks), ONE IDAT (78 01, the
 *            chunks' blocks, the final empty block 03 00, Adler-32), IEND; CRC-32 and the framing on the host.
 *
 * bbocr_png_encode_bound: host only; a capacity that always suffices:
 *     59 + (icc_bytes ? 31 + icc_bytes + 5 * ceil(icc_bytes / 65535) : 0) + ceil(stream / 16384) * 5 + stream + 2 + 4,
 *     stream = H * (1 + W * channels)
 * -- signature, IHDR, IDAT's and IEND's framing and the zlib header; the iCCP chunk; every chunk stored; the final block; Adler-32.  0 for
 * H or W below 1, channels not 1 or 3, or a chunk whose payload would exceed 2^31 - 1 bytes.
 * bbocr_png_encode: the complete file into host_out[capacity], *bytes = its length.  A pipeline call: runs in a call slot next to readtext
 * calls, scratch from the slot, returns with its work finished.  BBOCR_ERR_ARG before anything is queued: a null pointer, a layout other
 * than the three above, a pitch shorter than a row, a page for which the bound is 0, a capacity below the bound.
 * bbocr_op_deflate: the tokens / codes / emit stages and the zlib framing (78 01 ... 03 00, Adler-32) of an arbitrary DEVICE byte stream
 * of n <= 2^31 - 1 bytes, into host_out[capacity >= 2 + ceil(n / 16384) * 5 + n + 6]; zlib's inflate reads it back.
 * bbocr_op_png_stage: intermediates in DEVICE memory dev_dst[dst_bytes] (parity tests), *bytes = what was written, by the functions the
 * full call runs.  Stage 0 = the filtered stream of the page (dev_src, H, W, pitch, layout; n is ignored).  Stages 1 .. 3 take dev_src as
 * a byte stream of n bytes (H, W, pitch, layout are ignored), chunks = ceil(n / 16384): 1 = uint32 [chunks][288], per chunk the counts of
 * the 286 literal/length symbols (end of block: 1), then the match count, then the token count; 2 = uint8 [chunks][320], per chunk the
 * block kind (0 stored, 1 dynamic), flags (bit 0: a literal/length code was deeper than 15 bits before the limiter, bit 1: a code-length
 * code deeper than 7), the 286 literal/length code lengths, the distance code's length, the 19 lengths of the code-length code in symbol
 * order, zeros; 3 = int64 [chunks + 1], the byte offsets of the chunks' blocks in the compacted buffer, then its length. */
#define BBOCR_PNG_CHUNK 16384
size_t bbocr_png_encode_bound(int H, int W, int channels, size_t icc_bytes);
int bbocr_png_encode(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, const uint8_t* icc, size_t icc_bytes,
                     uint8_t* host_out, size_t capacity, size_t* bytes);
int bbocr_op_deflate(bbocr_ctx* ctx, const uint8_t* dev_bytes, size_t n, uint8_t* host_out, size_t capacity, size_t* bytes);
int bbocr_op_png_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, size_t n, void* dev_dst,
                       size_t dst_bytes, size_t* bytes);

/* ---- PNG files decoded on the device (csrc/pngdec.hip; opt-in: Reader(png_decode=True)): what reader.decode_file holds for a PNG file
 * -- Pillow's convert("RGB") and the gray plane of its stated rule -- from the file's bytes, of which only the IDAT payloads cross the link.
 * Scope: non-interlaced files of colour type 0 at depth 1 / 2 / 4 / 8, colour type 3 at depth 1 / 2 / 4 / 8 with PLTE, colour types 2, 4
 * and 6 at depth 8.  tRNS and every other ancillary chunk are skipped (convert("RGB") ignores them).  Defined by tests/png_decode_ref.py.
 * bbocr_host_png_plan: host only, no GPU: one pass over the chunks.  Fields the walk did not reach stay 0; the IHDR fields of a file that
 * is refused behind its IHDR are filled. */
enum {
    BBOCR_PNG_OK = 0,
    BBOCR_PNG_NOT_PNG = 1,      /* no signature */
    BBOCR_PNG_TRUNCATED = 2,    /* a chunk runs past the end of the file, or the file ends before IEND */
    BBOCR_PNG_CRC = 3,          /* CRC-32 mismatch of any chunk up to IEND -- IHDR, PLTE, IDAT, IEND and the ancillary ones: Pillow refuses such a file */
    BBOCR_PNG_DIMENSIONS = 4,   /* width or height 0, the filtered stream H * (1 + row_bytes) above 2^31 - 1 bytes, or more than 178,956,970
                                 * pixels (twice Pillow's MAX_IMAGE_PIXELS, where its decode raises) */
    BBOCR_PNG_DEPTH = 5,        /* 16-bit samples, or a depth the colour type does not allow */
    BBOCR_PNG_INTERLACE = 6,    /* Adam7 */
    BBOCR_PNG_PALETTE = 7,      /* colour type 3 without PLTE, PLTE behind IDAT, a second PLTE, a PLTE of 0, more than 256 or not whole entries */
    BBOCR_PNG_IDAT_ORDER = 8,   /* IDAT chunks that are not consecutive */
    BBOCR_PNG_APNG = 9,         /* an acTL chunk */
    BBOCR_PNG_ZLIB = 10,        /* the zlib header: method other than 8, window above 32 KiB, FDICT set, failing FCHECK, fewer than 2 bytes */
    BBOCR_PNG_HEADER = 11       /* the first chunk is not a 13-byte IHDR, an unknown colour type, compression, filter or interlace method, no IDAT */
};
typedef struct bbocr_png_plan {
    int width, height, bit_depth, color_type;
    int channels;               /* samples per pixel of the filtered scanline: 1, 2, 3 or 4 (a palette index counts as one) */
    int bpp;                    /* the filters' byte distance: channels at depth 8, 1 below */
    long long row_bytes;        /* of a filtered scanline without its filter byte: ceil(width * channels * bit_depth / 8) */
    int palette_entries;        /* of PLTE (any colour type), 0 without one */
    int idat_chunks;
    long long idat_bytes;       /* the IDAT payloads together: the zlib stream */
    int supported;              /* 1: bbocr_png_decode takes the file */
    int reason;                 /* BBOCR_PNG_* */
    int reserved[2];
} bbocr_png_plan;
int bbocr_host_png_plan(const void* file, size_t bytes, bbocr_png_plan* plan);
/* n files (HOST bytes) -> both planes in DEVICE memory, one call per batch: dst_rgb[k] receives uint8 [H,W,3], rows pitch_rgb[k] bytes
 * apart, dst_gray[k] uint8 [H,W], rows pitch_gray[k] bytes apart -- one shape per file, so that the call serves a uniform batch and pages
 * of mixed shapes alike.  RGB: Pillow's convert("RGB") (a gray sample replicated, depths 1 / 2 / 4 scaled by 255 / 85 / 17; alpha dropped;
 * the palette looked up).  Gray: the stored (scaled) sample for colour types 0 and 4, else (9797 R + 19234 G + 3737 B) >> 15.
 * status[k]: 0, BBOCR_ERR_ARG (a null pointer, a pitch shorter than a row, a file the plan refuses) or BBOCR_ERR_DATA: the zlib stream is
 * damaged (the input runs out, block type 3, LEN != ~NLEN, an over-subscribed or incomplete code -- a single code of one bit excepted, as
 * in zlib --, a bit pattern without a code, a distance beyond the bytes produced, more or fewer bytes than H * (1 + row_bytes), another
 * Adler-32 than the trailer's), a filter byte is above 4, or a palette index is at or above palette_entries.  Such a file's destinations
 * are undefined; no byte outside a destination's rows is ever written, the other files decode all the same and the context stays usable.
 * Stream, one-batch-at-a-time contract and work buffers: bbocr_jpeg_decode's.  Returns with its work finished, also when it fails.
 * bbocr_op_png_decode_stage: the intermediates of ONE file in DEVICE memory dev_dst[dst_bytes] (parity tests), by the kernels the full call
 * runs: stage 0 = the inflated stream, H * (1 + row_bytes) bytes (only the inflate stage runs); 1 = the same after the filters are
 * reversed; 2 = RGB [H,W,3] followed by gray [H,W], tight.  *file_status as status[k] above, of the stages that ran. */
int bbocr_png_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status);
int bbocr_op_png_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status);

/* ---- TIFF files decoded on the device (csrc/tiffdec.hip; opt-in: Reader(tiff_decode=True)): what reader.decode_file holds for a TIFF file
 * -- Pillow's convert("RGB") of frame 0 and the gray plane of its stated rule -- from the file's bytes, of which only the strips cross the
 * link.  Scope: classic TIFF (II or MM), strips, chunky samples, fill order 1, unsigned samples; compression 1 (none), 32773 (PackBits),
 * 5 (LZW, MSB-first codes with the early change) and 8 / 32946 (one zlib stream per strip); predictor 1, or 2 on 8-bit samples under LZW
 * or Deflate (libtiff applies the tag to those codecs only); photometric 0 / 1 with one sample of 1 or 8 bits, 2 with 8,8,8 or with
 * 8,8,8,8 and ExtraSamples 0 or 2 (the fourth sample dropped), 3 with one 8-bit sample and a ColorMap of 3 x 256 SHORTs, of which a colour
 * is the HIGH byte (value >> 8: Pillow's rule).  The Orientation tag is not applied (decode_file does not).  Defined by
 * tests/tiff_decode_ref.py.
 * bbocr_host_tiff_plan: host only, no GPU: one walk over the header and the first IFD.  Fields the walk did not reach stay 0. */
enum {
    BBOCR_TIFF_OK = 0,
    BBOCR_TIFF_NOT_TIFF = 1,     /* fewer than 8 bytes, no II / MM mark, a magic other than 42 or 43 */
    BBOCR_TIFF_BIGTIFF = 2,      /* magic 43 */
    BBOCR_TIFF_TRUNCATED = 3,    /* the IFD, a value or a strip runs past the end of the file */
    BBOCR_TIFF_HEADER = 4,       /* a required tag is missing, has no value or a type other than BYTE / SHORT / LONG; BitsPerSample does not
                                  * hold SamplesPerPixel values */
    BBOCR_TIFF_DIMENSIONS = 5,   /* width or height 0 or above 2^31 - 1, more than 178,956,970 pixels (bbocr_host_png_plan's limit), or a
                                  * decoded stream height * row_bytes above 2^31 - 1 bytes */
    BBOCR_TIFF_TILES = 6,        /* any of the tile tags 322 .. 325 */
    BBOCR_TIFF_PLANAR = 7,       /* PlanarConfiguration other than 1 */
    BBOCR_TIFF_FILL_ORDER = 8,   /* FillOrder other than 1 */
    BBOCR_TIFF_DEPTH = 9,        /* 16-bit or wider samples, a SampleFormat other than unsigned integer, samples of unequal or odd depth,
                                  * 1-bit samples under photometric 2 or 3 */
    BBOCR_TIFF_SUBBYTE = 10,     /* 2- or 4-bit samples */
    BBOCR_TIFF_GRAY_ALPHA = 11,  /* photometric 0 / 1 with two samples */
    BBOCR_TIFF_ASSOC_ALPHA = 12, /* ExtraSamples 1: premultiplied alpha */
    BBOCR_TIFF_PHOTOMETRIC = 13, /* CMYK, YCbCr, CIELab and every other interpretation above 3 */
    BBOCR_TIFF_SAMPLES = 14,     /* a sample count the interpretation does not allow; four samples without one ExtraSamples value of 0 or 2 */
    BBOCR_TIFF_JPEG = 15,        /* compression 6 or 7 */
    BBOCR_TIFF_CCITT = 16,       /* compression 2, 3 or 4 */
    BBOCR_TIFF_COMPRESSION = 17, /* any other compression */
    BBOCR_TIFF_PREDICTOR = 18,   /* predictor 3 or unknown; predictor 2 on 1-bit samples or under a codec for which libtiff ignores the tag */
    BBOCR_TIFF_OLD_LZW = 19,     /* old-style LZW: the first strip starts 00 followed by an odd byte (libtiff's test) */
    BBOCR_TIFF_STRIPS = 20,      /* no strip table, RowsPerStrip 0, or tables whose length is not ceil(height / rows_per_strip) */
    BBOCR_TIFF_PALETTE = 21      /* photometric 3 without a ColorMap of 3 x 256 SHORTs */
};
typedef struct bbocr_tiff_plan {
    int width, height, bits, samples, photometric, compression, predictor;
    int big_endian;             /* the byte order: 0 "II", 1 "MM" */
    long long rows_per_strip;   /* as used: min(RowsPerStrip, height); the tag absent counts as 2^32 - 1 */
    int strips;                 /* ceil(height / rows_per_strip) */
    int extra_sample;           /* the ExtraSamples value of a four-sample file, else -1 */
    long long row_bytes;        /* ceil(width * samples * bits / 8) */
    long long strip_bytes;      /* the strips' stored bytes together: what crosses the link */
    int supported;              /* 1: bbocr_tiff_decode takes the file */
    int reason;                 /* BBOCR_TIFF_* */
    int reserved[2];
} bbocr_tiff_plan;
int bbocr_host_tiff_plan(const void* file, size_t bytes, bbocr_tiff_plan* plan);
/* n files (HOST bytes) -> both planes in DEVICE memory, one call per batch whatever mix of codecs and shapes it holds: dst_rgb[k] receives
 * uint8 [H,W,3], rows pitch_rgb[k] bytes apart, dst_gray[k] uint8 [H,W], rows pitch_gray[k] bytes apart -- one shape per file.  RGB:
 * Pillow's convert("RGB") (a gray sample replicated, 1-bit samples 0 / 255, photometric 0 inverted, the palette looked up, a fourth sample
 * dropped).  Gray: the stored (inverted) sample for photometric 0 / 1, else (9797 R + 19234 G + 3737 B) >> 15.
 * status[k]: 0, BBOCR_ERR_ARG (a null pointer, a pitch shorter than a row, a file the plan refuses) or BBOCR_ERR_DATA: a strip is damaged
 * -- it runs out of input before it has produced rows_in_strip * row_bytes bytes, a run or a string would write beyond that count, an LZW
 * strip does not begin with a Clear code, uses a code above the next free entry or follows a Clear with a code that is no literal, a
 * Deflate strip fails one of bbocr_png_decode's checks (zlib header, stream, Adler-32).  Such a file's destinations are undefined; no byte
 * outside a destination's rows is ever written, the other files decode all the same and the context stays usable.  Stream,
 * one-batch-at-a-time contract and work buffers: bbocr_jpeg_decode's.  Returns with its work finished, also when it fails.
 * bbocr_op_tiff_decode_stage: the intermediates of ONE file in DEVICE memory dev_dst[dst_bytes] (parity tests), by the kernels the full
 * call runs: stage 0 = the strips' decoded stream, height * row_bytes bytes (only the strip launch runs); 1 = the same after the predictor;
 * 2 = RGB [H,W,3] followed by gray [H,W], tight.  *file_status as status[k] above, of the stages that ran. */
int bbocr_tiff_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                      uint8_t* const* dst_gray, const long long* pitch_gray, int* status);
int bbocr_op_tiff_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status);

/* ---- CCITT TIFF files decoded on the device (csrc/tiff_fax.h, the codec TD_FAX of csrc/tiffdec.hip; opt-in on top of the TIFF decoder:
 * Reader(tiff_decode="fax")): what document scanners and fax gateways write for a bitonal page.  Scope: compression 2 (modified Huffman:
 * rows start on a byte boundary, no EOL), 3 (T.4: 1-D, or 2-D with T4Options bit 0; with or without the byte-aligned EOLs of bit 2) and
 * 4 (T.6); one 1-bit sample, photometric 0 or 1, either byte order, any RowsPerStrip, FillOrder 1 or 2 (with 2 the bits of every stored
 * byte are reversed on read).  A white run decodes to 0 bits and a black run to 1 bits; the output pass applies the photometric tag as it
 * does for any 1-bit file.  The reference line of a strip's first row is white.  Accepted: any number of make-up codes before a
 * terminating code, a zero-length white run at the start of a row, any number of 0 fill bits before an EOL, a leading EOL; bytes behind
 * the strip's last row (RTC, EOFB) are not read.  STRICTER than libtiff, which patches a bad line and carries on: a strip is decoded
 * exactly or the file gets BBOCR_ERR_DATA (and its caller takes the host decode) -- a bit pattern that is no code, an extension
 * (uncompressed mode) code, a row whose runs do not end exactly at the width, a vertical mode that does not move a0 forwards or moves it
 * past the width, a pass mode whose b2 is the end of the line, a T.4 row without its EOL or tag bit, input that ends early.  Defined by
 * tests/tiff_fax_ref.py.
 * The widest row the decoder's line buffers hold (two lists of changing elements and the row's bitmap in LDS, 42,272 bytes at the limit;
 * A3 at 600 dpi is 7016 pixels wide): */
#define BBOCR_FAX_MAX_WIDTH 10240
enum {
    BBOCR_FAX_OK = 0,           /* the plain plan or the fax plan takes the file */
    BBOCR_FAX_PLAIN = 1,        /* the walk refuses the file for something other than CCITT or fill order: plan.reason says what (a
                                 * photometric above 1 is among these: the walk refuses it on one 1-bit sample, DEPTH or PHOTOMETRIC) */
    BBOCR_FAX_FILL_ORDER = 2,   /* a FillOrder other than 1 or 2, or FillOrder 2 on a file that is not CCITT */
    BBOCR_FAX_DEPTH = 3,        /* BitsPerSample or SamplesPerPixel other than 1 */
    BBOCR_FAX_OPTIONS = 4,      /* the uncompressed-mode bit or an unknown bit of T4Options (292) / T6Options (293), or a malformed tag */
    BBOCR_FAX_WIDTH = 5         /* wider than BBOCR_FAX_MAX_WIDTH */
};
typedef struct bbocr_tiff_fax {
    int scheme;                 /* 0: no CCITT file; else the compression, 2, 3 or 4 */
    int t4_options;             /* tag 292 of a compression-3 file, tag 293 of a compression-4 file; 0 when absent */
    int fill_order;             /* FillOrder as stored (1 when absent or not reached) */
    int reason;                 /* BBOCR_FAX_* */
    int reserved[4];
} bbocr_tiff_fax;
/* bbocr_host_tiff_fax_plan: host only, no GPU: bbocr_host_tiff_plan's walk in the mode that goes on behind a CCITT compression and a fill
 * order other than 1 and finishes its remaining checks, then the checks above in the order of the enum.  plan: as bbocr_host_tiff_plan fills
 * it for a supported file (supported 1, reason 0) when either plan takes the file; when the walk refuses the file for another reason, as
 * it left it (fax->reason BBOCR_FAX_PLAIN); when the fax checks refuse it, every field filled, supported 0 and reason BBOCR_TIFF_CCITT
 * or BBOCR_TIFF_FILL_ORDER.  bbocr_host_tiff_plan itself answers as before for every file.
 * bbocr_tiff_decode_fax / bbocr_op_tiff_fax_decode_stage: the contracts of bbocr_tiff_decode / bbocr_op_tiff_decode_stage with the files
 * admitted by bbocr_host_tiff_fax_plan, so a batch may mix CCITT files with raw, PackBits, LZW and Deflate ones; still three launches, the
 * CCITT strips one wavefront each in the strip launch.  bbocr_tiff_decode and bbocr_op_tiff_decode_stage keep refusing a CCITT file. */
int bbocr_host_tiff_fax_plan(const void* file, size_t bytes, bbocr_tiff_plan* plan, bbocr_tiff_fax* fax);
int bbocr_tiff_decode_fax(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                          uint8_t* const* dst_gray, const long long* pitch_gray, int* status);
int bbocr_op_tiff_fax_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status);

/* ---- GIF files decoded on the device (csrc/gifdec.hip; opt-in: Reader(gif_decode=True)): what reader.decode_file holds for a GIF file
 * -- Pillow's convert("RGB") of frame 0 and the gray plane of its stated rule -- from the file's bytes, of which only the de-framed LZW
 * payload and the colour table cross the link.  The code stream is split at its clear codes: the width of a GIF code depends only on the
 * count of codes since the last clear, so the position of every code behind a clear is a closed form, a wavefront finds the next clear 64
 * codes at a time, and every piece between two clears is decoded by a wavefront of its own (csrc/gif_lzw.h).  Defined by
 * tests/gif_decode_ref.py, which also lists Pillow's rules as restated and the classes that are stricter than Pillow.
 * bbocr_host_gif_plan: host only, no GPU: the signature, the screen descriptor, the global table, the extensions up to the first image
 * descriptor (a graphic control extension's transparency index is read, every other extension skipped), the descriptor, the local table,
 * the minimum code size and the data sub-blocks.  Later frames are not read.  Fields the walk did not reach stay 0 (transparency: -1). */
enum {
    BBOCR_GIF_OK = 0,
    BBOCR_GIF_NOT_GIF = 1,      /* no "GIF87a" / "GIF89a" signature */
    BBOCR_GIF_TRUNCATED = 2,    /* the file ends inside the structure, the data sub-blocks have no terminator, a block introducer before the
                                 * image is none of 21 / 2C / 3B, or a graphic control block is shorter than four bytes */
    BBOCR_GIF_NO_IMAGE = 3,     /* the trailer comes before any image descriptor */
    BBOCR_GIF_EMPTY = 4,        /* a frame of width or height 0 */
    BBOCR_GIF_PIXELS = 5,       /* a canvas of more than 178,956,970 pixels (bbocr_host_png_plan's limit) */
    BBOCR_GIF_CODE_SIZE = 6     /* a minimum code size outside 2 .. 8 */
};
typedef struct bbocr_gif_plan {
    int screen_w, screen_h;
    int x0, y0, width, height;  /* the frame rectangle */
    int canvas_w, canvas_h;     /* Pillow's image size: max(screen, x0 + width) by max(screen, y0 + height) */
    int interlace;
    int table_len;              /* entries of the table in force -- the local one over the global one --, 0: the file has none */
    int local_table;            /* 1: the table in force is the local one */
    int transparency;           /* the index pixels outside the frame hold, or -1 (they hold 0) */
    int min_code;
    int mode_l;                 /* 1: Pillow's mode L (every entry i of the table in force is (i, i, i), or no table): gray = the index */
    long long payload_bytes;    /* the data sub-blocks together: what crosses the link */
    int supported;              /* 1: bbocr_gif_decode takes the file */
    int reason;                 /* BBOCR_GIF_* */
    int reserved[2];
    uint8_t table[768];         /* the RGB plane's lookup, R G B per index: the table in force, black where it has no entry; mode L: the
                                 * ramp, or the global table behind a local ramp (Pillow's reading) */
} bbocr_gif_plan;
int bbocr_host_gif_plan(const void* file, size_t bytes, bbocr_gif_plan* plan);
/* n files (HOST bytes) -> both planes [canvas_h, canvas_w] in DEVICE memory, one call per batch whatever mix of shapes, piece counts and
 * code sizes it holds; destinations as bbocr_tiff_decode's.  Five launches: the scan (one wavefront per file: the piece table -- first
 * bit, data codes, how the piece ends), the lengths (one wavefront per piece: its decoded byte count and validity), the offsets (an
 * exclusive prefix sum per file, saturated at width * height, and the file's status), the decode (one wavefront per piece: match copies
 * into the file's index stream at the piece's offset, clipped at width * height) and the output (de-interlace, placement on the canvas,
 * table lookup, both planes).  No launch waits on another workgroup.
 * status[k]: 0, BBOCR_ERR_ARG (a null pointer, a pitch shorter than a row, a file the plan refuses, a payload of 2^28 bytes or more) or
 * BBOCR_ERR_DATA: before width * height indices exist, the first code behind a clear is no literal, a code lies above the next free
 * entry, the end code or the payload's end is met, or the stream has more pieces than the piece table holds (min(payload_bits /
 * (min_code + 1) + 1, max(4096, payload_bytes / 16))).  What follows the full frame is ignored.  Such a file's destinations are
 * undefined; no byte outside a destination's rows is ever written, the other files decode all the same and the context stays usable.
 * Stream, one-batch-at-a-time contract and work buffers: bbocr_jpeg_decode's.  Returns with its work finished, also when it fails.
 * bbocr_op_gif_decode_stage: the intermediates of ONE file in DEVICE memory dev_dst[dst_bytes] (parity tests), by the kernels the full
 * call runs: stage 0 = the piece table: uint32 count, scan error bits, 0, 0, then per piece uint32 first bit (low, high), data codes, end
 * (0 clear, 1 end code, 2 end of payload) -- dst_bytes at least 16 + 16 * the table's room; 1 = uint32 offsets[count] and the total;
 * 2 = the index stream in stored row order, width * height bytes.  *file_status as status[k] above, of the launches that ran. */
int bbocr_gif_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status);
int bbocr_op_gif_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status);
/* Measurement and test helpers, no part of the decode interface.  bbocr_gif_decode_timed: bbocr_gif_decode, and launch_ms[5] (may be
 * null) = the five launches' times in milliseconds, between events on the stream (tools/bench_gif_bmp_decode.py).
 * bbocr_gif_piece_room: the piece table's room for a payload, by which a caller of bbocr_op_gif_decode_stage sizes its destination. */
int bbocr_gif_decode_timed(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                           uint8_t* const* dst_gray, const long long* pitch_gray, int* status, float* launch_ms);
size_t bbocr_gif_piece_room(long long payload_bytes, int min_code);

/* ---- BMP files decoded on the device (csrc/bmpdec.hip; opt-in: Reader(bmp_decode=True)): what reader.decode_file holds for a BMP file
 * -- Pillow's convert("RGB") and the gray plane of its stated rule -- from the file's bytes, which cross the link whole.  Pillow's
 * BmpImagePlugin._bitmap restated: headers of 12, 40, 52, 56, 64, 108 and 124 bytes; bottom-up, or top-down when the height's top byte is
 * FF; rows ((width * bits + 31) >> 3) & ~3 bytes apart; 1, 4 and 8 bits with a table of B G R entries (3 bytes behind a 12-byte header,
 * else 4) -- mode 1 when it is exactly black then white, L when an 8-bit file's table is the ramp, P otherwise, an index without an entry
 * black --; 16 bits 5-5-5 uncompressed or bit fields 5-6-5 / 5-5-5, a channel v expanded as v * 255 / 31 (63) in integers; 24 bits; 32
 * bits B G R X uncompressed and the eight mask layouts Pillow lists, alpha dropped.  Defined by tests/bmp_decode_ref.py.
 * bbocr_host_bmp_plan: host only, no GPU.  Fields the walk did not reach stay 0. */
enum {
    BBOCR_BMP_OK = 0,
    BBOCR_BMP_NOT_BMP = 1,      /* no "BM" */
    BBOCR_BMP_TRUNCATED = 2,    /* the file ends inside the headers, the masks behind a 40-byte header or the table, or is shorter than
                                 * data_offset + row_stride * height (Pillow raises when a whole row is missing and reads on when less is) */
    BBOCR_BMP_HEADER = 3,       /* a header size other than 12, 40, 52, 56, 64, 108, 124 */
    BBOCR_BMP_DIMENSIONS = 4,   /* width 0 or above 2^31 - 1 (a negative width), height 0 */
    BBOCR_BMP_PIXELS = 5,       /* more than 178,956,970 pixels (bbocr_host_png_plan's limit) */
    BBOCR_BMP_DEPTH = 6,        /* a depth other than 1, 4, 8, 16, 24, 32 */
    BBOCR_BMP_RLE = 7,          /* RLE8, RLE4 */
    BBOCR_BMP_COMPRESSION = 8,  /* JPEG, PNG and every other compression above 3 */
    BBOCR_BMP_MASKS = 9,        /* bit fields in a layout Pillow does not list, or on a file of 8 bits or fewer */
    BBOCR_BMP_PALETTE = 10,     /* a table of more than 65,536 entries, or of more than 256 that is no gray ramp: Pillow opens such a file and
                                 * raises "invalid palette size" when it loads it */
    BBOCR_BMP_GRAY_TABLE = 11   /* a table that makes Pillow's mode 1 or L on samples of another depth -- a gray ramp on 1 or 4 bits, black then
                                 * white on 4 or 8 bits: Pillow raises or reads the rows at the wrong depth */
};
typedef struct bbocr_bmp_plan {
    int width, height, bits, compression, header_size;
    int top_down;
    int colors;                 /* entries of the table (1, 4, 8 bits), else 0 */
    int mode;                   /* 0 P, 1 Pillow's mode 1, 2 L, 3 direct colour */
    int r_at, g_at, b_at;       /* 24 and 32 bits: the byte of a pixel that holds R, G, B */
    int six_bit_green;          /* 16 bits: 1 for 5-6-5 */
    long long table_offset;     /* the table's place in the file */
    int table_entry;            /* 3 or 4 bytes */
    int supported;              /* 1: bbocr_bmp_decode takes the file */
    long long row_stride, data_offset;
    int reason;                 /* BBOCR_BMP_* */
    int reserved[3];
} bbocr_bmp_plan;
int bbocr_host_bmp_plan(const void* file, size_t bytes, bbocr_bmp_plan* plan);
/* n files (HOST bytes) -> both planes [height, width] in DEVICE memory by ONE launch, whatever mix of shapes and depths; destinations as
 * bbocr_tiff_decode's.  A workgroup runs over a row, its lanes over the row's pixels: they unpack bits, nibbles, bytes, 16-bit words or 3- and 4-byte groups, flip the row
 * order and write both planes.  status[k]: 0 or BBOCR_ERR_ARG (a null pointer, a pitch shorter than a row, a file the plan refuses):
 * every byte the launch reads lies inside the file, as the plan has checked.  Stream, one-batch-at-a-time contract and work buffers:
 * bbocr_jpeg_decode's.  Returns with its work finished, also when it fails. */
int bbocr_bmp_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status);

#ifdef __cplusplus
}
#endif
#endif
