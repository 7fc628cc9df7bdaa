// Internal header of libbbocr: context, small host helpers and the functions the translation units share.
// Translation units: weights.cpp (BN folding, MFMA packing), detector.cpp (CRAFT forward, box extraction), recognizer.cpp (crops,
// CRNN, CTC), preprocess.cpp (the f2 chain), abi.cpp (context + pipeline entry points of include/bbocr.h), pages.cpp (the pipeline call
// for pages of mixed shapes, its plan and page tables), abi_ops.cpp (stage-level
// entry points used by the parity tests).
#pragma once
#include "../../include/bbocr.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "boxpost.h"
#include "hostpool.h"
#include "common.h"
#include "kernels.h"
#include "word_dict.h"


using clk = std::chrono::steady_clock;
static inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

struct StatusError {
    int code;
    std::string msg;
};
[[noreturn]] inline void fail(int code, const std::string& m) { throw StatusError{code, m}; }
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) fail(BBOCR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

struct DevBuf {   // growable device buffer, freed with its owner (the context)
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        HIPCHK(hipMalloc(&p, n));
        cap = n;
    }
    void ensure_keep(size_t n, size_t used) {   // grow, keeping the first `used` bytes (waits for the device: the old buffer may be in use)
        if (n <= cap) return;
        void* q = nullptr;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMalloc(&q, n));
        if (p && used) HIPCHK(hipMemcpy(q, p, std::min(used, cap), hipMemcpyDeviceToDevice));
        if (p) (void)hipFree(p);
        p = q;
        cap = n;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct PinBuf {   // growable pinned host buffer: the source of truly asynchronous H2D copies (a pageable source makes hipMemcpyAsync wait
                  // for the stream first, which stalls the host exactly where it should be queueing work behind a running kernel)
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) { HIPCHK(hipDeviceSynchronize()); (void)hipHostFree(p); }     // a queued copy may still read the old buffer
        p = nullptr;
        cap = 0;
        HIPCHK(hipHostMalloc(&p, n, hipHostMallocDefault));
        cap = n;
    }
};

struct Arena {   // bump allocator over one device buffer; a dry pass sizes it, the real pass carves it
    DevBuf buf;
    size_t off = 0;
    bool dry = true;
    void begin(bool d) { off = 0; dry = d; }
    template <typename T> T* alloc(size_t count) {
        off = align_up(off, 256);
        T* r = dry ? nullptr : (T*)((char*)buf.p + off);
        off += count * sizeof(T);
        return r;
    }
};

struct Carve {   // offsets into one buffer at 256-byte steps: add() while the buffer is sized, at<T>() once it exists
    size_t off = 0;
    size_t add(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
    template <typename T> static T* at(void* base, size_t o) { return (T*)((char*)base + o); }
};

struct Act {   // bf16 NHWC activation
    uint16_t* p;
    int N, H, W, C;
};

// A page in device memory as the page-level entry points take it: H rows of W packed pixels of a PAGE_* layout, `pitch` bytes apart.
struct DevPage {
    const void* p;
    int H, W;
    long long pitch;
    int layout;
};
constexpr unsigned page_set(int layout) { return 1u << layout; }
constexpr unsigned PAGE_ANY = page_set(PAGE_YCC3 + 1) - 1;
// the one rule of a valid page; `allowed`: page_set() bits of the layouts the caller takes
inline void check_page(const DevPage& g, unsigned allowed = PAGE_ANY) {
    if (!g.p) fail(BBOCR_ERR_ARG, "null device pointer");
    if (g.H < 1 || g.W < 1) fail(BBOCR_ERR_ARG, "bad image shape");
    if ((long long)g.H * g.W >= (1LL << 30)) fail(BBOCR_ERR_ARG, "image too large");
    if (g.layout < PAGE_GRAY || g.layout > PAGE_YCC3 || !(allowed & page_set(g.layout))) fail(BBOCR_ERR_ARG, "layout must be one of the BBOCR_PAGE_* taken here");
    if (g.pitch < (long long)g.W * page_px_bytes(g.layout)) fail(BBOCR_ERR_ARG, "row pitch smaller than a row");
}

// A mutex plus a lazily created non-blocking stream on the root, outside the call slots: work on a lane never waits for a running call
// (lane_guarded below).  One call at a time per lane.
struct SideLane {
    std::mutex mu;
    hipStream_t stream = nullptr;
};



// Everything bbocr_load_weights leaves on the device, as the kernels read it.  A context's extra CALL SLOTS (below) hold a copy of this
// view -- pointers into the root context's blocks, which alone owns (and frees) them.
struct WeightView {
    // ---- detector
    bool craft_loaded = false;
    uint16_t* c11_wf = nullptr;               // conv1_1 weights in the layout of the producer fused into conv1_2
    float* c11_b = nullptr;
    float* c11_w32 = nullptr;                 // exact mode: conv1_1 folded fp32 [64][3][3][3] (craft_pair.hip::pair_conv1_1_kernel)
    float* cls6_w32 = nullptr;                // exact mode: conv_cls.6.weight fp32 [16][16] (pair_cls_tail_kernel)
    ConvPlan conv1_2, conv2_1, conv2_2, conv3_1, conv3_2, conv3_3, conv4_1, conv4_2, conv4_3, conv5_1, conv5_2, fc6, fc7;
    ConvPlan up1a, up1b, up2b, up3b, up4b, cls0, cls2, cls4;
    // fast modes: fc6, fc7 and the fc7 half of upconv1's 1x1 folded into ONE dilated 3x3 512 -> 512 (no bias), and the skip half of that 1x1 with
    // the composite bias, whose epilogue adds fcfold's output (fc_fold.h, weights.cpp::load_fc_fold); fc7 is an exact-mode plan only, fc6 is
    // still uploaded in the fast modes though nothing launches it (the blob-size pin, see load_fc_fold), up1a (the 1x1 over the whole
    // concat) stays loaded for its stage entry point
    ConvPlan fcfold, up1s;
    // U-net 1x1 layers over cat[up(y), skip], split by linearity: upNy = the columns of y (no bias, run at y's resolution),
    // upNs = the columns of the skip tensor (+ bias), whose epilogue adds the 2x bilinear up-sampling of upNy's output
    ConvPlan up2y, up2s, up3y, up3s, up4y, up4s;
    float* cls_tail = nullptr;   // b1[16] w2[32] b2[2]
    uint16_t* cls_tail_frag = nullptr;   // conv_cls.6 weight as an MFMA A fragment
    uint16_t* up4y_post = nullptr;       // upconv4's 1x1, y half (64 -> 64), as the A fragments of the 1x1 applied in upconv3.3x3's epilogue
    // ---- recogniser
    bool crnn_loaded = false;
    float* r0_wb = nullptr;      // w[9][32] (tap-major) b[32]
    uint16_t* r0_afrag = nullptr;  // taps 0..7 three-way split into element-type terms, as MFMA A fragments (crnn_conv0_mfma_kernel)
    ConvPlan r1, r2, r3, r4, r5, r6, xproj[2], lin[2], pred;
    uint16_t* pred_wide = nullptr;   // more than 128 classes, 16-bit modes: Prediction.weight as pred_ctc_kernel's A fragments (pack_pred_ctc_weights)
    float* pred_wide_b = nullptr;    // and its bias, padded to whole 16-class fragments
    uint16_t* whh[2] = {nullptr, nullptr};
    float whh_scale[2] = {1.f, 1.f};   // exact mode: 2^-s of the packed W_hh (pack_lstm_whh_split)
    // rec_quant (bbocr_config::rec_quant): the eleven tensors of the sequence half as symmetric qint8, packed for quant.hip; scales per
    // 16-column block (the two directions of a projection have their own), fp32 biases.  xproj / lin / pred / whh above stay empty then.
    struct Q8Layer { int8_t* w = nullptr; float* scale = nullptr; float* bias = nullptr; };
    Q8Layer q_ih[2], q_hh[2], q_lin[2], q_pred;      // q_ih: 256 -> 2048 (b_ih); q_hh: packed by pack_q8_whh, scale [2], bias b_hh [2][1024]
    void* zero_page = nullptr;   // 256 zero bytes (padding source of the LDS-DMA conv variant)
    // ---- the dictionary of decoder='wordbeamsearch' (bbocr_set_dictionary): the root owns both copies (wd_buf, wd_table below)
    WordDictDev wd_dev;          // the uploaded table; slots == null: none on the device (no dictionary, or more than 128 classes)
    const WdTable* wd_host = nullptr;   // the host's copy; null: no dictionary
};

// One bbocr_ctx = the ROOT (what bbocr_create returns: configuration, weights, the compute stream, the call-slot pool) and, at the
// same time, call slot 0.  The reference shares ONE Reader between ThreadPoolExecutor workers (batch_processor_enhanced.py:215,
// default 2): a second call arriving while one is in flight takes a second slot -- a context of the same type that owns its own work
// buffers, side stream and events, shares the root's weights (WeightView copy) and queues its kernels on the SAME compute stream, so
// the card executes the two calls' kernels in issue order with no gap: call B's detector runs while call A's host thread is busy
// with the last pass's box geometry, CTC read-back and result export (the ~8 % of a step that left the card idle).
struct bbocr_ctx : WeightView {
    bbocr_config cfg{};
    int cfg_beam_wide = 0;                    // bbocr_config_v2::beam_wide (bbocr_create: 0)
    bbocr_ctx* root = nullptr;                // slot -> its root; the root points at itself
    std::vector<bbocr_ctx*> slots;            // root only: extra call slots, created when a second call arrives while the first is running
    std::mutex pool_mu;                       // root only: guards slot_busy / slots / err / prof totals / last_times
    std::condition_variable pool_cv;
    std::mutex enq_mu;                        // root only: held while a slot queues ONE block of launches (a detector pass, a recogniser part, a
                                              // sequence stage) on the shared compute stream, so that blocks of concurrent calls do not interleave kernel
                                              // by kernel (the per-launch HIP events of the roofline leg would then time foreign kernels too)
    ConvRoute op_conv_route{};                // root only (guarded by pool_mu): what the last bbocr_op_conv2d launch recorded (bbocr_op_conv2d_route)
    bool slot_busy = false;                   // this slot is running a call
    hipStream_t stream = nullptr;             // the compute stream (root's; slots share it: kernels of concurrent calls run in issue order)
    DevBuf pp_gray, pp_a, pp_b, pp_c, pp_tab;  // pre-processing chain (f2): planes and small tables
    DevBuf ac_work;                            // text-region auto-crop (autocrop.cpp): planes, packed masks, labels, boxes
    DevBuf th_coef;                            // OCR-input thumbnail (thumb.cpp): resample tables, kept while the geometry repeats
    int th_coef_key[6] = {0, 0, 0, 0, 0, 0};
    int th_coef_ks[2] = {0, 0};
    int th_coef_rows[2] = {0, 0};
    DevBuf je_scan, je_out;                    // model-input JPEG encoder (jpegenc.cpp): the unstuffed scan + stuffing counters, the stuffed scan
    DevBuf pe_out;                             // device PNG writer (pngenc.cpp): the compacted deflate blocks
    DevBuf pp_cubic;                           // cubic-resize weight tables, kept on the device while (W, dw, H, dh) repeats
    int pp_cubic_key[4] = {0, 0, 0, 0};
    unsigned long long pp_cubic_K[2] = {0, 0};
    unsigned int ignore_mask[4] = {0, 0, 0, 0};   // recogniser class mask of the running call (bbocr_params::ignore_mask)
    int beam_width = 0;                           // > 0: decoder='beamsearch' for the running call (bbocr_params::decoder / beam_width)
    bool word_beam = false;                       // ... 'wordbeamsearch' over the root's dictionary, at that width
    DevBuf wd_buf;                                // root only: the uploaded dictionary, slots then byte pool (WeightView::wd_dev points into it)
    std::unique_ptr<WdTable> wd_table;            // root only: the host's table (WeightView::wd_host)
    DevBuf wb_segs, wb_meta, wb_text;             // word search on the device: segment table + lengths, per-sequence {first segment, count} + the counter, the segments' texts
    std::vector<unsigned int> class_mask;         // more than 128 classes: the calling thread's bbocr_set_class_mask words, padded to ceil(C / 32)
    DevBuf ctc_mask;                              // ... on the device (uploaded by the sequence stage that reads them)
    int ctc_host_seqs = 0;                        // sequences of this slot's latest call that a CTC_BEAM_DEVICE_WIDE pass left to the host search (bbocr_last_ctc_host_sequences)
    int ctc_last_route = -1;                      // what ctc_route answered for this slot's latest sequence pass (CTC_*); published per calling thread with the stage times (bbocr_last_ctc_route)
    hipStream_t cur = nullptr;                // stream the layer helpers launch on
    SideLane upload_lane;                     // root only: bbocr_upload_pages copies here (an upload never waits for a running call)
    SideLane jpeg_lane;                       // root only: the JPEG batches of jpegdec.cpp run here; its mutex guards the jd_* buffers
    PinBuf jd_pin;                            // the batch's tables + unstuffed entropy bytes, staged for one H2D copy into jd_in
    DevBuf jd_in, jd_work, jd_coef, jd_stage; // per-subsequence states and component planes, coefficients, bbocr_op_jpeg_stage's scratch image
    DevBuf jd_page;                           // bbocr_jpeg_imread: the batch's un-oriented decodes, between the decoder and page_orient
    long long jd_count[4] = {0, 0, 0, 0};     // bbocr_jpeg_counters: files decoded, entropy runs, IDCT passes, output passes (per file each)
    hipStream_t seq_stream = nullptr;         // per slot: the recogniser's SEQUENCE stage (projections, BiLSTMs, linears, CTC, read-back) -- latency-bound
                                              // launches of 100-300 workgroups that leave most of the card idle -- runs here, behind an event of this
                                              // slot's feature parts, so that it overlaps the OTHER call's detector instead of queueing in front of it
    hipEvent_t feat_ev = nullptr;             // end of this slot's latest feature part on the compute stream
    hipStream_t stream2 = nullptr;            // box extraction of detector sub-batch k runs here while sub-batch k+1 is on `stream` (per slot)
    std::vector<hipEvent_t> sub_events;       // one per detector sub-batch of a readtext_batch call
    hipEvent_t ccl_t0 = nullptr, ccl_t1 = nullptr;   // GPU span of the CCL kernels of one boxes_impl call
    hipEvent_t det_t0 = nullptr, det_t1 = nullptr;   // detector span on `stream` (the host is busy with boxes meanwhile)
    hipEvent_t sync_ev = nullptr;             // "this slot's work so far" on a stream (slot_sync)
    hipEvent_t seq_t1 = nullptr, seq_t2 = nullptr;   // end of the sequence stage / of CTC + read-back (rec_finish)
    std::string err;                          // root: message of the last failed call (any slot)
    float times[8] = {0};                     // the running call's stage times; published per calling thread when the call ends

    // ---- optional per-launch timing of the conv_mfma kernel (HIP events on the compute stream)
    struct ProfRec { hipEvent_t e0, e1; double flops; int group; };
    int profiling = 0;                        // root: 0 off, 1 = time the detector's conv launches (group 0), 2 = also the recogniser's
    int prof_group = 0;                     // 0 = detector, 1 = recogniser
    std::vector<ProfRec> prof_recs;           // per slot: launches recorded by the running call
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[2] = {0, 0}, prof_flops[2] = {0, 0};   // root: totals
    long long prof_launches[2] = {0, 0};

    void* dist_comm = nullptr;                // root: RCCL communicator of the bbocr_dist_* entry points (dist.cpp), or null
    int dist_rank = 0, dist_world = 0;
    std::unique_ptr<HostPool> pool;           // per slot, made on first use: host threads for box geometry / beam search (hostpool.h)
    std::vector<void*> owned;    // root: every hipMalloc'd weight block, in load order (the order of the weight blob, bbocr_weights_export)
    std::vector<size_t> owned_bytes;

    Arena arena;
    DevBuf heat, gray, resized;
    DevBuf pg_rgb, pg_tab;                    // bbocr_readtext_pages: the packed RGB pages (shape group by shape group; `gray` holds the planes), the page tables
    PinBuf pg_pin;                            // staging of the page tables' upload
    DevBuf ccl_label, ccl_stat, ccl_slot, ccl_comps, ccl_rowext, ccl_counters;
    DevBuf crop_desc, crop_scratch, crop_hscratch, crop_wscratch, crop_luts, crop_hist;
    DevBuf ctc_idx, ctc_pmax, ctc_out_idx, ctc_out, ctc_probs, ctc_beam_idx, ctc_beam_len, ctc_cand, ctc_cand_n, crop_desc2;
    PinBuf desc_pin, desc_pin2;               // staging of crop_desc / crop_desc2 uploads
    PinBuf ctc_pin;                           // CTC results land here (pinned: the 1.7 MB D2H copy of a 64-page pass runs at link speed)
    DevBuf seq_v, seq_xp, seq_h, seq_lin, seq_logits, seq_tables;
    DevBuf seq_q8, seq_rowp;                  // rec_quant: the coded rows int8 [rows, 512] and their float4 parameters
};

// element type of a network's MFMA operands / stored activations (El<> in common.h), from bbocr_config::precision
inline int det_el(const bbocr_ctx* c) { return (c->cfg.precision == BBOCR_PREC_FP16 || c->cfg.precision == BBOCR_PREC_EXACT || c->cfg.precision == BBOCR_PREC_EXACT_REC) ? 1 : 0; }
inline int rec_el(const bbocr_ctx* c) { return c->cfg.precision != BBOCR_PREC_BF16 ? 1 : 0; }     // MIXED: bf16 detector, fp16 recogniser
inline bool rec_split(const bbocr_ctx* c) { return c->cfg.precision == BBOCR_PREC_EXACT || c->cfg.precision == BBOCR_PREC_EXACT_REC; }   // recogniser tensors are [hi | lo] fp16 pairs
inline bool rec_quant(const bbocr_ctx* c) { return c->cfg.rec_quant == 1; }     // sequence half in dynamic int8 (quant.hip); needs rec_split
// classes of the recogniser (bbocr_config::rec_classes, 0 = english_g2's 97) and the row stride of its fp32 logits / probabilities: whole
// 16-column groups, as the conv epilogue stores them (97 -> 112)
constexpr int kRecClassesDefault = 97;
inline int rec_classes(const bbocr_ctx* c) { return c->cfg.rec_classes > 0 ? c->cfg.rec_classes : kRecClassesDefault; }
inline int rec_cs(const bbocr_ctx* c) { return (rec_classes(c) + 15) / 16 * 16; }
inline bool rec_wide(const bbocr_ctx* c) { return rec_classes(c) > 128; }       // beyond ctc_rows_kernel, bbocr_params::ignore_mask and ctc_beam_kernel
inline bool rec_beam_wide(const bbocr_ctx* c) { return c->cfg_beam_wide == 1 && rec_wide(c); }   // beam searches of a wide context go to ctc_beam_wide.hip
inline bool det_split(const bbocr_ctx* c) { return c->cfg.precision == BBOCR_PREC_EXACT; }   // and so are the detector's (split-fp16 plans in every layer)

// ------------------------------------------------------------------------------------------------ shared types
struct TensorMap {
    std::unordered_map<std::string, const bbocr_tensor_desc*> m;
    bool zeros = false;                       // allocation-only load (bbocr_alloc_weights): every tensor exists and is all zeros
    std::vector<float> zero_buf;              // sized once (pointers handed out stay valid): the largest tensor is fc6, 1024 x 512 x 9
    TensorMap() : zeros(true), zero_buf((size_t)5 << 20, 0.f) {}
    TensorMap(const bbocr_tensor_desc* d, int n) {
        for (int i = 0; i < n; ++i) {
            std::string k = d[i].name ? d[i].name : "";
            if (k.rfind("module.", 0) == 0) k = k.substr(7);
            m[k] = &d[i];
        }
    }
    const float* get(const std::string& name, size_t numel, bool required = true) const {
        if (zeros) {
            if (zero_buf.size() < numel) fail(BBOCR_ERR_INTERNAL, "allocation-only load: tensor '" + name + "' larger than the zero buffer");
            return zero_buf.data();
        }
        auto it = m.find(name);
        if (it == m.end()) {
            if (required) fail(BBOCR_ERR_WEIGHTS, "missing tensor '" + name + "'");
            return nullptr;
        }
        size_t n = 1;
        for (int i = 0; i < it->second->ndim; ++i) n *= (size_t)it->second->shape[i];
        if (n != numel || !it->second->data)
            fail(BBOCR_ERR_WEIGHTS, "tensor '" + name + "' has " + std::to_string(n) + " elements, expected " + std::to_string(numel));
        return it->second->data;
    }
};

struct RgbSource { const uint8_t* rgb; int Himg, Wimg; };   // conv1_2 with conv1_1 fused in: a0 then only carries the canvas shape

struct DetDims {
    int H32, W32, h, w, th, tw;
    double ratio;
};

struct DetPlan {           // det_plan: the detector passes of B pages of one shape H x W
    int H, W;
    DetDims d;
    std::vector<int> passes;                 // pages per pass
    size_t arena_bytes, resized_bytes;       // activation arena of the largest pass; its resized pages (0: the pages are not resized)
};

// The gray planes a recognition reads: B pages of ONE shape back to back at `gray`, or -- tab != null, bbocr_readtext_pages -- pages of
// their own shapes, page b at gray + tab[b].off (tab_dev: the same table on the device, what the crop kernels index with CropDesc::img)
struct GrayPages {
    const uint8_t* gray;
    int H, W;
    const CropPage* tab = nullptr;
    const CropPage* tab_dev = nullptr;
    int h(int b) const { return tab ? tab[b].H : H; }
    int w(int b) const { return tab ? tab[b].W : W; }
};

struct HostBoxes {
    std::vector<std::vector<std::array<int, 8>>> polys;
    std::vector<std::vector<std::array<int, 4>>> hori;
    std::vector<std::vector<std::array<double, 8>>> freeb;
};

struct BoxJob {            // one box to recognise
    int img;
    bool is_free;
    double quad[8];        // reported corners
    CropDesc d;
    std::vector<int> text;
    double conf = 0.0;
};

struct RecChunk {
    int imgW, T, first, n;   // descriptors [first, first+n) share the padded width imgW
    size_t row0;             // first pooled row of the chunk in the pass's sequence tensors
};

struct RecPart {
    std::vector<CropDesc> descs;
    std::vector<int> order;          // position in the pass's result vectors for each descriptor
    std::vector<RecChunk> chunks;
    size_t rows = 0, cols = 0;       // pooled rows / wide-image columns of this part
    bool any_warp = false, any_tall = false;
};

struct RecRun {
    std::vector<int> tiles, seqs, seq_k;   // int4 {row0, n, T, 0} per LSTM workgroup; int2 {row0, T} and result position per sequence
    size_t rows = 0;
    int n_results = 0;
};

struct RecEarly {
    bool active = false;
    int pages = 0;
    std::vector<BoxJob> jobs;
    std::vector<int> box_off;        // [pages + 1]
    size_t a_total = 0, w_total = 0; // crop scratch consumed by those jobs
    RecPart part;
};

constexpr int REC_GAP = 4;
constexpr int REC_STAGES = 8;        // stages of the recogniser's conv stack (crnn_features_stages)

// ------------------------------------------------------------------------------------------------ shared functions
template <typename T> inline T* upload(bbocr_ctx* c, const std::vector<T>& v) {
    void* d = nullptr;
    HIPCHK(hipMalloc(&d, v.size() * sizeof(T)));
    c->owned.push_back(d);
    c->owned_bytes.push_back(v.size() * sizeof(T));
    HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T*)d;
}

ConvPlan make_plan(int Cin, int Cout, int KH, int KW, int pad, int dil, int el = 0, int bn = 0);
void upload_plan(bbocr_ctx* c, ConvPlan& p, const std::vector<float>& w, const std::vector<float>& b);
void free_weights(bbocr_ctx* c);
size_t weights_blob_bytes(const bbocr_ctx* c);
void weights_export(bbocr_ctx* c, void* dev_dst, size_t bytes);
void weights_import(bbocr_ctx* c, const void* dev_src, size_t bytes);
void load_craft(bbocr_ctx* c, const TensorMap& tm);
void load_crnn(bbocr_ctx* c, const TensorMap& tm);
ConvArgs conv_args(const ConvPlan& p, const Act& a0, const Act* a1 = nullptr, const Act* addup = nullptr, const Act* addsame = nullptr);
hipError_t launch_conv_profiled(bbocr_ctx* c, const ConvPlan& p, ConvArgs a, bool may_decline = false);   // may_decline: hipErrorNotSupported is returned, not thrown
void run_conv(bbocr_ctx* c, const ConvPlan& p, const Act& a0, bool relu0, const Act* a1, bool relu1, bool relu_out, void* out, int out_cs, int cout_store, bool out_f32, const Act* addup = nullptr, const Act* addsame = nullptr);
hipError_t launch_seq_proj_profiled(bbocr_ctx* c, const ConvPlan& p, const uint16_t* x, size_t rows_pad, uint16_t* out);   // hipErrorNotSupported is returned, not thrown
void prof_collect(bbocr_ctx* c);
Act conv_act(bbocr_ctx* c, const ConvPlan& p, const Act& a0, bool relu0, const Act* a1, bool relu1, bool relu_out, int store);
Act conv_pool_act(bbocr_ctx* c, const ConvPlan& p, const Act& a0, bool relu0, bool relu_out, int store, int mode, bool pool_relu, Act* full, const RgbSource* rgb = nullptr);
Act pool_act(bbocr_ctx* c, const Act& a, int kh, int kw, int sh, int sw, int ph, int pw, bool relu_in);
void craft_up_stage(bbocr_ctx* c, const ConvPlan& py, const ConvPlan& ps, const Act& y, const Act& skip, uint16_t* z, uint16_t* out);
void craft_fc_stage(bbocr_ctx* c, const Act& p5, const Act& s4, uint16_t* z, uint16_t* out);
bool craft_up3b_post(bbocr_ctx* c, const Act& u3a, uint16_t* u3b, uint16_t* z);      // true: the one fused launch ran; false: the two launches
bool craft_up4(bbocr_ctx* c, const Act& s1, const uint16_t* z, uint16_t* u4b);       // likewise
void craft_cls_tail(bbocr_ctx* c, const Act& c2, float* heat);
// The exact-mode detector (craft_forward_exact): its stage functions and the table of its conv launches, in the pass's order.  Every Act is a
// pair tensor [hi | lo] whose C counts both halves.
struct ExactConvRow {
    const char* name;
    ConvPlan bbocr_ctx::* plan;
    bool relu_out;
    int store;             // logical channels stored
    int pool_mode;         // 0: none, 1: MaxPool2d(2, 2) in the epilogue
    bool pool_relu;        // ReLU on the pooled values (the full tensor stays as relu_out says)
    bool keep_full;        // the un-pooled tensor is written too (a U-net skip)
};
int craft_exact_rows();
const ExactConvRow& craft_exact_row(int row);
Act craft_exact_conv(bbocr_ctx* c, int row, const Act& in, Act* full = nullptr);
Act craft_exact_conv1_1(bbocr_ctx* c, const uint8_t* rgb, int nb, int Himg, int Wimg, int H32, int W32);
Act craft_exact_relu(bbocr_ctx* c, const Act& a);
Act craft_exact_upcat(bbocr_ctx* c, const Act& y, const Act& skip);
Act craft_exact_pool5(bbocr_ctx* c, const Act& s4);
void craft_exact_cls_tail(bbocr_ctx* c, const Act& c3, float* heat);
DetDims det_dims(int H, int W, int canvas, double mag);
void detect_impl(bbocr_ctx* c, const uint8_t* rgb, int B, int H, int W, const bbocr_params& p, float* heat, const std::function<void(int, int)>& after_sub = nullptr);
DetPlan det_plan(bbocr_ctx* c, int B, int H, int W, const bbocr_params& p, bool overlapped);      // detect_impl's three steps
void det_size(bbocr_ctx* c, size_t arena_bytes, size_t resized_bytes);
void det_run(bbocr_ctx* c, const DetPlan& s, const uint8_t* rgb, float* heat, const std::function<void(int, int)>& after_sub = nullptr);
int ccl_cap_comps(int B, int h, int w);
void ccl_size(bbocr_ctx* c, size_t npx, int cap_comps);
void boxes_impl(bbocr_ctx* c, const float* heat, int B, int h, int w, double ratio, const bbocr_params& p, HostBoxes& hb, hipStream_t st);
bbocr_boxlist* export_boxes(const HostBoxes& hb);
void import_boxes(const bbocr_boxlist* bl, HostBoxes& hb);
bool plan_horizontal(const std::array<int, 4>& box, int img, int H, int W, BoxJob& j);
bool plan_free(const std::array<double, 8>& fq, int img, BoxJob& j);
int rec_mode(const bbocr_ctx* c);
void crop_refit_fw(CropDesc& d);
void rec_layout_scratch(std::vector<BoxJob>& jobs, size_t first, size_t& a_total, size_t& w_total);
bool contrast_lut(const unsigned int* hist, size_t npx, double target, uint8_t* lut);
std::vector<int> crop_contrast_luts(bbocr_ctx* c, const CropDesc* descs_dev, std::vector<CropDesc>& descs, double target, std::vector<uint8_t>& luts);
void rec_launch_crops(bbocr_ctx* c, const GrayPages& g, const RecPart& part, const CropDesc* dd, uint16_t* wide, int stage);
void rec_plan_part(const std::vector<BoxJob>& jobs, const std::vector<int>& sel, int res0, size_t row_base, RecPart& part);
const CropDesc* rec_upload_descs(bbocr_ctx* c, const RecPart& part, DevBuf& desc_buf);
uint16_t* rec_wide_image(bbocr_ctx* c, const RecPart& part);
void crnn_features_wide(bbocr_ctx* c, const RecPart& part, const CropDesc* descs, const uint16_t* wide);
Act crnn_stage_shape(const bbocr_ctx* c, const RecPart& part, int stage);
Act crnn_features_stages(bbocr_ctx* c, const RecPart& part, const CropDesc* descs, Act a, int first, int last);
void rec_add_tables(RecRun& run, const RecPart& part, int tile_seqs);
void crnn_sequence(bbocr_ctx* c, size_t rows, size_t rows_pad, const int* tiles_dev, int ntiles, const int* seqs_dev, int nseq, float* logits);
void crnn_seq_xproj(bbocr_ctx* c, int l, const uint16_t* x, size_t rows_pad, void* xp);         // crnn_sequence's three GEMMs
void crnn_seq_xproj_conv(bbocr_ctx* c, int l, const uint16_t* x, size_t rows_pad, void* xp);    // xproj through run_conv (exact mode; declined shapes)
void crnn_seq_lin(bbocr_ctx* c, int l, const uint16_t* h, size_t rows_pad, uint16_t* out);
void crnn_seq_pred(bbocr_ctx* c, const uint16_t* x, size_t rows_pad, float* logits);
void rec_seq_tiles(const bbocr_ctx* c, RecRun& run);    // rec_quant: run.tiles rebuilt as the int8 recurrence's {first sequence, n, longest T, 0}
// where the text of a CTC pass comes from (ctc_route).  CTC_GREEDY_FUSED: greedy over more than 128 classes with Prediction inside the CTC
// kernel (pred_ctc.hip) -- the pass has no logits.  CTC_BEAM_DEVICE_WIDE: the device search over more than 128 classes (ctc_beam_wide.hip),
// taken only by a context created with bbocr_config_v2::beam_wide
// CTC_WORD_HOST / CTC_WORD_DEVICE: decoder='wordbeamsearch' (wordbeam_route below; ctc_wordbeam.cpp / ctc_wordbeam.hip).
enum { CTC_GREEDY = 0, CTC_BEAM_HOST = 1, CTC_BEAM_DEVICE = 2, CTC_GREEDY_FUSED = 3, CTC_BEAM_DEVICE_WIDE = 4, CTC_WORD_HOST = 5, CTC_WORD_DEVICE = 6 };
int wordbeam_route(int beam_width, int C, const int* seqs, int nseq);
// the device half of a word search over sequences already on the device at seqs_dev (ctc_wordbeam.cpp): buffers sized, kernels queued on s;
// the text lands in c->ctc_beam_idx (row-indexed) / c->ctc_beam_len.  idx_dev null: the rows' arg-max is computed from the probabilities
void wordbeam_device(bbocr_ctx* c, const float* probs_dev, const int* idx_dev, size_t rows, int C, int cs, const int* seqs, const int* seqs_dev, int nseq,
                     int beam_width, hipStream_t s);
// seqs: {first row, T} per sequence (host); fused_ok: the caller holds Prediction's input and pred_ctc_kernel's weights (a 16-bit recognition pass);
// beam_wide: bbocr_config_v2::beam_wide of the context
int ctc_route(int beam_width, int C, const int* seqs, int nseq, bool fused_ok = false, bool beam_wide = false);
// after the wait of a CTC_BEAM_DEVICE_WIDE pass: the sequences the kernel left to the host (blen[i] == -1, a row of more than kBeamWideCand
// candidates) are searched by ctc_beam_search_host from their own rows of probs_dev, copied over `s` -> texts[i] (sized nseq); returns their number
int ctc_beam_wide_fallback(bbocr_ctx* c, hipStream_t s, const float* probs_dev, const int* seqs, int nseq, int C, int cs, int beam_width, const int* blen,
                           std::vector<std::vector<int>>& texts);
const unsigned int* thread_class_mask(const bbocr_ctx* root, int* n_words);   // abi.cpp: the calling thread's bbocr_set_class_mask words for `root`, or null
void ctc_size(bbocr_ctx* c, size_t rows, int nseq, int cs, int route);
double ctc_decode(const CtcOut& o, const int* idx, int n, std::vector<int>& text);
void rec_early_begin(bbocr_ctx* c, const GrayPages& g, int pages, int B, const HostBoxes& hb, const bbocr_params& p, RecEarly& e);
void recognize_impl(bbocr_ctx* c, const GrayPages& g, int B, const HostBoxes& hb, const bbocr_params& p, std::vector<BoxJob>& jobs, std::vector<int>& box_off, RecEarly* early = nullptr);
bbocr_result* export_result(int B, const std::vector<BoxJob>& jobs, const std::vector<int>& box_off);
void pp_resize(bbocr_ctx* c, const uint8_t* src, int H, int W, uint8_t* dst, int dh, int dw, bool src_bgr = false);   // enqueues; the caller waits
void pp_gauss(bbocr_ctx* c, const uint8_t* src, int H, int W, uint8_t* dst, double sigma);
const uint8_t* pp_fold_lut(bbocr_ctx* c, size_t n, double contrast, double brightness);
bool pp_clahe_tiles(int H, int W, int* th, int* tw);
int pp_unsharp_box_r(float radius);
void pp_clahe(bbocr_ctx* c, const uint8_t* src, int H, int W, const uint8_t* d_lut, uint8_t* dst, double clip_limit);
void pp_unsharp(bbocr_ctx* c, const uint8_t* src, int H, int W, uint8_t* dst, uint8_t* tmp1, uint8_t* tmp2, float radius, int percent, int threshold);
void preprocess_chain_impl(bbocr_ctx* c, const uint8_t* bgr, int H, int W, const bbocr_preproc_params& q, uint8_t* out, int dh, int dw);
void gaussian_taps_fixed(int n, double sigma, int* k);   // autocrop.cpp

// worker threads of this slot: bbocr_config::host_threads, or min(16, the process's CPU share); the pool is made once and kept
inline HostPool& host_pool(bbocr_ctx* c) {
    if (!c->pool) {
        const int want = c->cfg.host_threads > 0 ? c->cfg.host_threads : std::min(16, host_cpu_share());
        c->pool.reset(new HostPool(std::max(1, std::min(want, 64)) - 1));
    }
    return *c->pool;
}

// is another pipeline call running on this context right now (another call slot busy)?
inline bool other_call_in_flight(bbocr_ctx* c) {
    bbocr_ctx* root = c->root;
    std::lock_guard<std::mutex> lk(root->pool_mu);
    if (root != c && root->slot_busy) return true;
    for (bbocr_ctx* s : root->slots)
        if (s != c && s->slot_busy) return true;
    return false;
}

// ---- call slots
struct EnqLock {       // see bbocr_ctx::enq_mu; never held across a host wait for the device
    std::unique_lock<std::mutex> lk;
    explicit EnqLock(bbocr_ctx* c) : lk(c->root->enq_mu) {}
};
constexpr int kMaxSlots = 2;       // calls in flight per context (the reference runs 2 ThreadPoolExecutor workers on one Reader)
bbocr_ctx* slot_create(bbocr_ctx* root);                 // abi.cpp
void slot_destroy(bbocr_ctx* s);                         // abi.cpp (everything but the shared compute stream and the weights)
void publish_times(const bbocr_ctx* s);                  // abi.cpp: the finished call's stage times -> the calling thread's record
void dist_release(bbocr_ctx* root);                      // dist.cpp

// wait for what THIS slot has queued on `st` so far (the compute stream is shared between slots: hipStreamSynchronize would also wait for
// the other call's kernels queued behind ours -- and the card would then run dry while both hosts wait)
inline void slot_sync(bbocr_ctx* c, hipStream_t st) {
    if (!c->sync_ev) HIPCHK(hipEventCreateWithFlags(&c->sync_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->sync_ev, st));
    HIPCHK(hipEventSynchronize(c->sync_ev));
}

inline void prof_release(bbocr_ctx* c, const bbocr_ctx::ProfRec& r) { c->prof_pool.push_back(r.e0); c->prof_pool.push_back(r.e1); }   // events back to the pool

// bbocr.h promises that a call returns with its own work finished -- also when it fails half-way: kernels already queued may still
// read caller-owned inputs / write caller-owned outputs, and host vectors that were async-copy targets die during unwinding
inline void guarded_drain(bbocr_ctx* ctx) {
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->seq_stream) (void)hipStreamSynchronize(ctx->seq_stream);
    ctx->cur = ctx->stream;
    (void)hipGetLastError();
    for (auto& r : ctx->prof_recs) prof_release(ctx, r);
    ctx->prof_recs.clear();
}

// RAII lease of a call slot.  exclusive: every slot (weight loading / export / import, anything that changes what the slots share).
struct SlotLease {
    bbocr_ctx* root;
    bbocr_ctx* slot = nullptr;
    bool exclusive;
    SlotLease(bbocr_ctx* r, bool excl) : root(r), exclusive(excl) {
        std::unique_lock<std::mutex> lk(root->pool_mu);
        const int max_slots = root->cfg.call_slots == 1 ? 1 : kMaxSlots;
        if (exclusive) {
            root->pool_cv.wait(lk, [&] {
                if (root->slot_busy) return false;
                for (bbocr_ctx* s : root->slots) if (s->slot_busy) return false;
                return true;
            });
            root->slot_busy = true;
            for (bbocr_ctx* s : root->slots) s->slot_busy = true;
            slot = root;
            return;
        }
        for (;;) {
            if (!root->slot_busy) { slot = root; break; }
            for (bbocr_ctx* s : root->slots) if (!s->slot_busy) { slot = s; break; }
            if (slot) break;
            if ((int)root->slots.size() + 1 < max_slots) {
                slot = slot_create(root);              // may throw StatusError: nothing is leased then
                root->slots.push_back(slot);
                break;
            }
            root->pool_cv.wait(lk);
        }
        slot->slot_busy = true;
        if (slot != root) {
            static_cast<WeightView&>(*slot) = static_cast<const WeightView&>(*root);   // weights may have been loaded since the slot was made
            slot->cfg = root->cfg;
            slot->cfg_beam_wide = root->cfg_beam_wide;
            slot->profiling = root->profiling;
        }
    }
    ~SlotLease() {
        {
            std::lock_guard<std::mutex> lk(root->pool_mu);
            if (exclusive) {
                root->slot_busy = false;
                for (bbocr_ctx* s : root->slots) s->slot_busy = false;
            } else if (slot) {
                slot->slot_busy = false;
            }
        }
        root->pool_cv.notify_all();
    }
};

inline void set_err(bbocr_ctx* root, const std::string& m) {
    std::lock_guard<std::mutex> lk(root->pool_mu);
    root->err = m;
}

// f() as an entry point's status: the one mapping of a failure to a status code and the context's message (bbocr_last_error)
template <typename F> inline int status_of(bbocr_ctx* root, F&& f) {
    if (!root) return BBOCR_ERR_ARG;
    try {
        f();
        return BBOCR_OK;
    } catch (const StatusError& se) {
        set_err(root, se.msg);
        return se.code;
    } catch (const std::exception& ex) {
        set_err(root, ex.what());
        return BBOCR_ERR_INTERNAL;
    } catch (...) {
        set_err(root, "unknown failure");
        return BBOCR_ERR_INTERNAL;
    }
}

// every pipeline entry point runs inside guarded(): device selected, a call slot leased, exceptions mapped to status codes.  f(slot) does the work.
template <typename F> inline int guarded(bbocr_ctx* root, F&& f, bool exclusive = false) {
    return status_of(root, [&] {
        HIPCHK(hipSetDevice(root->cfg.device));
        SlotLease lease(root, exclusive);
        bbocr_ctx* ctx = lease.slot;
        try {
            ctx->cur = ctx->stream;
            // the library runs on its own non-blocking streams: what the caller queued on the default stream (torch's) -- fills of
            // output buffers, input copies -- must be complete before our kernels touch the same memory
            HIPCHK(hipStreamSynchronize(nullptr));
            f(ctx);
            publish_times(ctx);
        } catch (...) {
            guarded_drain(ctx);                      // still inside the lease: nobody else touches this slot's buffers meanwhile
            throw;
        }
    });
}

// an entry point outside the call slots runs inside lane_guarded(): device selected, the lane's mutex held, its stream made on first use,
// the default stream waited for where the caller's fills and allocations matter (wait_default).  f(stream) does the work; when it fails
// the lane's stream is drained before the status is returned, so that nothing queued still reads or writes caller-owned memory.
template <typename F> inline int lane_guarded(bbocr_ctx* root, SideLane bbocr_ctx::*which, bool wait_default, F&& f) {
    return status_of(root, [&] {
        HIPCHK(hipSetDevice(root->cfg.device));
        SideLane& lane = root->*which;
        std::lock_guard<std::mutex> lk(lane.mu);
        try {
            if (!lane.stream) HIPCHK(hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking));
            if (wait_default) HIPCHK(hipStreamSynchronize(nullptr));
            f(lane.stream);
        } catch (...) {
            if (lane.stream) (void)hipStreamSynchronize(lane.stream);
            (void)hipGetLastError();
            throw;
        }
    });
}
