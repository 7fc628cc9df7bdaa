// Recogniser orchestration: crops (utils.py::get_image_list), AlignCollate, CRNN forward, CTC, contrast retry, rotation variants (easyocr recognition.py::get_text).
#include "ctx.h"

// AlignCollate's content width of the stage-A image rw x rh (after a rotation, if any) inside the padded width imgW
void crop_refit_fw(CropDesc& d) {
    const int cw = (int)std::ceil(64 * ((double)d.rw / (double)d.rh));
    d.fw = cw > d.imgW ? d.imgW : cw;
}

// get_image_list's resize target and own padded width of a width x height crop; false = degenerate
static bool plan_sizes(CropDesc& d, int width, int height) {
    double ratio = (double)width / (double)height;
    if (ratio < 1.0) {
        ratio = 1.0 / ratio;
        d.rw = 64; d.rh = (int)(64 * ratio);
    } else {
        d.rw = (int)(64 * ratio); d.rh = 64;
    }
    if ((int)(64 * ratio) == 0) return false;
    d.imgW = (int)std::ceil(std::max(ratio, 1.0)) * 64;
    crop_refit_fw(d);
    return d.rw > 0 && d.rh > 0 && d.fw > 0;
}

// AlignCollate / get_image_list geometry of one horizontal box; false = skipped (degenerate)
bool plan_horizontal(const std::array<int, 4>& box, int img, int H, int W, BoxJob& j) {
    const int x_min = std::max(0, box[0]), x_max = std::min(box[1], W), y_min = std::max(0, box[2]), y_max = std::min(box[3], H);
    const int width = x_max - x_min, height = y_max - y_min;
    if (width <= 0 || height <= 0) return false;
    j.img = img;
    j.is_free = false;
    const double q[8] = {(double)x_min, (double)y_min, (double)x_max, (double)y_min, (double)x_max, (double)y_max, (double)x_min, (double)y_max};
    memcpy(j.quad, q, sizeof(q));
    CropDesc& d = j.d;
    memset(&d, 0, sizeof(d));
    d.img = img; d.sx0 = x_min; d.sy0 = y_min; d.sw = width; d.sh = height; d.warp = 0; d.lut_off = -1;
    return plan_sizes(d, width, height);
}

bool plan_free(const std::array<double, 8>& fq, int img, BoxJob& j) {
    float rect[4][2];
    for (int i = 0; i < 4; ++i) { rect[i][0] = (float)fq[2 * i]; rect[i][1] = (float)fq[2 * i + 1]; }
    auto dist = [&](int a, int b) {
        const float dx = rect[a][0] - rect[b][0], dy = rect[a][1] - rect[b][1];
        const float t0 = dx * dx, t1 = dy * dy;
        return std::sqrt(t0 + t1);   // float32, as numpy on a float32 array
    };
    const int maxW = std::max((int)dist(2, 3), (int)dist(1, 0));
    const int maxH = std::max((int)dist(1, 2), (int)dist(0, 3));
    if (maxW <= 0 || maxH <= 0) return false;
    j.img = img;
    j.is_free = true;
    memcpy(j.quad, fq.data(), 64);
    CropDesc& d = j.d;
    memset(&d, 0, sizeof(d));
    d.img = img; d.sx0 = 0; d.sy0 = 0; d.sw = maxW; d.sh = maxH; d.warp = 1; d.lut_off = -1;
    bbocr::perspective_inverse(rect, maxW, maxH, d.Minv);
    return plan_sizes(d, maxW, maxH);
}

// tensor mode of the recogniser (kernels.h REC_*) and stored 16-bit elements per logical channel
int rec_mode(const bbocr_ctx* c) { return rec_split(c) ? REC_SPLIT : (rec_el(c) ? REC_F16 : REC_BF16); }
static inline int rec_mul(const bbocr_ctx* c) { return rec_split(c) ? 2 : 1; }

// The conv stack of the recogniser over the WIDE image [64][part.cols] of a part (16-bit; exact mode: codes): every crop side by side with
// 4 zero columns between neighbours (CropDesc::slot = first column), so each layer is ONE launch over [H, Wt] whatever the mix of width
// buckets.  The separator columns are each layer's zero padding; convolutions write into them, so they are cleared on every layer output
// (4 >> shift columns per crop).  The 3-row mean is gathered straight into every crop's pooled rows of c->seq_v (CropDesc::pad_).
// The stack is REC_STAGES stages, a stage = a layer with the gap clear that follows it:
//   0 conv0 + ReLU + pool | 1 r1 + pool | 2 r2 | 3 r3 + (2,1) pool | 4 r4 | 5 r5 + (2,1) pool | 6 r6 | 7 3-row mean + gather
// crnn_stage_shape: the wide tensor stage `stage` reads (p = null); stage == REC_STAGES: what the last one leaves, the part's rows of seq_v.
Act crnn_stage_shape(const bbocr_ctx* c, const RecPart& part, int stage) {
    static const int H[REC_STAGES] = {64, 32, 16, 16, 8, 8, 4, 3}, C[REC_STAGES] = {1, 32, 64, 128, 128, 256, 256, 256};
    const int m = rec_mul(c), Wt = (int)part.cols;
    if (stage < 0 || stage > REC_STAGES) fail(BBOCR_ERR_INTERNAL, "recogniser conv stack: no such stage");
    if (stage == REC_STAGES) return Act{nullptr, 1, 1, (int)part.rows, 256 * m};
    const int W = stage == 0 ? Wt : (stage == 1 ? Wt / 2 : (stage == 7 ? Wt / 4 - 1 : Wt / 4));
    return Act{nullptr, 1, H[stage], W, stage == 0 ? 1 : C[stage] * m};
}

// Stages first..last on `a`, the input of stage `first` in the wide layout (crnn_stage_shape; its gap columns zero).  Returns the output of
// stage `last`: an arena tensor, or after stage 7 c->seq_v (whose rows CropDesc::pad_ + t were written).  A recognition pass runs 0..7
// (crnn_features_wide), the per-stage tests (tools/micro/stage_shim.hip) any range.
// descs: the part's descriptors on the device.  In a dry arena pass nothing is launched.
Act crnn_features_stages(bbocr_ctx* c, const RecPart& part, const CropDesc* descs, Act a, int first, int last) {
    Arena& ar = c->arena;
    c->prof_group = 1;
    const int m = rec_mul(c), count = (int)part.descs.size();
    if (first < 0 || last >= REC_STAGES || first > last) fail(BBOCR_ERR_INTERNAL, "recogniser conv stack: bad stage range");
    auto gaps = [&](const Act& t, int shift) {
        if (!ar.dry) HIPCHK(launch_crnn_zero_gaps(t.p, descs, 0, count, t.H, t.W, t.C, shift, c->cur));
    };
    for (int s = first; s <= last; ++s) {
        const Act want = crnn_stage_shape(c, part, s);
        if (a.N != want.N || a.H != want.H || a.W != want.W || a.C != want.C) fail(BBOCR_ERR_INTERNAL, "recogniser conv stack: stage input of another shape");
        switch (s) {
        case 0: {
            const int Wt = a.W;
            Act c0{ar.alloc<uint16_t>((size_t)32 * (Wt / 2) * 32 * m), 1, 32, Wt / 2, 32 * m};
            if (!ar.dry) HIPCHK(launch_crnn_conv0(a.p, c->r0_wb, c->r0_wb + 288, c0.p, 1, Wt, rec_mode(c), c->cur, c->r0_afrag));
            gaps(c0, 1);
            a = c0;
            break;
        }
        case 1: a = conv_pool_act(c, c->r1, a, false, true, 64, 1, false, nullptr); gaps(a, 2); break;
        case 2: a = conv_act(c, c->r2, a, false, nullptr, false, true, 128); gaps(a, 2); break;
        case 3: a = conv_pool_act(c, c->r3, a, false, true, 128, 2, false, nullptr); gaps(a, 2); break;
        case 4: a = conv_act(c, c->r4, a, false, nullptr, false, true, 256); gaps(a, 2); break;
        case 5: a = conv_pool_act(c, c->r5, a, false, true, 256, 2, false, nullptr); gaps(a, 2); break;
        case 6: a = conv_act(c, c->r6, a, false, nullptr, false, true, 256); break;   // [1, 3, Wt/4 - 1, 256]
        default:
            if (!ar.dry) HIPCHK(launch_rowmean3_gather(a.p, a.W, 256, descs, 0, count, (uint16_t*)c->seq_v.p, rec_mode(c), c->cur));
            a = Act{(uint16_t*)c->seq_v.p, 1, 1, (int)part.rows, 256 * m};
        }
    }
    return a;
}

void crnn_features_wide(bbocr_ctx* c, const RecPart& part, const CropDesc* descs, const uint16_t* wide) {
    (void)crnn_features_stages(c, part, descs, Act{(uint16_t*)wide, 1, 64, (int)part.cols, 1}, 0, REC_STAGES - 1);
}

// Sequence half of the recogniser over the POOLED time steps of every bucket (rows = sum n_i*T_i, padded to x256):
// v bf16 [rows,256] (ctx->seq_v) -> logits fp32 [rows,112].  The two linear layers and both input projections are
// single GEMMs over all rows; each BiLSTM layer is ONE launch whose workgroups carry their own sequence length.
// rec_quant: every matrix product as [parameter pass, coding pass, int8 GEMM] with one set of activation parameters per crop (seqs_dev), the
// recurrence as lstm_q8_kernel; all tensors between the products are fp32.
static void crnn_sequence_q8(bbocr_ctx* c, size_t rows, size_t rows_pad, const int* tiles_dev, int ntiles, const int* seqs_dev, int nseq, float* logits) {
    c->seq_xp.ensure(rows_pad * 2048 * 4);
    c->seq_h.ensure(rows_pad * 512 * 4);
    c->seq_lin.ensure(rows_pad * 256 * 4);
    c->seq_q8.ensure(rows_pad * 512);
    c->seq_rowp.ensure(rows_pad * 16);
    int8_t* a8 = (int8_t*)c->seq_q8.p;
    float* rowp = (float*)c->seq_rowp.p;
    auto qlinear = [&](const void* x, int pair, int K, const bbocr_ctx::Q8Layer& L, int N, float* out) {
        HIPCHK(launch_q8_quantize(x, pair, K, rows, rows_pad, seqs_dev, nseq, rowp, a8, nullptr, nullptr, c->cur));
        HIPCHK(launch_q8_gemm(a8, rows_pad, K, L.w, N, rowp, L.scale, L.bias, out, N, c->cur));
    };
    const void* cur = c->seq_v.p;                     // the conv stack's features: the exact mode's fp16 pair, rebuilt in fp32 by the coding pass
    for (int l = 0; l < 2; ++l) {
        qlinear(cur, l == 0, 256, c->q_ih[l], 2048, (float*)c->seq_xp.p);
        HIPCHK(launch_lstm_q8((const float*)c->seq_xp.p, c->q_hh[l].w, c->q_hh[l].scale, c->q_hh[l].bias, (float*)c->seq_h.p, seqs_dev, tiles_dev, ntiles,
                              nullptr, nullptr, nullptr, c->cur));
        float* dst = (float*)(l == 0 ? c->seq_lin.p : c->seq_v.p);
        qlinear(c->seq_h.p, 0, 512, c->q_lin[l], 256, dst);
        cur = dst;
    }
    qlinear(cur, 0, 256, c->q_pred, rec_cs(c), logits);
}

// the int8 recurrence's workgroups take LSTM_Q8_SEQS consecutive sequences of the table, each with its own T
void rec_seq_tiles(const bbocr_ctx* c, RecRun& run) {
    if (!rec_quant(c)) return;
    run.tiles.clear();
    const int nseq = (int)(run.seqs.size() / 2);
    for (int s0 = 0; s0 < nseq; s0 += LSTM_Q8_SEQS) {
        const int n = std::min(LSTM_Q8_SEQS, nseq - s0);
        int tmax = 0;
        for (int i = 0; i < n; ++i) tmax = std::max(tmax, run.seqs[2 * (s0 + i) + 1]);
        const int t[4] = {s0, n, tmax, 0};
        run.tiles.insert(run.tiles.end(), t, t + 4);
    }
}

void crnn_sequence(bbocr_ctx* c, size_t rows, size_t rows_pad, const int* tiles_dev, int ntiles, const int* seqs_dev, int nseq, float* logits) {
    c->prof_group = 1;
    c->arena.dry = false;
    if (rec_quant(c)) { crnn_sequence_q8(c, rows, rows_pad, tiles_dev, ntiles, seqs_dev, nseq, logits); return; }
    const bool sp = rec_split(c);
    const int m = rec_mul(c);
    c->seq_xp.ensure(rows_pad * 2048 * (sp ? 4 : 2));            // exact mode: the input projection stays fp32
    c->seq_h.ensure(rows_pad * 512 * 2 * m);
    c->seq_lin.ensure(rows_pad * 256 * 2 * m);
    const uint16_t* cur = (const uint16_t*)c->seq_v.p;
    for (int l = 0; l < 2; ++l) {
        crnn_seq_xproj(c, l, cur, rows_pad, c->seq_xp.p);
        HIPCHK(launch_lstm(c->seq_xp.p, c->whh[l], (uint16_t*)c->seq_h.p, tiles_dev, ntiles, rec_mode(c), c->whh_scale[l], c->cur));
        uint16_t* dst = (uint16_t*)(l == 0 ? c->seq_lin.p : c->seq_v.p);
        crnn_seq_lin(c, l, (const uint16_t*)c->seq_h.p, rows_pad, dst);
        cur = dst;
    }
    if (logits) crnn_seq_pred(c, cur, rows_pad, logits);      // null: the pass's CTC route holds Prediction itself (CTC_GREEDY_FUSED) and reads seq_v
}

// The sequence half's three GEMMs as 1x1 convs over the rows laid out as an image [1, rows_pad / 256, 256, C] (rows_pad: a multiple of 256).
// Exact mode: x and h are [hi | lo] pairs and the plans are split-fp16 plans; the input projection and the logits leave as fp32.
static Act seq_rows(const bbocr_ctx* c, const uint16_t* p, size_t rows_pad, int C) { return Act{(uint16_t*)p, 1, (int)(rows_pad / 256), 256, C * rec_mul(c)}; }
// x [rows_pad, 256] -> the LSTM's input projection [rows_pad, 2048] in lstm8_xproj_channel's order (fp32 in the exact mode)
// as a 1x1 conv (conv1x1_dma_kernel's 256 x 256 tiles): the exact mode's path, and the path of any shape launch_seq_proj declines
void crnn_seq_xproj_conv(bbocr_ctx* c, int l, const uint16_t* x, size_t rows_pad, void* xp) {
    run_conv(c, c->xproj[l], seq_rows(c, x, rows_pad, 256), false, nullptr, false, false, xp, 2048, 2048, rec_split(c));
}
// the 16-bit modes stream the rows past register-resident weights (seq_proj.hip); the values are crnn_seq_xproj_conv's bit for bit
void crnn_seq_xproj(bbocr_ctx* c, int l, const uint16_t* x, size_t rows_pad, void* xp) {
    if (!rec_split(c)) {
        if (c->arena.dry) return;
        if (launch_seq_proj_profiled(c, c->xproj[l], x, rows_pad, (uint16_t*)xp) == hipSuccess) return;
    }
    crnn_seq_xproj_conv(c, l, x, rows_pad, xp);
}
// h [rows_pad, 512] (exact: the LSTM's pair, lo half unscaled) -> [rows_pad, 256]
void crnn_seq_lin(bbocr_ctx* c, int l, const uint16_t* h, size_t rows_pad, uint16_t* out) {
    run_conv(c, c->lin[l], seq_rows(c, h, rows_pad, 512), false, nullptr, false, false, out, 256 * rec_mul(c), 256, false);
}
// x [rows_pad, 256] -> logits fp32 [rows_pad, rec_cs] (english_g2: 97 classes in 112 columns; the columns behind the classes belong to no class)
void crnn_seq_pred(bbocr_ctx* c, const uint16_t* x, size_t rows_pad, float* logits) {
    run_conv(c, c->pred, seq_rows(c, x, rows_pad, 256), false, nullptr, false, false, logits, rec_cs(c), rec_cs(c), true);
}

// A recognition pass = feature PARTS + one sequence stage.  A part is a set of crops standing side by side in ONE wide image
// (CropDesc::slot = first column, 4 zero columns after every crop; ::pad_ = first pooled row), so each CRNN conv layer is a single
// launch per part whatever the mix of widths; every part gathers its pooled time steps into the pass's shared [rows,256] tensor,
// and the sequence stage (input projections, both BiLSTM layers, linear layers, class projection, CTC) then runs ONCE over all rows.
// readtext_batch uses two parts: the crops of the first detector pass's pages go through the conv stack while the last pass's boxes
// are still being extracted (CCL + host geometry), so that stretch no longer leaves the card idle.
// pooled time steps per sequence pass (~6.6 KB of work buffers each); bbocr_config::rec_max_cols (pixel columns, 4 per time step) overrides
// More than 128 classes on the unfused route (beam search, the exact modes): the pass also holds rows_pad * rec_cs fp32 logits, and as many
// probabilities for a beam search -- each buffer is kept at or below kRecWideBufBytes, which at 6,719 classes is 39,936 rows
constexpr size_t kRecWideBufBytes = (size_t)1 << 30;
static bool rec_fused_ok(const bbocr_ctx* c) { return rec_wide(c) && !rec_split(c) && !rec_quant(c) && c->pred_wide; }
static size_t rec_max_rows(const bbocr_ctx* c) {
    size_t lim = c->cfg.rec_max_cols > 0 ? (size_t)std::max(64, c->cfg.rec_max_cols / 4) : (size_t)1500000;
    if (rec_wide(c) && !(rec_fused_ok(c) && c->beam_width <= 0))
        lim = std::min(lim, std::max<size_t>(256, kRecWideBufBytes / ((size_t)rec_cs(c) * 4) / 256 * 256));
    return lim;
}

// lay the crops `sel` (indices into jobs; result position = res0 + position in sel) out as one part whose rows start at row_base
void rec_plan_part(const std::vector<BoxJob>& jobs, const std::vector<int>& sel, int res0, size_t row_base, RecPart& part) {
    std::map<int, std::vector<int>> buckets;          // by padded width, box order kept inside a bucket
    for (size_t k = 0; k < sel.size(); ++k) buckets[jobs[sel[k]].d.imgW].push_back((int)k);
    size_t rows = row_base, cols = 0;
    for (auto& kv : buckets) {
        const int imgW = kv.first, T = imgW / 4 - 1;
        RecChunk ch{imgW, T, (int)part.descs.size(), (int)kv.second.size(), rows};
        for (int i = 0; i < ch.n; ++i) {
            const int k = kv.second[i];
            CropDesc d = jobs[sel[k]].d;
            if (cols > 0x7ff00000u) fail(BBOCR_ERR_OVERFLOW, "recogniser pass wider than 2^31 columns");
            d.slot = (int)cols;
            d.pad_ = (int)(rows + (size_t)i * T);
            cols += (size_t)imgW + REC_GAP;
            part.any_warp |= d.warp != 0;
            part.any_tall |= !(d.fw == d.rw && d.rh == 64);
            part.descs.push_back(d);
            part.order.push_back(res0 + k);
        }
        rows += (size_t)ch.n * T;
        part.chunks.push_back(ch);
    }
    part.rows = rows - row_base;
    part.cols = cols;
}

// The three steps of enqueueing a part; nothing here waits for the device (the buffers it needs are sized by the caller).
// 1. the part's descriptors -> desc_buf, through the pinned staging buffer that goes with it
const CropDesc* rec_upload_descs(bbocr_ctx* c, const RecPart& part, DevBuf& desc_buf) {
    const size_t bytes = part.descs.size() * sizeof(CropDesc);
    desc_buf.ensure(bytes);
    PinBuf& pin = (&desc_buf == &c->crop_desc2) ? c->desc_pin2 : c->desc_pin;
    pin.ensure(bytes);
    memcpy(pin.p, part.descs.data(), bytes);
    HIPCHK(hipMemcpyAsync(desc_buf.p, pin.p, bytes, hipMemcpyHostToDevice, c->stream));
    return (const CropDesc*)desc_buf.p;
}

// 2. the arena sized for the part's conv stack (dry pass) and begun again; returns the part's wide image [64][part.cols], carved first.
// The caller fills it, then 3. crnn_features_wide.
uint16_t* rec_wide_image(bbocr_ctx* c, const RecPart& part) {
    c->arena.begin(true);
    (void)c->arena.alloc<uint16_t>((size_t)64 * part.cols);
    crnn_features_wide(c, part, nullptr, nullptr);
    c->arena.buf.ensure(c->arena.off);
    c->arena.begin(false);
    return c->arena.alloc<uint16_t>((size_t)64 * part.cols);
}

// the crop launches of a part whose descriptors are on the device at dd: stage 1 = gather / warp + cv2 resize into the crop scratch (wide: null),
// stage 2 = AlignCollate into the wide image [64][part.cols] in the context's recogniser mode
void rec_launch_crops(bbocr_ctx* c, const GrayPages& g, const RecPart& part, const CropDesc* dd, uint16_t* wide, int stage) {
    const int n = (int)part.descs.size(), Wt = (int)part.cols;
    HIPCHK(launch_crops(g.gray, g.H, g.W, dd, 0, n, 0, part.any_warp, part.any_tall, (uint8_t*)c->crop_wscratch.p, (uint8_t*)c->crop_scratch.p,
                        (uint8_t*)c->crop_hscratch.p, (const uint8_t*)c->crop_luts.p, wide, stage, c->stream, wide ? Wt : 0, wide ? REC_GAP : 0,
                        wide ? rec_mode(c) : 0, g.tab_dev));
}

// enqueue a part: descriptor upload, crops (stage A = gather / warp + cv2 resize when asked, stage B = AlignCollate into the wide image),
// conv stack, pooled rows into seq_v
static void rec_launch_part(bbocr_ctx* c, const GrayPages& g, const RecPart& part, DevBuf& desc_buf, bool stage_a) {
    if (part.descs.empty()) return;
    EnqLock enq(c);                           // one feature part = one contiguous block on the compute stream
    const CropDesc* dd = rec_upload_descs(c, part, desc_buf);
    if (stage_a) rec_launch_crops(c, g, part, dd, nullptr, 1);
    uint16_t* wide = rec_wide_image(c, part);
    rec_launch_crops(c, g, part, dd, wide, 2);
    crnn_features_wide(c, part, dd, wide);
    if (!c->feat_ev) HIPCHK(hipEventCreateWithFlags(&c->feat_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->feat_ev, c->stream));      // what the sequence stage (on seq_stream) waits for
}

void rec_add_tables(RecRun& run, const RecPart& part, int tile_seqs) {
    for (const RecChunk& ch : part.chunks) {
        for (int s0 = 0; s0 < ch.n; s0 += tile_seqs) {
            run.tiles.push_back((int)(ch.row0 + (size_t)s0 * ch.T));
            run.tiles.push_back(std::min(tile_seqs, ch.n - s0));
            run.tiles.push_back(ch.T);
            run.tiles.push_back(0);
        }
        for (int i = 0; i < ch.n; ++i) {
            run.seqs.push_back((int)(ch.row0 + (size_t)i * ch.T));
            run.seqs.push_back(ch.T);
            run.seq_k.push_back(part.order[ch.first + i]);
        }
    }
    run.rows += part.rows;
}

// where a CTC pass's text comes from: the greedy collapse, or ctcBeamSearch on the device (widths up to BBOCR_BEAM_DEVICE_MAX whose longest
// sequence fits the kernel's LDS block) or on the host (wider beams, longer sequences: the probabilities cross to the host).  More than 128
// classes are searched on the device only where the context asks for it (bbocr_config_v2::beam_wide), under the same two conditions.
int ctc_route(int beam_width, int C, const int* seqs, int nseq, bool fused_ok, bool beam_wide) {
    if (beam_width <= 0) return (C > 128 && fused_ok) ? CTC_GREEDY_FUSED : CTC_GREEDY;
    int max_T = 0;
    for (int i = 0; i < nseq; ++i) max_T = std::max(max_T, seqs[2 * i + 1]);
    if (beam_wide && ctc_beam_wide_on_device(beam_width, C, max_T)) return CTC_BEAM_DEVICE_WIDE;
    return ctc_beam_on_device(beam_width, C, max_T) ? CTC_BEAM_DEVICE : CTC_BEAM_HOST;
}

int ctc_beam_wide_fallback(bbocr_ctx* c, hipStream_t s, const float* probs_dev, const int* seqs, int nseq, int C, int cs, int beam_width, const int* blen,
                           std::vector<std::vector<int>>& texts) {
    texts.assign((size_t)nseq, {});
    std::vector<int> over, tab;            // the overflowed sequences; their {first row, T} in the host copy
    size_t rows = 0;
    for (int i = 0; i < nseq; ++i)
        if (blen[i] < 0) {
            over.push_back(i);
            tab.push_back((int)rows);
            tab.push_back(seqs[2 * i + 1]);
            rows += (size_t)seqs[2 * i + 1];
        }
    if (over.empty()) return 0;
    std::vector<float> probs(rows * (size_t)cs);
    for (size_t k = 0; k < over.size(); ++k)
        if (tab[2 * k + 1] > 0)
            HIPCHK(hipMemcpyAsync(probs.data() + (size_t)tab[2 * k] * cs, probs_dev + (size_t)seqs[2 * over[k]] * cs, (size_t)tab[2 * k + 1] * cs * sizeof(float),
                                  hipMemcpyDeviceToHost, s));
    slot_sync(c, s);
    std::vector<std::vector<int>> found;
    ctc_beam_search_batch(probs.data(), tab.data(), (int)over.size(), C, cs, beam_width, found, &host_pool(c));
    for (size_t k = 0; k < over.size(); ++k) texts[over[k]].swap(found[k]);
    return (int)over.size();
}

// device buffers of one launch_ctc over `rows` time steps of `nseq` sequences (cs: row stride of the logits; a beam route keeps the
// probabilities, the device route adds the search's row-indexed text and its lengths)
void ctc_size(bbocr_ctx* c, size_t rows, int nseq, int cs, int route) {
    c->ctc_idx.ensure(rows * 4);
    c->ctc_pmax.ensure(rows * 4);
    c->ctc_out_idx.ensure(rows * 4);
    c->ctc_out.ensure((size_t)nseq * sizeof(CtcOut));
    if (route == CTC_BEAM_HOST || route == CTC_BEAM_DEVICE || route == CTC_BEAM_DEVICE_WIDE || route == CTC_WORD_HOST || route == CTC_WORD_DEVICE)
        c->ctc_probs.ensure(rows * cs * sizeof(float));          // (the word search's own device buffers: wordbeam_device)
    if (route == CTC_BEAM_DEVICE || route == CTC_BEAM_DEVICE_WIDE) {
        c->ctc_beam_idx.ensure(rows * 4);
        c->ctc_beam_len.ensure((size_t)nseq * 4);
    }
    if (route == CTC_BEAM_DEVICE_WIDE) {         // the rows' candidate lists: 1 KB per row, and their counts
        c->ctc_cand.ensure(rows * (size_t)kBeamWideCand * 8);
        c->ctc_cand_n.ensure(rows * 4);
    }
}

// CtcOut -> (text, confidence) of one sequence: the text is the n classes at idx (the sequence's rows of launch_ctc's out_idx and o.len, or a
// beam search's answer); the confidence is the greedy path's either way
double ctc_decode(const CtcOut& o, const int* idx, int n, std::vector<int>& text) {
    text.assign(idx, idx + n);
    // custom_mean: prod ** (2 / sqrt(len)); an all-blank sequence scores np.array([0])
    return o.cnt > 0 ? std::pow((double)o.prod, 2.0 / std::sqrt((double)o.cnt)) : 0.0;
}

// sequence stage + CTC over every row the parts of `run` produced; texts / confs are indexed by result position
static void rec_finish(bbocr_ctx* c, RecRun& run, std::vector<std::vector<int>>& texts, std::vector<double>& confs) {
    const size_t rows = run.rows;
    if (rows == 0) return;
    const size_t rows_pad = align_up(rows, 256);
    auto t0 = clk::now();
    rec_seq_tiles(c, run);
    {   // longest sequences first: the launch ends with the shortest tails
        std::vector<int>& tiles = run.tiles;
        const size_t nt = tiles.size() / 4;
        std::vector<size_t> perm(nt);
        for (size_t i = 0; i < nt; ++i) perm[i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](size_t x, size_t y) { return tiles[x * 4 + 2] > tiles[y * 4 + 2]; });
        std::vector<int> t2(tiles.size());
        for (size_t i = 0; i < nt; ++i) memcpy(&t2[i * 4], &tiles[perm[i] * 4], 16);
        tiles.swap(t2);
    }
    const std::vector<int>&tiles = run.tiles, &seqs = run.seqs;
    const int ntiles = (int)(tiles.size() / 4), nseq = (int)(seqs.size() / 2);
    const int C = rec_classes(c), cs = rec_cs(c);
    const int route = c->word_beam ? wordbeam_route(c->beam_width, C, seqs.data(), nseq)
                                   : ctc_route(c->beam_width, C, seqs.data(), nseq, rec_fused_ok(c), rec_beam_wide(c));
    c->ctc_last_route = route;
    const bool dev_beam = route == CTC_BEAM_DEVICE || route == CTC_BEAM_DEVICE_WIDE || route == CTC_WORD_DEVICE;   // text and lengths come back, not probabilities
    const bool host_beam = route == CTC_BEAM_HOST || route == CTC_WORD_HOST;               // the probabilities cross to the host's search
    const bool fused = route == CTC_GREEDY_FUSED, beam = host_beam || dev_beam;
    if (!fused) c->seq_logits.ensure(rows_pad * cs * 4);
    c->seq_tables.ensure((tiles.size() + seqs.size()) * 4);
    int* tiles_dev = (int*)c->seq_tables.p;
    int* seqs_dev = tiles_dev + tiles.size();
    ctc_size(c, rows, nseq, cs, route);
    if (rec_wide(c)) c->ctc_mask.ensure(c->class_mask.size() * 4);
    // pinned read-back block: greedy classes [rows] | CtcOut [nseq] | device route: beam text [rows] | its lengths [nseq]
    const size_t oo_off = align_up(rows * 4, 16);
    const size_t bi_off = align_up(oo_off + (size_t)nseq * sizeof(CtcOut), 16), bl_off = bi_off + align_up(rows * 4, 16);
    c->ctc_pin.ensure(dev_beam ? bl_off + (size_t)nseq * 4 : bi_off);
    const int* oidx = (const int*)c->ctc_pin.p;
    const CtcOut* oo = (const CtcOut*)((const char*)c->ctc_pin.p + oo_off);
    const int* bidx = (const int*)((const char*)c->ctc_pin.p + bi_off);
    const int* blen = (const int*)((const char*)c->ctc_pin.p + bl_off);
    std::vector<float> probs(host_beam ? rows * cs : 0);      // only a host route moves the probabilities off the card
    std::vector<std::vector<int>> beam_texts;
    if (!c->seq_t1) { HIPCHK(hipEventCreate(&c->seq_t1)); HIPCHK(hipEventCreate(&c->seq_t2)); }
    {
        // Sequence stage, CTC and the read-back of its results: one block, ONE host wait.  It runs on the slot's own seq_stream behind the
        // event of this slot's feature parts: its launches are latency chains of 100-300 workgroups (BiLSTM: 4.9 us per time step against
        // 1 us of MFMA work) that leave most of the card idle -- with a second call in flight that call's detector fills it, instead of
        // waiting in (or making this stage wait in) the compute stream's FIFO.
        hipStream_t ss = (c->seq_stream && c->feat_ev) ? c->seq_stream : c->stream;
        std::unique_lock<std::mutex> enq;
        if (ss == c->stream) enq = std::unique_lock<std::mutex>(c->root->enq_mu);
        else HIPCHK(hipStreamWaitEvent(ss, c->feat_ev, 0));
        c->cur = ss;
        struct Restore { bbocr_ctx* c; ~Restore() { c->cur = c->stream; } } restore{c};
        HIPCHK(hipMemcpyAsync(tiles_dev, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, ss));
        HIPCHK(hipMemcpyAsync(seqs_dev, seqs.data(), seqs.size() * 4, hipMemcpyHostToDevice, ss));
        if (rec_wide(c)) HIPCHK(hipMemcpyAsync(c->ctc_mask.p, c->class_mask.data(), c->class_mask.size() * 4, hipMemcpyHostToDevice, ss));
        crnn_sequence(c, rows, rows_pad, tiles_dev, ntiles, seqs_dev, nseq, fused ? nullptr : (float*)c->seq_logits.p);
        HIPCHK(hipEventRecord(c->seq_t1, ss));
        if (fused) {             // Prediction inside the CTC kernel: the second BiLSTM stage's output (seq_v) in, no logits anywhere
            HIPCHK(launch_pred_ctc(rec_el(c), (const uint16_t*)c->seq_v.p, rows, c->pred_wide, c->pred_wide_b, C, (const unsigned int*)c->ctc_mask.p,
                                   (int*)c->ctc_idx.p, (float*)c->ctc_pmax.p, ss));
            HIPCHK(launch_ctc_collapse((const int*)c->ctc_idx.p, (const float*)c->ctc_pmax.p, seqs_dev, nseq, (int*)c->ctc_out_idx.p, (CtcOut*)c->ctc_out.p, ss));
        } else if (rec_wide(c)) {
            HIPCHK(launch_ctc_wide((const float*)c->seq_logits.p, rows, C, cs, seqs_dev, nseq, (int*)c->ctc_idx.p, (float*)c->ctc_pmax.p,
                                   (int*)c->ctc_out_idx.p, (CtcOut*)c->ctc_out.p, ss, (const unsigned int*)c->ctc_mask.p, beam ? (float*)c->ctc_probs.p : nullptr));
        } else {
            HIPCHK(launch_ctc((const float*)c->seq_logits.p, rows, C, cs, seqs_dev, nseq, (int*)c->ctc_idx.p, (float*)c->ctc_pmax.p,
                              (int*)c->ctc_out_idx.p, (CtcOut*)c->ctc_out.p, ss, c->ignore_mask, beam ? (float*)c->ctc_probs.p : nullptr));
        }
        if (!dev_beam) HIPCHK(hipMemcpyAsync(c->ctc_pin.p, c->ctc_out_idx.p, rows * 4, hipMemcpyDeviceToHost, ss));    // the search's text replaces it
        HIPCHK(hipMemcpyAsync((char*)c->ctc_pin.p + oo_off, c->ctc_out.p, (size_t)nseq * sizeof(CtcOut), hipMemcpyDeviceToHost, ss));
        if (dev_beam) {
            int max_T = 0;
            for (int i = 0; i < nseq; ++i) max_T = std::max(max_T, seqs[2 * i + 1]);
            if (route == CTC_WORD_DEVICE)          // word groups from the row kernel's arg-max, one search per group, the join: all behind the row kernel
                wordbeam_device(c, (const float*)c->ctc_probs.p, (const int*)c->ctc_idx.p, rows, C, cs, seqs.data(), seqs_dev, nseq, c->beam_width, ss);
            else if (route == CTC_BEAM_DEVICE_WIDE)
                HIPCHK(launch_ctc_beam_wide((const float*)c->ctc_probs.p, rows, C, cs, seqs_dev, nseq, max_T, c->beam_width, (int*)c->ctc_cand_n.p,
                                            (int*)c->ctc_cand.p, (int*)c->ctc_beam_idx.p, (int*)c->ctc_beam_len.p, ss));
            else
                HIPCHK(launch_ctc_beam((const float*)c->ctc_probs.p, rows, C, cs, seqs_dev, nseq, max_T, c->beam_width, (int*)c->ctc_beam_idx.p,
                                       (int*)c->ctc_beam_len.p, ss));
            HIPCHK(hipMemcpyAsync((char*)c->ctc_pin.p + bi_off, c->ctc_beam_idx.p, rows * 4, hipMemcpyDeviceToHost, ss));
            HIPCHK(hipMemcpyAsync((char*)c->ctc_pin.p + bl_off, c->ctc_beam_len.p, (size_t)nseq * 4, hipMemcpyDeviceToHost, ss));
        } else if (host_beam) {
            HIPCHK(hipMemcpyAsync(probs.data(), c->ctc_probs.p, probs.size() * sizeof(float), hipMemcpyDeviceToHost, ss));
        }
        HIPCHK(hipEventRecord(c->seq_t2, ss));
    }
    HIPCHK(hipEventSynchronize(c->seq_t2));
    float ctc_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ctc_ms, c->seq_t1, c->seq_t2));
    c->times[4] += (float)ms_since(t0) - ctc_ms;     // host wait for the recogniser's device work (conv stack of the parts + sequence stage)
    c->times[5] += ctc_ms;                           // CTC kernels + read-back (device span) ...
    t0 = clk::now();                                 // ... + the host decode below
    if (route == CTC_BEAM_HOST) ctc_beam_search_batch(probs.data(), seqs.data(), nseq, C, cs, c->beam_width, beam_texts, &host_pool(c));
    if (route == CTC_WORD_HOST)
        ctc_wordbeam_search_batch(probs.data(), seqs.data(), nseq, C, cs, c->beam_width, c->wd_host->space, c->wd_host, beam_texts, &host_pool(c));
    if (route == CTC_BEAM_DEVICE_WIDE) {   // the probabilities are still resident: only the overflowed sequences' rows cross the link
        hipStream_t ss = (c->seq_stream && c->feat_ev) ? c->seq_stream : c->stream;
        c->ctc_host_seqs += ctc_beam_wide_fallback(c, ss, (const float*)c->ctc_probs.p, seqs.data(), nseq, C, cs, c->beam_width, blen, beam_texts);
    }
    for (int i = 0; i < nseq; ++i) {       // the confidence stays the greedy path's for every route
        const int k = run.seq_k[i];
        if (host_beam || (route == CTC_BEAM_DEVICE_WIDE && blen[i] < 0)) confs[k] = ctc_decode(oo[i], beam_texts[i].data(), (int)beam_texts[i].size(), texts[k]);
        else if (dev_beam) confs[k] = ctc_decode(oo[i], bidx + seqs[2 * i], std::clamp(blen[i], 0, seqs[2 * i + 1]), texts[k]);
        else confs[k] = ctc_decode(oo[i], oidx + seqs[2 * i], oo[i].len, texts[k]);
    }
    c->times[5] += (float)ms_since(t0);
}

// split `sel` into runs whose pooled rows fit one sequence pass (in width order, like the wide image)
static std::vector<std::vector<int>> rec_split_runs(const bbocr_ctx* c, const std::vector<BoxJob>& jobs, const std::vector<int>& sel) {
    std::vector<int> byw(sel.size());
    for (size_t k = 0; k < sel.size(); ++k) byw[k] = (int)k;
    std::stable_sort(byw.begin(), byw.end(), [&](int x, int y) { return jobs[sel[x]].d.imgW < jobs[sel[y]].d.imgW; });
    std::vector<std::vector<int>> runs(1);
    size_t rows = 0;
    for (int k : byw) {
        const size_t t = (size_t)(jobs[sel[k]].d.imgW / 4 - 1);
        if (!runs.back().empty() && rows + t > rec_max_rows(c)) { runs.emplace_back(); rows = 0; }
        runs.back().push_back(k);
        rows += t;
    }
    return runs;
}

// run one recognition pass over `sel` (indices into jobs); descs must already carry lut_off for a contrast pass.
static void recognise_pass(bbocr_ctx* c, const GrayPages& g, std::vector<BoxJob>& jobs, const std::vector<int>& sel,
                           bool stage_a, std::vector<std::vector<int>>& texts, std::vector<double>& confs) {
    texts.assign(sel.size(), {});
    confs.assign(sel.size(), 0.0);
    if (sel.empty()) return;
    for (const std::vector<int>& ks : rec_split_runs(c, jobs, sel)) {
        // positions inside sel -> a sub-selection whose result positions are the positions in sel
        std::vector<int> sub(ks.size());
        for (size_t i = 0; i < ks.size(); ++i) sub[i] = sel[ks[i]];
        RecPart part;
        rec_plan_part(jobs, sub, 0, 0, part);
        for (size_t i = 0; i < part.order.size(); ++i) part.order[i] = ks[part.order[i]];
        auto t0 = clk::now();
        c->seq_v.ensure(align_up(part.rows, 256) * 256 * 2 * rec_mul(c));
        rec_launch_part(c, g, part, c->crop_desc, stage_a);
        c->times[3] += (float)ms_since(t0);
        RecRun run;
        rec_add_tables(run, part, lstm_tile_seqs(rec_mode(c)));
        rec_finish(c, run, texts, confs);
    }
}

// np.percentile(img, q) (method 'linear') from a 256-bin histogram of n uint8 samples
static double percentile_u8(const unsigned int* hist, size_t n, double q) {
    const double virt = (double)(n - 1) * (q / 100.0);
    const double prev = std::floor(virt);
    const double gamma = virt - prev;
    const size_t i0 = (size_t)prev, i1 = std::min(i0 + 1, n - 1);
    auto at = [&](size_t idx) {
        size_t acc = 0;
        for (int v = 0; v < 256; ++v) {
            acc += hist[v];
            if (idx < acc) return v;
        }
        return 255;
    };
    const int a = at(i0), b = at(i1);
    const double diff = (double)(b - a);
    double r = (double)a + diff * gamma;
    if (gamma >= 0.5) r = (double)b - diff * (1 - gamma);
    return r;
}

// adjust_contrast_grey of one crop of npx pixels from its histogram: false = its contrast is already >= target and the crop stays as it is,
// true = lut[256] maps it
bool contrast_lut(const unsigned int* hist, size_t npx, double target, uint8_t* lut) {
    const double high = percentile_u8(hist, npx, 90.0), lowp = percentile_u8(hist, npx, 10.0);
    const double contrast = (high - lowp) / std::max(10.0, high + lowp);
    if (!(contrast < target)) return false;
    const double ratio = 200.0 / std::max(10.0, high - lowp);
    for (int v = 0; v < 256; ++v) {
        double x = ((double)v - lowp + 25) * ratio;
        x = std::max(0.0, std::min(255.0, x));
        lut[v] = (uint8_t)x;
    }
    return true;
}

// adjust_contrast_grey's decision for stage-A crops that lie in the crop scratch (descs: their descriptors, on the device at descs_dev): the
// histograms, ONE host wait, then per crop whose contrast is below the target its LUT appended to `luts` and lut_off set to it.  Returns the
// indices of those crops; the others stay as they are (lut_off untouched).  Neither `luts` nor the changed descriptors are uploaded here.
std::vector<int> crop_contrast_luts(bbocr_ctx* c, const CropDesc* descs_dev, std::vector<CropDesc>& descs, double target, std::vector<uint8_t>& luts) {
    c->crop_hist.ensure(descs.size() * 256 * 4);
    HIPCHK(launch_crop_hist((const uint8_t*)c->crop_scratch.p, descs_dev, 0, (int)descs.size(), (unsigned int*)c->crop_hist.p, c->stream));
    std::vector<unsigned int> hist(descs.size() * 256);
    HIPCHK(hipMemcpyAsync(hist.data(), c->crop_hist.p, hist.size() * 4, hipMemcpyDeviceToHost, c->stream));
    slot_sync(c, c->stream);
    std::vector<int> changed;
    for (size_t k = 0; k < descs.size(); ++k) {
        uint8_t lut[256];
        if (!contrast_lut(&hist[k * 256], (size_t)descs[k].rw * descs[k].rh, target, lut)) continue;
        descs[k].lut_off = (int)luts.size();
        luts.insert(luts.end(), lut, lut + 256);
        changed.push_back((int)k);
    }
    return changed;
}

static void rec_check_params(bbocr_ctx* c, const bbocr_params& p) {
    if (!c->crnn_loaded) fail(BBOCR_ERR_STATE, "recogniser weights not loaded");
    if (p.ignore_mask[0] & 1u) fail(BBOCR_ERR_ARG, "the CTC blank (class 0) cannot be ignored");
    c->ctc_last_route = -1;          // until a sequence pass of this call has been routed (bbocr_last_ctc_route)
    c->ctc_host_seqs = 0;
    for (int i = 0; i < 4; ++i) c->ignore_mask[i] = p.ignore_mask[i];
    if (rec_wide(c)) {       // the calling thread's bbocr_set_class_mask words, copied into this slot: another call's mask is another slot's
        int n = 0;
        const unsigned int* w = thread_class_mask(c->root, &n);
        c->class_mask.assign((size_t)(rec_classes(c) + 31) / 32, 0u);
        for (int i = 0; i < n && i < (int)c->class_mask.size(); ++i) c->class_mask[i] = w[i];
    }
    if (p.decoder != BBOCR_DECODER_GREEDY && p.decoder != BBOCR_DECODER_BEAMSEARCH && p.decoder != BBOCR_DECODER_WORDBEAMSEARCH) fail(BBOCR_ERR_ARG, "unknown decoder");
    if (p.decoder != BBOCR_DECODER_GREEDY && p.beam_width <= 0) fail(BBOCR_ERR_ARG, "beam_width must be positive");
    if (p.decoder == BBOCR_DECODER_WORDBEAMSEARCH && !c->wd_host) fail(BBOCR_ERR_ARG, "decoder wordbeamsearch needs a dictionary (bbocr_set_dictionary)");
    c->beam_width = p.decoder != BBOCR_DECODER_GREEDY ? p.beam_width : 0;
    c->word_beam = p.decoder == BBOCR_DECODER_WORDBEAMSEARCH;
}

// Reader.recognize's per-box branch: horizontal boxes first, then free boxes, page by page
static void rec_plan_pages(const HostBoxes& hb, int b0, int b1, const GrayPages& g, std::vector<BoxJob>& jobs, std::vector<int>& box_off) {
    for (int b = b0; b < b1; ++b) {
        for (const auto& hbx : hb.hori[b]) {
            BoxJob j;
            if (plan_horizontal(hbx, b, g.h(b), g.w(b), j)) jobs.push_back(j);
        }
        for (const auto& fq : hb.freeb[b]) {
            BoxJob j;
            if (plan_free(fq, b, j)) jobs.push_back(j);
        }
        box_off[b + 1] = (int)jobs.size();
    }
}

// crop scratch offsets of jobs [first, end), continuing at a_total / w_total
void rec_layout_scratch(std::vector<BoxJob>& jobs, size_t first, size_t& a_total, size_t& w_total) {
    for (size_t i = first; i < jobs.size(); ++i) {
        BoxJob& j = jobs[i];
        j.d.a_off = (int)a_total;
        a_total += align_up((size_t)j.d.rw * j.d.rh, 16);
        if (j.d.warp) {
            j.d.warp_off = (int)w_total;
            w_total += align_up((size_t)j.d.sw * j.d.sh, 16);
        }
        if (a_total > 0x7fffffff || w_total > 0x7fffffff) fail(BBOCR_ERR_OVERFLOW, "crop scratch exceeds 2 GiB");
    }
}

// RecEarly: state of a recognition whose FIRST feature part (the crops of pages [0, pages)) was enqueued before the boxes of the remaining
// pages existed (readtext_batch: while the last detector pass's CCL + host geometry run).  recognize_impl picks it up and adds the rest.
// rec_early_begin enqueues the feature part of pages [0, pages) of a B-page batch; the buffers that must survive until the rest arrives (stage-A
// crops for the contrast retry, pooled rows) are sized for the whole batch by extrapolation
void rec_early_begin(bbocr_ctx* c, const GrayPages& g, int pages, int B, const HostBoxes& hb, const bbocr_params& p, RecEarly& e) {
    rec_check_params(c, p);
    e.box_off.assign(pages + 1, 0);
    rec_plan_pages(hb, 0, pages, g, e.jobs, e.box_off);
    if (e.jobs.empty()) return;
    rec_layout_scratch(e.jobs, 0, e.a_total, e.w_total);
    std::vector<int> all(e.jobs.size());
    for (size_t i = 0; i < all.size(); ++i) all[i] = (int)i;
    rec_plan_part(e.jobs, all, 0, 0, e.part);
    const double grow = 1.25 * (double)B / (double)pages;
    if ((double)e.part.rows * grow > (double)rec_max_rows(c)) { e = RecEarly(); return; }   // would not fit one sequence pass: no early part
    c->crop_scratch.ensure(std::max<size_t>((size_t)((double)e.a_total * grow), 16));
    c->crop_hscratch.ensure(std::max<size_t>((size_t)((double)e.a_total * grow), 16));
    c->crop_wscratch.ensure(std::max<size_t>((size_t)((double)e.w_total * grow), 16));
    c->crop_luts.ensure(256);
    c->seq_v.ensure(align_up((size_t)((double)e.part.rows * grow), 256) * 256 * 2 * rec_mul(c));
    auto t0 = clk::now();
    rec_launch_part(c, g, e.part, c->crop_desc, true);
    c->times[3] += (float)ms_since(t0);
    e.pages = pages;
    e.active = true;
}

void recognize_impl(bbocr_ctx* c, const GrayPages& g, int B, const HostBoxes& hb, const bbocr_params& p,
                           std::vector<BoxJob>& jobs, std::vector<int>& box_off, RecEarly* early) {
    rec_check_params(c, p);
    jobs.clear();
    box_off.assign(B + 1, 0);
    // rotation_info: Reader.recognize then takes its batched branch -- get_image_list over the whole page (free boxes first, result sorted
    // by the top y of the first corner), ONE padded width for every crop of the page (max_width), the list extended by np.rot90 copies of
    // every crop per angle (make_rotated_img_list), and per box the most confident variant kept (set_result_with_confidence)
    int angles[4] = {0, 0, 0, 0}, nrot = 0;
    for (int i = 0; i < 4 && p.rotation_info[i] != 0; ++i) {
        const int a = p.rotation_info[i];
        if (a != 90 && a != 180 && a != 270) fail(BBOCR_ERR_ARG, "rotation_info angles must be 90, 180 or 270");
        angles[nrot++] = a;
    }
    const bool resume = early && early->active && nrot == 0;
    size_t n_early = 0;
    if (resume) {                                  // pages [0, early->pages) are planned and their feature part is on the device
        jobs = std::move(early->jobs);
        n_early = jobs.size();
        for (int b = 0; b <= early->pages; ++b) box_off[b] = early->box_off[b];
        rec_plan_pages(hb, early->pages, B, g, jobs, box_off);
    }
    for (int b = 0; b < B && !resume; ++b) {
        if (nrot == 0) {
            rec_plan_pages(hb, b, b + 1, g, jobs, box_off);
            continue;
        } else {
            std::vector<BoxJob> page;
            for (const auto& fq : hb.freeb[b]) {
                BoxJob j;
                if (plan_free(fq, b, j)) page.push_back(j);
            }
            for (const auto& hbx : hb.hori[b]) {
                BoxJob j;
                if (plan_horizontal(hbx, b, g.h(b), g.w(b), j)) page.push_back(j);
            }
            std::stable_sort(page.begin(), page.end(), [](const BoxJob& x, const BoxJob& y) { return x.quad[1] < y.quad[1]; });
            int page_w = 64;                      // max(max_width, imgH); max_width = ceil(max ratio) * 64 = the widest own bucket
            for (const BoxJob& j : page) page_w = std::max(page_w, j.d.imgW);
            for (BoxJob& j : page) {
                j.d.imgW = page_w;
                crop_refit_fw(j.d);
                jobs.push_back(j);
            }
        }
        box_off[b + 1] = (int)jobs.size();
    }
    const size_t n_base = jobs.size();
    for (int r = 0; r < nrot; ++r)
        for (size_t i = 0; i < n_base; ++i) {
            BoxJob j = jobs[i];
            j.d.rot = angles[r] / 90;
            if (j.d.rot & 1) std::swap(j.d.rw, j.d.rh);
            crop_refit_fw(j.d);                       // AlignCollate on the rotated image
            jobs.push_back(j);
        }
    // the variants only live inside this function: whatever path returns, the caller sees one job per box
    struct Collapse {
        std::vector<BoxJob>& jobs; size_t n_base; int nrot;
        ~Collapse() {
            if (nrot == 0 || jobs.size() != n_base * (size_t)(nrot + 1)) return;
            for (size_t i = 0; i < n_base; ++i) {
                size_t best = i;
                for (int r = 1; r <= nrot; ++r)
                    if (jobs[(size_t)r * n_base + i].conf > jobs[best].conf) best = (size_t)r * n_base + i;     // first maximum wins
                if (best != i) { jobs[i].text = jobs[best].text; jobs[i].conf = jobs[best].conf; }
            }
            jobs.resize(n_base);
        }
    } collapse{jobs, n_base, nrot};
    if (jobs.empty()) return;
    std::vector<std::vector<int>> texts;
    std::vector<double> confs;
    if (resume) {
        size_t a_total = early->a_total, w_total = early->w_total;
        rec_layout_scratch(jobs, n_early, a_total, w_total);
        c->crop_scratch.ensure_keep(std::max<size_t>(a_total, 16), early->a_total);   // part 1's stage-A crops feed the contrast retry
        c->crop_hscratch.ensure_keep(std::max<size_t>(a_total, 16), 0);
        c->crop_wscratch.ensure_keep(std::max<size_t>(w_total, 16), 0);
        texts.assign(jobs.size(), {});
        confs.assign(jobs.size(), 0.0);
        std::vector<int> rest(jobs.size() - n_early);
        for (size_t i = 0; i < rest.size(); ++i) rest[i] = (int)(n_early + i);
        RecPart part2;
        rec_plan_part(jobs, rest, (int)n_early, early->part.rows, part2);
        RecRun run;
        rec_add_tables(run, early->part, lstm_tile_seqs(rec_mode(c)));
        if (early->part.rows + part2.rows <= rec_max_rows(c)) {
            c->seq_v.ensure_keep(align_up(early->part.rows + part2.rows, 256) * 256 * 2 * rec_mul(c), early->part.rows * 256 * 2 * rec_mul(c));
            auto t0 = clk::now();
            rec_launch_part(c, g, part2, c->crop_desc2, true);
            c->times[3] += (float)ms_since(t0);
            rec_add_tables(run, part2, lstm_tile_seqs(rec_mode(c)));
            rec_finish(c, run, texts, confs);
        } else {                                   // the rest does not fit the same sequence pass: finish part 1, then the rest on its own
            rec_finish(c, run, texts, confs);
            std::vector<std::vector<int>> t2;
            std::vector<double> c2;
            recognise_pass(c, g, jobs, rest, true, t2, c2);
            for (size_t i = 0; i < rest.size(); ++i) { texts[rest[i]] = t2[i]; confs[rest[i]] = c2[i]; }
        }
        early->active = false;
    } else {
        size_t a_total = 0, w_total = 0;
        rec_layout_scratch(jobs, 0, a_total, w_total);
        c->crop_scratch.ensure(std::max<size_t>(a_total, 16));
        c->crop_hscratch.ensure(std::max<size_t>(a_total, 16));
        c->crop_wscratch.ensure(std::max<size_t>(w_total, 16));
        c->crop_luts.ensure(256);
        std::vector<int> all(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) all[i] = (int)i;
        recognise_pass(c, g, jobs, all, true, texts, confs);
    }
    for (size_t i = 0; i < jobs.size(); ++i) { jobs[i].text = texts[i]; jobs[i].conf = confs[i]; }
    // second round: adjust_contrast_grey for low-confidence boxes
    std::vector<int> low;
    for (size_t i = 0; i < jobs.size(); ++i)
        if (jobs[i].conf < p.contrast_ths) low.push_back((int)i);
    if (low.empty() || !(p.adjust_contrast > 0)) return;
    auto t0 = clk::now();
    std::vector<CropDesc> ld(low.size());
    for (size_t k = 0; k < low.size(); ++k) ld[k] = jobs[low[k]].d;
    c->crop_desc.ensure(ld.size() * sizeof(CropDesc));
    HIPCHK(hipMemcpyAsync(c->crop_desc.p, ld.data(), ld.size() * sizeof(CropDesc), hipMemcpyHostToDevice, c->stream));
    // adjust_contrast_grey leaves a crop whose contrast is already >= the target untouched: its second prediction would be computed
    // from bit-identical input, equals the first one, and get_text's `pred1[1] > pred2[1] ? pred1 : pred2` picks the same pair either
    // way.  Only the crops that really change are run again.
    std::vector<int> redo;
    std::vector<uint8_t> luts;
    for (int k : crop_contrast_luts(c, (const CropDesc*)c->crop_desc.p, ld, p.adjust_contrast, luts)) {
        jobs[low[k]].d.lut_off = ld[k].lut_off;
        redo.push_back(low[k]);
    }
    if (!redo.empty()) {
        c->crop_luts.ensure(luts.size());
        HIPCHK(hipMemcpyAsync(c->crop_luts.p, luts.data(), luts.size(), hipMemcpyHostToDevice, c->stream));   // `luts` outlives the pass below, which ends synchronised
        std::vector<std::vector<int>> t2;
        std::vector<double> c2;
        recognise_pass(c, g, jobs, redo, false, t2, c2);
        for (size_t k = 0; k < redo.size(); ++k) {
            BoxJob& j = jobs[redo[k]];
            j.d.lut_off = -1;
            if (!(j.conf > c2[k])) { j.text = t2[k]; j.conf = c2[k]; }
        }
    }
    c->times[6] += (float)ms_since(t0);
}

bbocr_result* export_result(int B, const std::vector<BoxJob>& jobs, const std::vector<int>& box_off) {
    bbocr_result* r = (bbocr_result*)calloc(1, sizeof(bbocr_result));
    const size_t nb = jobs.size();
    r->n_images = B;
    r->box_off = (int*)calloc(B + 1, sizeof(int));
    for (int b = 0; b <= B; ++b) r->box_off[b] = box_off[b];
    r->quads = (double*)calloc(std::max<size_t>(1, nb) * 8, sizeof(double));
    r->is_free = (int*)calloc(std::max<size_t>(1, nb), sizeof(int));
    r->text_off = (int*)calloc(nb + 1, sizeof(int));
    r->conf = (double*)calloc(std::max<size_t>(1, nb), sizeof(double));
    size_t nt = 0;
    for (const BoxJob& j : jobs) nt += j.text.size();
    r->text_idx = (int*)calloc(std::max<size_t>(1, nt), sizeof(int));
    size_t o = 0;
    for (size_t i = 0; i < nb; ++i) {
        memcpy(r->quads + i * 8, jobs[i].quad, 64);
        r->is_free[i] = jobs[i].is_free;
        r->conf[i] = jobs[i].conf;
        r->text_off[i] = (int)o;
        for (int v : jobs[i].text) r->text_idx[o++] = v;
    }
    r->text_off[nb] = (int)o;
    return r;
}
