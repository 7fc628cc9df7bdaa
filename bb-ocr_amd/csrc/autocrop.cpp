// Text-region auto-crop of the extractor (enhanced_extractor.py::_auto_crop_text_region), host side: work-buffer layout, the launch
// sequence of autocrop.hip and the box arithmetic on the external components' bounding boxes.
#include "ctx.h"

#include <climits>

// getGaussianKernelBitExact (imgproc/smooth.dispatch.cpp; the x = 1 - n, 3 - n, ... exponents, sigma 0 -> 0.3 ((n - 1) / 2 - 1) + 0.8)
// followed by getGaussianKernelFixedPoint_ED with 8 fraction bits: the left half is rounded (half to even) with the error carried on,
// mirrored, and the centre tap takes what is left of 256.  For n = 3 this is oracle/preprocess.py::gaussian_kernel3_fixed.
void gaussian_taps_fixed(int n, double sigma, int* k) {
    if (sigma <= 0) sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8;
    const double scale2x = -0.125 / (sigma * sigma);
    const int half = (n - 1) / 2;
    std::vector<double> v(half);
    double sum = 0;
    for (int i = 0, x = 1 - n; i < half; ++i, x += 2) {
        v[i] = std::exp((double)(x * x) * scale2x);
        sum += v[i];
    }
    sum = sum * 2 + 1;
    const double mul = 1.0 / sum;
    double err = 0;
    int total = 0;
    for (int i = 0; i < half; ++i) {
        const double adj = v[i] * mul * 256.0 + err;
        const int r = (int)std::nearbyint(adj);
        err = adj - r;
        k[i] = k[n - 1 - i] = r;
        total += r;
    }
    k[half] = 256 - 2 * total;
}

namespace {

struct AcPlan {
    int H, W, WW, cap;
    uint8_t *blur, *clahe, *part, *grad, *flag;
    uint16_t *rbox, *rgau;
    int* label;
    uint32_t* bits[5];
    unsigned int* hist;
    int *thr, *count, *boxes;
};

// one carve of the slot's auto-crop buffer; the labels reuse the row planes and the flags the cue plane (both dead by then).
// any_mask: the components are taken of a mask that no morphology has merged (bbocr_op_autocrop_mask_stage, `components`)
AcPlan ac_plan(bbocr_ctx* c, int H, int W, bool any_mask = false) {
    AcPlan p{};
    p.H = H;
    p.W = W;
    p.WW = (W + 31) / 32;
    const size_t n = (size_t)H * W, nw = (size_t)p.WW * H;
    // every component of the merged mask holds a whole 13 x 5 dilation window (clipped at the edges), so at most n / that many exist;
    // of any mask, 8-connected: no two components share a 2 x 2 cell
    p.cap = any_mask ? (int)(((size_t)(H + 1) / 2) * ((size_t)(W + 1) / 2)) : (int)(n / ((size_t)std::min(W, 7) * std::min(H, 3))) + 1;
    Carve cv;
    const size_t o_blur = cv.add(n), o_clahe = cv.add(n), o_rows = cv.add(4 * n), o_part = cv.add(n), o_grad = cv.add(n);
    size_t o_bits[5];
    for (auto& o : o_bits) o = cv.add(nw * 4);
    const size_t o_hist = cv.add(512 * 4), o_small = cv.add(16), o_boxes = cv.add((size_t)p.cap * 16);
    c->ac_work.ensure(cv.off);
    void* b = c->ac_work.p;
    p.blur = Carve::at<uint8_t>(b, o_blur);
    p.clahe = Carve::at<uint8_t>(b, o_clahe);
    p.rbox = Carve::at<uint16_t>(b, o_rows);
    p.rgau = p.rbox + n;
    p.label = Carve::at<int>(b, o_rows);
    p.part = Carve::at<uint8_t>(b, o_part);
    p.flag = p.part;
    p.grad = Carve::at<uint8_t>(b, o_grad);
    for (int i = 0; i < 5; ++i) p.bits[i] = Carve::at<uint32_t>(b, o_bits[i]);
    p.hist = Carve::at<unsigned int>(b, o_hist);
    p.thr = Carve::at<int>(b, o_small);
    p.count = p.thr + 2;
    p.boxes = Carve::at<int>(b, o_boxes);
    return p;
}

// the morphology: packed mask bits[0] -> merged mask bits[4]
void ac_enqueue_merge(bbocr_ctx* c, const AcPlan& p) {
    const int H = p.H, W = p.W, WW = p.WW;
    hipStream_t s = c->stream;
    // per variant: CLOSE (rect kernel, 2 iterations folded by OpenCV into (k - 1) * 2 + 1), OPEN 3x3, dilate 11x3.  Rect erosions and
    // dilations with the in-bounds-only border compose into one rect each: dilate K2, erode K2 + 3x3, and -- shared by both variants,
    // dilation distributing over OR -- dilate 3x3 + 11x3 = 13x5 once on the OR of the two.  Radii (x, y):
    //   9x3 -> 17x5: dilate (8, 2), erode 19x7 (9, 3);   15x5 -> 29x9: dilate (14, 4), erode 31x11 (15, 5);   final dilate (6, 2)
    uint32_t *m = p.bits[0], *t = p.bits[1], *a = p.bits[2], *v = p.bits[3], *out = p.bits[4];
    HIPCHK(launch_ac_rect(m, t, a, H, W, WW, 8, 2, 0, nullptr, s));
    HIPCHK(launch_ac_rect(a, t, out, H, W, WW, 9, 3, 1, nullptr, s));     // variant 1 -> out (scratch until the last step)
    HIPCHK(launch_ac_rect(m, t, a, H, W, WW, 14, 4, 0, nullptr, s));
    HIPCHK(launch_ac_rect(a, t, v, H, W, WW, 15, 5, 1, out, s));                               // variant 2 | variant 1 -> v
    HIPCHK(launch_ac_rect(v, t, out, H, W, WW, 6, 2, 0, nullptr, s));
}

// the external components of a packed mask: numbered in p.label, counted in p.count, their raw boxes in p.boxes
void ac_enqueue_components(bbocr_ctx* c, const AcPlan& p, const uint32_t* mask) {
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(p.flag, 0, (size_t)p.H * p.W, s));
    HIPCHK(hipMemsetAsync(p.count, 0, 4, s));
    HIPCHK(launch_ac_components(mask, p.H, p.W, p.WW, p.label, p.flag, p.count, p.cap, p.boxes, s));
}

// enqueues the chain up to `last`: 0 = CLAHE output, 1 = composite mask (bits[0]), 2 = merged mask (bits[4]), 3 = external components
void ac_enqueue(bbocr_ctx* c, const AcPlan& p, const uint8_t* src, size_t pitch, int channels, int last) {
    const int H = p.H, W = p.W, WW = p.WW;
    const size_t n = (size_t)H * W;
    hipStream_t s = c->stream;
    HIPCHK(launch_ac_gray_blur(src, H, W, pitch, channels, p.blur, s));
    pp_clahe(c, p.blur, H, W, pp_fold_lut(c, n, 0.0, 0.0), p.clahe, 2.0);
    if (last == 0) return;
    AcTaps taps;
    gaussian_taps_fixed(AC_GAU, 0.0, taps.k);
    HIPCHK(hipMemsetAsync(p.hist, 0, 512 * 4, s));
    HIPCHK(launch_ac_cues(p.clahe, H, W, taps, p.rbox, p.rgau, p.part, p.grad, p.hist, p.thr, s));
    HIPCHK(launch_ac_pack(p.clahe, p.part, p.grad, p.thr, H, W, WW, p.bits[0], s));
    if (last == 1) return;
    ac_enqueue_merge(c, p);
    if (last == 2) return;
    ac_enqueue_components(c, p, p.bits[4]);
}

// waits for the queued work; the raw boxes (x0, y0, x1, y1 inclusive) of the external components, in the device's enumeration order
std::vector<int> ac_read_raw_boxes(bbocr_ctx* ctx, const AcPlan& p) {
    int count = 0;
    HIPCHK(hipMemcpyAsync(&count, p.count, 4, hipMemcpyDeviceToHost, ctx->stream));
    slot_sync(ctx, ctx->stream);
    if (count > p.cap) fail(BBOCR_ERR_OVERFLOW, "more external components than the bound allows");
    std::vector<int> raw((size_t)count * 4);
    if (count) {
        HIPCHK(hipMemcpyAsync(raw.data(), p.boxes, raw.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
    }
    return raw;
}

void ac_check_args(const void* src, int H, int W, long long pitch, int channels) {
    if (channels != 1 && channels != 3) fail(BBOCR_ERR_ARG, "channels must be 1 or 3");
    check_page({src, H, W, pitch, channels == 1 ? PAGE_GRAY : PAGE_BGR});
    // clahe.cpp pads both axes to the 8x8 grid when either does not divide; the padding must stay inside the image (preprocess.cpp::pp_clahe)
    const bool pad = (H % 8) || (W % 8);
    if (pad && ((8 - H % 8) >= H || (8 - W % 8) >= W)) fail(BBOCR_ERR_ARG, "image smaller than the CLAHE tile grid");
}

}  // namespace

extern "C" {

int bbocr_auto_crop(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int channels, int margin, int box[4], int* found,
                    int* comp_boxes, int max_comps, int* n_comps) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        ac_check_args(dev_src, H, W, pitch, channels);
        if (!box || !found || !n_comps || margin < 0 || max_comps < 0 || (max_comps > 0 && !comp_boxes)) fail(BBOCR_ERR_ARG, "bad arguments");
        const AcPlan p = ac_plan(ctx, H, W);
        ac_enqueue(ctx, p, dev_src, (size_t)pitch, channels, 3);
        const std::vector<int> raw = ac_read_raw_boxes(ctx, p);
        const int count = (int)(raw.size() / 4);
        // boundingRect + the reference's area filter, in double like the Python floats (enhanced_extractor.py:287-297)
        const double img_area = (double)H * (double)W;
        std::vector<std::array<int, 4>> kept;
        for (int k = 0; k < count; ++k) {
            const int* r = &raw[(size_t)k * 4];
            const int bw = r[2] - r[0] + 1, bh = r[3] - r[1] + 1;
            const double area = (double)bw * (double)bh;
            if (area < 0.0001 * img_area || area > 0.10 * img_area) continue;
            kept.push_back({r[0], r[1], bw, bh});
        }
        std::sort(kept.begin(), kept.end(), [](const std::array<int, 4>& a, const std::array<int, 4>& b) {
            return std::make_tuple(a[1], a[0], a[2], a[3]) < std::make_tuple(b[1], b[0], b[2], b[3]);
        });
        *n_comps = (int)kept.size();
        for (int k = 0; k < std::min(max_comps, (int)kept.size()); ++k)
            for (int q = 0; q < 4; ++q) comp_boxes[4 * k + q] = kept[k][q];
        *found = 0;
        box[0] = box[1] = box[2] = box[3] = 0;
        if (kept.empty()) return;      // the fallback over the raw mask's contours never adds a box (:298-310)
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
        for (const auto& b : kept) {
            x0 = std::min(x0, b[0]);
            y0 = std::min(y0, b[1]);
            x1 = std::max(x1, b[0] + b[2]);
            y1 = std::max(y1, b[1] + b[3]);
        }
        if ((double)(x1 - x0) * (double)(y1 - y0) < 0.12 * img_area) {   // too small a union: inflate by 3 % of the longer side
            const int pad = (int)(0.03 * (double)std::max(W, H));
            x0 = std::max(0, x0 - pad);
            y0 = std::max(0, y0 - pad);
            x1 = std::min(W, x1 + pad);
            y1 = std::min(H, y1 + pad);
        }
        x0 = std::max(0, x0 - margin);
        y0 = std::max(0, y0 - margin);
        x1 = std::min(W, x1 + margin);
        y1 = std::min(H, y1 + margin);
        if (x1 <= x0 || y1 <= y0) return;
        box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
        *found = 1;
    });
}

int bbocr_op_autocrop_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int channels, uint8_t* dev_dst) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        ac_check_args(dev_src, H, W, pitch, channels);
        if (!dev_dst || stage < 0 || stage > 3) fail(BBOCR_ERR_ARG, "bad arguments");
        const AcPlan p = ac_plan(ctx, H, W);
        ac_enqueue(ctx, p, dev_src, (size_t)pitch, channels, stage);
        if (stage == 0) HIPCHK(hipMemcpyAsync(dev_dst, p.clahe, (size_t)H * W, hipMemcpyDeviceToDevice, ctx->stream));
        else HIPCHK(launch_ac_unpack(stage == 1 ? p.bits[0] : p.bits[4], stage == 3 ? p.label : nullptr, H, W, p.WW, dev_dst, ctx->stream));
        int count = 0;
        if (stage == 3) HIPCHK(hipMemcpyAsync(&count, p.count, 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        if (count > p.cap) fail(BBOCR_ERR_OVERFLOW, "more external components than the bound allows");
    });
}

int bbocr_op_autocrop_mask_stage(bbocr_ctx* ctx, int mode, const uint8_t* dev_mask, int H, int W, long long pitch, uint8_t* dev_dst, int* boxes,
                                 int max_boxes, int* n_boxes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        check_page({dev_mask, H, W, pitch, PAGE_GRAY});
        if (!dev_dst || !n_boxes || max_boxes < 0 || (max_boxes > 0 && !boxes)) fail(BBOCR_ERR_ARG, "bad arguments");
        if (mode < BBOCR_AC_MASK_MERGED || mode > BBOCR_AC_MASK_COMPONENTS) fail(BBOCR_ERR_ARG, "unknown mode");
        const AcPlan p = ac_plan(ctx, H, W, mode == BBOCR_AC_MASK_COMPONENTS);
        HIPCHK(launch_ac_pack_mask(dev_mask, (size_t)pitch, H, W, p.WW, p.bits[0], ctx->stream));
        if (mode != BBOCR_AC_MASK_COMPONENTS) ac_enqueue_merge(ctx, p);
        const uint32_t* mask = mode == BBOCR_AC_MASK_COMPONENTS ? p.bits[0] : p.bits[4];
        if (mode != BBOCR_AC_MASK_MERGED) ac_enqueue_components(ctx, p, mask);
        HIPCHK(launch_ac_unpack(mask, mode == BBOCR_AC_MASK_MERGED ? nullptr : p.label, H, W, p.WW, dev_dst, ctx->stream));
        *n_boxes = 0;
        if (mode == BBOCR_AC_MASK_MERGED) {
            slot_sync(ctx, ctx->stream);
            return;
        }
        const std::vector<int> raw = ac_read_raw_boxes(ctx, p);
        *n_boxes = (int)(raw.size() / 4);
        for (int k = 0; k < std::min(max_boxes, *n_boxes); ++k) {
            const int* r = &raw[(size_t)k * 4];
            boxes[4 * k + 0] = r[0];
            boxes[4 * k + 1] = r[1];
            boxes[4 * k + 2] = r[2] - r[0] + 1;
            boxes[4 * k + 3] = r[3] - r[1] + 1;
        }
    });
}

}  // extern "C"
