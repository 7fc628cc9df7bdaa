// OCR-input thumbnail + JPEG round trip (enhanced_extractor.py:486-512), host side: Pillow's thumbnail geometry (preserve_aspect_ratio,
// resize's reducing_gap rule), the resample coefficient tables (precompute_coeffs + normalize_coeffs_8bpc), libjpeg's quality-scaled
// quantisation tables, and the launch sequence of thumb.hip.  Also the resize with a fractional source box that Image.thumbnail runs after
// a JPEG draft (bbocr_thumbnail_box: the trace previews, enhanced_extractor.py:184-199), on the same kernels.
#include "ctx.h"

#include <cmath>

namespace {

constexpr int kStdLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40, 57,
                             69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                             81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr int kStdChrom[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                               99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jcparam.c::jpeg_set_quality(quality, force_baseline = TRUE)
void jpeg_qtables(int quality, unsigned short* out) {
    quality = std::min(std::max(quality, 1), 100);
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const long v = ((long)(t ? kStdChrom : kStdLum)[i] * scale + 50) / 100;
            out[t * 64 + i] = (unsigned short)std::min(std::max(v, 1L), 255L);
        }
}

// Image.thumbnail's preserve_aspect_ratio (Python floats are doubles; min() keeps the first of equal keys)
void thumb_dims(int H, int W, int max_dim, int* oh, int* ow) {
    *oh = H;
    *ow = W;
    if (max_dim >= W && max_dim >= H) return;
    const double aspect = (double)W / (double)H;
    const double x = max_dim, y = max_dim;
    if (x / y >= aspect) {
        const double n = y * aspect, f = std::floor(n), c = std::ceil(n);
        const double r = std::fabs(aspect - c / y) < std::fabs(aspect - f / y) ? c : f;
        *ow = std::max((int)r, 1);
        *oh = max_dim;
    } else {
        const double n = x / aspect, f = std::floor(n), c = std::ceil(n);
        auto key = [&](double v) { return v == 0 ? 0.0 : std::fabs(aspect - x / v); };
        const double r = key(c) < key(f) ? c : f;
        *oh = std::max((int)r, 1);
        *ow = max_dim;
    }
}

struct ThPlan {
    int oh, ow, fx, fy, rh, rw;   // output, reduce factors, reduced size
    float box[4];                 // the resample box in the reduced image (x0, y0, x1, y1)
};

// Image.resize((ow, oh), BICUBIC, reducing_gap=2.0) of the whole image: reduce factors int(size / out / 2) or 1, _get_safe_box of
// the whole box is the whole image, the box handed on is (0, 0, W / fx, H / fy) as C floats
ThPlan thumb_plan(int H, int W, int max_dim) {
    ThPlan p{};
    thumb_dims(H, W, max_dim, &p.oh, &p.ow);
    p.fx = std::max((int)((double)W / p.ow / 2.0), 1);
    p.fy = std::max((int)((double)H / p.oh / 2.0), 1);
    p.rw = (W + p.fx - 1) / p.fx;
    p.rh = (H + p.fy - 1) / p.fy;
    p.box[0] = p.box[1] = 0.0f;
    p.box[2] = (float)((double)W / p.fx);
    p.box[3] = (float)((double)H / p.fy);
    return p;
}

// Image.resize((ow, oh), BICUBIC, box=(0, 0, bw, bh), reducing_gap=2.0) for a box that ends inside the last pixel (W - 1 < bw <= W, the
// same down): what Image.thumbnail does after a JPEG draft, whose box is the original size over the draft scale.  The reduce factors
// come from the box, _get_safe_box of such a box is the whole image (the filter's support reaches past the last pixel whenever a factor
// exceeds 1), and the box handed on is (0, 0, bw / fx, bh / fy) as C floats.  false: the box is not of that kind.
bool resize_plan(int H, int W, int oh, int ow, double bw, double bh, ThPlan* out) {
    if (!(bw > (double)W - 1.0 && bw <= (double)W && bh > (double)H - 1.0 && bh <= (double)H)) return false;
    ThPlan p{};
    p.oh = oh;
    p.ow = ow;
    p.fx = std::max((int)(bw / ow / 2.0), 1);
    p.fy = std::max((int)(bh / oh / 2.0), 1);
    p.rw = (W + p.fx - 1) / p.fx;
    p.rh = (H + p.fy - 1) / p.fy;
    p.box[0] = p.box[1] = 0.0f;
    p.box[2] = (float)(bw / p.fx);
    p.box[3] = (float)(bh / p.fy);
    *out = p;
    return true;
}

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Resample.c::precompute_coeffs + normalize_coeffs_8bpc; returns ksize.  bounds [out][2] = (xmin, count), kk [out][ksize]
int resample_coeffs(int in_size, float in0, float in1, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
    const double scale = (double)(in1 - in0) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale, ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << TH_PRECISION_BITS)) : (int)(0.5 + v * (1 << TH_PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// The device coefficient tables of one plan, kept while (in, out, box) repeats (one page size per batch is the rule): int blocks
// bounds_h | kk_h | bounds_v | kk_v.  Returns the four pointers, the two kernel sizes and the source rows the vertical pass reads
// (ImagingResampleInner's ybox_first .. ybox_last: the horizontal pass covers these only).
struct ThCoef { const int *bh, *kh, *bv, *kv; int ksh, ksv, y0, y1; };
ThCoef thumb_coeffs(bbocr_ctx* c, const ThPlan& p) {
    int key[6];
    std::memcpy(&key[0], &p.box[2], 4);
    std::memcpy(&key[1], &p.box[3], 4);
    key[2] = p.rw; key[3] = p.rh; key[4] = p.ow; key[5] = p.oh;
    const bool hit = c->th_coef.p && std::memcmp(key, c->th_coef_key, sizeof key) == 0;
    ThCoef r{};
    if (!hit) {
        std::vector<int> bh, kh, bv, kv;
        const int ksh = resample_coeffs(p.rw, p.box[0], p.box[2], p.ow, bh, kh);
        const int ksv = resample_coeffs(p.rh, p.box[1], p.box[3], p.oh, bv, kv);
        std::vector<int> all;
        all.reserve(bh.size() + kh.size() + bv.size() + kv.size());
        for (auto* v : {&bh, &kh, &bv, &kv}) all.insert(all.end(), v->begin(), v->end());
        c->th_coef_key[4] = -1;                               // invalid until the upload below has landed
        slot_sync(c, c->stream);                              // an earlier call may still read the tables about to be replaced
        c->th_coef.ensure(all.size() * 4);
        HIPCHK(hipMemcpyAsync(c->th_coef.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, c->stream));
        slot_sync(c, c->stream);                              // the host vector must outlive the copy
        c->th_coef_ks[0] = ksh;
        c->th_coef_ks[1] = ksv;
        c->th_coef_rows[0] = bv[0];
        c->th_coef_rows[1] = bv[2 * p.oh - 2] + bv[2 * p.oh - 1];
        std::memcpy(c->th_coef_key, key, sizeof key);
    }
    const int* b = (const int*)c->th_coef.p;
    r.ksh = c->th_coef_ks[0];
    r.ksv = c->th_coef_ks[1];
    r.y0 = c->th_coef_rows[0];
    r.y1 = c->th_coef_rows[1];
    r.bh = b;
    r.kh = r.bh + 2 * p.ow;
    r.bv = r.kh + (size_t)p.ow * r.ksh;
    r.kv = r.bv + 2 * p.oh;
    return r;
}

// ImagingResampleInner of Pillow 12 runs the vertical pass first on an image more than 100 times taller than wide (pinned against the
// installed Pillow by tests/test_thumbnail_cpu.py); a pass that is not needed (size and box unchanged) has the identity weights 1 << 22,
// so running it anyway changes no pixel
bool th_vertical_first(const ThPlan& p) { return (long long)p.rh > 100LL * p.rw; }

void th_check(const void* src, int H, int W, long long pitch, int layout, int max_dim, int quality) {
    check_page({src, H, W, pitch, layout});
    if (max_dim < 1) fail(BBOCR_ERR_ARG, "max_dim must be >= 1");
    if (quality > 100) fail(BBOCR_ERR_ARG, "quality must be <= 100");
}

// Work buffers of one call, carved from the slot's arena (the call holds the slot; readtext calls size the arena afresh)
struct ThWork {
    uint8_t *rgb, *reduced, *hpass, *resized, *yp, *cbp, *crp;
};
ThWork th_work(bbocr_ctx* c, int H, int W, int layout, const ThPlan& p, int rows, bool thumb, int jh, int jw) {
    const int C = layout == PAGE_GRAY ? 1 : 3;
    const bool ycc = layout == PAGE_YCC4 || layout == PAGE_YCC3;
    const size_t hp = (size_t)((jh + 15) / 16) * 16, wp = (size_t)((jw + 15) / 16) * 16;
    Carve cv;
    const size_t o_rgb = cv.add(ycc && thumb ? (size_t)H * W * 3 : 0);
    const size_t o_red = cv.add(thumb && (p.fx > 1 || p.fy > 1) ? (size_t)p.rh * p.rw * C : 0);
    const size_t o_h = cv.add(thumb ? std::max((size_t)rows * p.ow, (size_t)p.oh * p.rw) * C : 0);
    const size_t o_res = cv.add(thumb ? (size_t)p.oh * p.ow * C : 0);
    const size_t o_y = cv.add(hp * wp), o_cb = cv.add(hp * wp / 4), o_cr = cv.add(hp * wp / 4);
    c->arena.buf.ensure(cv.off);
    auto at = [b = c->arena.buf.p](size_t o) { return Carve::at<uint8_t>(b, o); };
    return ThWork{at(o_rgb), at(o_red), at(o_h), at(o_res), at(o_y), at(o_cb), at(o_cr)};
}

// Enqueues the JPEG round trip of an RGB (C 3) or gray (C 1) page; ycc != null: the upsampled triple instead of rgb / gray
void th_jpeg(bbocr_ctx* c, const ThWork& w, const uint8_t* src, size_t pitch, int C, int H, int W, int quality, uint8_t* rgb, uint8_t* gray,
             uint8_t* ycc) {
    ThQuant q;
    jpeg_qtables(quality, &q.q[0][0]);
    const int wp = (W + 15) / 16 * 16;
    HIPCHK(launch_th_jpeg(src, pitch, C, H, W, q, w.yp, wp, w.cbp, w.crp, c->stream));
    HIPCHK(launch_th_upsample(w.yp, wp, w.cbp, w.crp, H, W, C == 1 ? 1 : 0, rgb, gray, ycc, c->stream));
}

// Enqueues reduce + resample of the page into w.resized (C channels, tight rows); returns C
int th_resize(bbocr_ctx* c, const ThWork& w, const uint8_t* src, size_t pitch, int layout, int H, int W, const ThPlan& p, const ThCoef& k) {
    const int C = layout == PAGE_GRAY ? 1 : 3;
    if (layout == PAGE_YCC4 || layout == PAGE_YCC3) {
        HIPCHK(launch_th_direct(src, pitch, layout, H, W, w.rgb, nullptr, c->stream));
        src = w.rgb;
        pitch = (size_t)W * 3;
        layout = PAGE_RGB;
    }
    if (p.fx > 1 || p.fy > 1) {
        HIPCHK(launch_th_reduce(src, pitch, layout, H, W, p.fx, p.fy, w.reduced, p.rh, p.rw, C, c->stream));
        src = w.reduced;
        pitch = (size_t)p.rw * C;
        layout = C == 1 ? PAGE_GRAY : PAGE_RGB;
    }
    if (th_vertical_first(p)) {                                  // the vertical pass runs on the source bytes (per channel, any order)
        HIPCHK(launch_th_resample_v(src, pitch, 0, p.rw * C, p.oh, k.bv, k.kv, k.ksv, w.hpass, (size_t)p.rw * C, c->stream));
        HIPCHK(launch_th_resample_h(w.hpass, (size_t)p.rw * C, layout, 0, p.oh, p.ow, C, k.bh, k.kh, k.ksh, w.resized, c->stream));
        return C;
    }
    HIPCHK(launch_th_resample_h(src, pitch, layout, k.y0, k.y1 - k.y0, p.ow, C, k.bh, k.kh, k.ksh, w.hpass, c->stream));
    HIPCHK(launch_th_resample_v(w.hpass, (size_t)p.ow * C, k.y0, p.ow * C, p.oh, k.bv, k.kv, k.ksv, w.resized, (size_t)p.ow * C, c->stream));
    return C;
}

}  // namespace

extern "C" {

int bbocr_thumbnail_dims(int H, int W, int max_dim, int* out_h, int* out_w) {
    if (H < 1 || W < 1 || max_dim < 1 || !out_h || !out_w) return BBOCR_ERR_ARG;
    thumb_dims(H, W, max_dim, out_h, out_w);
    return BBOCR_OK;
}

int bbocr_host_thumbnail_plan(int H, int W, int max_dim, int* out_h, int* out_w, int factors[2], int reduce_box[4], float resize_box[4]) {
    if (H < 1 || W < 1 || max_dim < 1 || !out_h || !out_w || !factors || !reduce_box || !resize_box) return BBOCR_ERR_ARG;
    const ThPlan p = thumb_plan(H, W, max_dim);
    *out_h = p.oh;
    *out_w = p.ow;
    factors[0] = p.fx;
    factors[1] = p.fy;
    reduce_box[0] = reduce_box[1] = 0;
    reduce_box[2] = W;
    reduce_box[3] = H;
    for (int i = 0; i < 4; ++i) resize_box[i] = p.box[i];
    return BBOCR_OK;
}

int bbocr_host_resample_coeffs(int in_size, float in0, float in1, int out_size, int* bounds, int* coeffs, int max_ksize, int* ksize) {
    if (in_size < 1 || out_size < 1 || !ksize || !(in1 > in0)) return BBOCR_ERR_ARG;
    std::vector<int> b, k;
    const int ks = resample_coeffs(in_size, in0, in1, out_size, b, k);
    *ksize = ks;
    if (!bounds && !coeffs) return BBOCR_OK;                     // size query
    if (!bounds || !coeffs || max_ksize < ks) return BBOCR_ERR_ARG;
    std::memcpy(bounds, b.data(), b.size() * 4);
    for (int i = 0; i < out_size; ++i) std::memcpy(coeffs + (size_t)i * max_ksize, k.data() + (size_t)i * ks, (size_t)ks * 4);
    return BBOCR_OK;
}

int bbocr_host_jpeg_qtables(int quality, uint16_t* out) {
    if (!out || quality < 1 || quality > 100) return BBOCR_ERR_ARG;
    jpeg_qtables(quality, out);
    return BBOCR_OK;
}

int bbocr_ocr_thumbnail(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int max_dim, int quality, uint8_t* dev_rgb,
                        uint8_t* dev_gray, int* out_h, int* out_w) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        th_check(dev_src, H, W, pitch, layout, max_dim, quality);
        if (!dev_rgb || !dev_gray || !out_h || !out_w) fail(BBOCR_ERR_ARG, "null pointer");
        const ThPlan p = thumb_plan(H, W, max_dim);
        *out_h = p.oh;
        *out_w = p.ow;
        const bool thumb = std::max(H, W) > max_dim;
        if (!thumb) {                                            // no thumbnail, no JPEG: the page as easyocr reads it
            HIPCHK(launch_th_direct(dev_src, (size_t)pitch, layout, H, W, dev_rgb, dev_gray, ctx->stream));
            slot_sync(ctx, ctx->stream);
            return;
        }
        const ThCoef k = thumb_coeffs(ctx, p);
        const ThWork w = th_work(ctx, H, W, layout, p, k.y1 - k.y0, true, p.oh, p.ow);
        const int C = th_resize(ctx, w, dev_src, (size_t)pitch, layout, H, W, p, k);
        if (quality > 0) th_jpeg(ctx, w, w.resized, (size_t)p.ow * C, C, p.oh, p.ow, quality, dev_rgb, dev_gray, nullptr);
        else HIPCHK(launch_th_direct(w.resized, (size_t)p.ow * C, C == 1 ? PAGE_GRAY : PAGE_RGB, p.oh, p.ow, dev_rgb, dev_gray, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_host_resize_plan(int H, int W, int out_h, int out_w, double box_w, double box_h, int factors[2], float resize_box[4]) {
    if (H < 1 || W < 1 || out_h < 1 || out_w < 1 || !factors || !resize_box) return BBOCR_ERR_ARG;
    ThPlan p;
    if (!resize_plan(H, W, out_h, out_w, box_w, box_h, &p)) return BBOCR_ERR_ARG;
    factors[0] = p.fx;
    factors[1] = p.fy;
    for (int i = 0; i < 4; ++i) resize_box[i] = p.box[i];
    return BBOCR_OK;
}

int bbocr_thumbnail_box(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int out_h, int out_w, double box_w,
                        double box_h, uint8_t* dev_dst) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        check_page({dev_src, H, W, pitch, layout});
        if (!dev_dst || out_h < 1 || out_w < 1) fail(BBOCR_ERR_ARG, "bad arguments");
        ThPlan p;
        if (!resize_plan(H, W, out_h, out_w, box_w, box_h, &p)) fail(BBOCR_ERR_ARG, "the box must start at (0, 0) and end inside the last pixel");
        const ThCoef k = thumb_coeffs(ctx, p);
        const ThWork w = th_work(ctx, H, W, layout, p, k.y1 - k.y0, true, 1, 1);
        const int C = th_resize(ctx, w, dev_src, (size_t)pitch, layout, H, W, p, k);
        HIPCHK(hipMemcpyAsync(dev_dst, w.resized, (size_t)p.oh * p.ow * C, hipMemcpyDeviceToDevice, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_thumbnail_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int max_dim, int quality,
                             uint8_t* dev_dst, uint8_t* dev_gray, int* out_h, int* out_w) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        th_check(dev_src, H, W, pitch, layout, max_dim, quality);
        if (!dev_dst || !out_h || !out_w || stage < 0 || stage > 2 || (stage == 1 && !dev_gray)) fail(BBOCR_ERR_ARG, "bad arguments");
        if (stage > 0 && (quality < 1 || (layout != PAGE_GRAY && layout != PAGE_RGB))) fail(BBOCR_ERR_ARG, "stages 1 and 2 take a gray or RGB page and a quality");
        if (stage == 0) {
            const ThPlan p = thumb_plan(H, W, max_dim);
            *out_h = p.oh;
            *out_w = p.ow;
            if (std::max(H, W) <= max_dim) {
                HIPCHK(launch_th_direct(dev_src, (size_t)pitch, layout, H, W, dev_dst, nullptr, ctx->stream));
            } else {
                const ThCoef k = thumb_coeffs(ctx, p);
                const ThWork w = th_work(ctx, H, W, layout, p, k.y1 - k.y0, true, 1, 1);
                const int C = th_resize(ctx, w, dev_src, (size_t)pitch, layout, H, W, p, k);
                HIPCHK(launch_th_direct(w.resized, (size_t)p.ow * C, C == 1 ? PAGE_GRAY : PAGE_RGB, p.oh, p.ow, dev_dst, nullptr, ctx->stream));
            }
        } else {
            *out_h = H;
            *out_w = W;
            const ThPlan p{};
            const ThWork w = th_work(ctx, H, W, layout, p, 0, false, H, W);
            const int C = layout == PAGE_GRAY ? 1 : 3;
            th_jpeg(ctx, w, dev_src, (size_t)pitch, C, H, W, quality, stage == 1 ? dev_dst : nullptr, stage == 1 ? dev_gray : nullptr,
                    stage == 2 ? dev_dst : nullptr);
        }
        slot_sync(ctx, ctx->stream);
    });
}

}  // extern "C"
