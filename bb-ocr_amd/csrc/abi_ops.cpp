// C ABI of libbbocr (include/bbocr.h), stage-level entry points: single kernels and host stages exposed so that the parity tests can pin each one.
#include "ctx.h"

// bbocr_op_crops / bbocr_op_crops_pages inside a call slot: the boxes of n pages (page k: hori [hori_off[k], hori_off[k+1]), free_q likewise)
// planned as recognize_impl plans them and cropped by one set of launches into the bucket tensor [crops][64][imgW], page after page
static void op_crops(bbocr_ctx* ctx, const GrayPages& g, int n, const int* hori, const int* hori_off, const double* free_q, const int* free_off, int imgW,
                     float contrast, uint16_t* dev_out, int* n_out, int mode) {
    if (!dev_out || !n_out || imgW < 64 || (imgW & 63) || mode < 0 || mode > 4) fail(BBOCR_ERR_ARG, "bad crop arguments");
    std::vector<BoxJob> jobs;
    auto take = [&](BoxJob& j) {
        if (mode == 0) {                       // per-box branch: the boxes whose own padded width is imgW
            if (j.d.imgW == imgW) jobs.push_back(j);
            return;
        }
        j.d.imgW = imgW;                       // batched branch (rotation_info): forced width, np.rot90(crop, mode - 1)
        j.d.rot = mode - 1;
        if (j.d.rot & 1) std::swap(j.d.rw, j.d.rh);
        crop_refit_fw(j.d);
        jobs.push_back(j);
    };
    for (int k = 0; k < n; ++k) {
        for (int i = hori_off[k]; i < hori_off[k + 1]; ++i) {
            BoxJob j;
            std::array<int, 4> b;
            memcpy(b.data(), hori + (size_t)i * 4, 16);
            if (plan_horizontal(b, k, g.h(k), g.w(k), j)) take(j);
        }
        for (int i = free_off[k]; i < free_off[k + 1]; ++i) {
            BoxJob j;
            std::array<double, 8> f;
            memcpy(f.data(), free_q + (size_t)i * 8, 64);
            if (plan_free(f, k, j)) take(j);
        }
    }
    *n_out = (int)jobs.size();
    if (jobs.empty()) return;
    size_t a_total = 0, w_total = 0;
    rec_layout_scratch(jobs, 0, a_total, w_total);
    bool any_warp = false, any_tall = false;
    std::vector<CropDesc> descs;
    for (size_t i = 0; i < jobs.size(); ++i) {
        CropDesc& d = jobs[i].d;
        d.slot = (int)i;                       // row of the bucket tensor [n, 64, imgW]
        any_warp |= d.warp != 0;
        any_tall |= !(d.fw == d.rw && d.rh == 64);
        descs.push_back(d);
    }
    ctx->crop_scratch.ensure(std::max<size_t>(a_total, 16));
    ctx->crop_hscratch.ensure(std::max<size_t>(a_total, 16));
    ctx->crop_wscratch.ensure(std::max<size_t>(w_total, 16));
    ctx->crop_desc.ensure(descs.size() * sizeof(CropDesc));
    ctx->crop_luts.ensure(descs.size() * 256);
    HIPCHK(hipMemcpyAsync(ctx->crop_desc.p, descs.data(), descs.size() * sizeof(CropDesc), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_crops(g.gray, g.H, g.W, (const CropDesc*)ctx->crop_desc.p, 0, (int)descs.size(), imgW, any_warp, any_tall,
                        (uint8_t*)ctx->crop_wscratch.p, (uint8_t*)ctx->crop_scratch.p, (uint8_t*)ctx->crop_hscratch.p,
                        (const uint8_t*)ctx->crop_luts.p, dev_out, 1, ctx->stream, 0, 0, 0, g.tab_dev));
    if (contrast > 0) {
        std::vector<uint8_t> luts;       // a crop whose contrast is high enough stays as it is (lut_off -1), as in recognize_impl's retry
        (void)crop_contrast_luts(ctx, (const CropDesc*)ctx->crop_desc.p, descs, (double)contrast, luts);
        if (!luts.empty()) HIPCHK(hipMemcpyAsync(ctx->crop_luts.p, luts.data(), luts.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->crop_desc.p, descs.data(), descs.size() * sizeof(CropDesc), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(launch_crops(g.gray, g.H, g.W, (const CropDesc*)ctx->crop_desc.p, 0, (int)descs.size(), imgW, any_warp, any_tall,
                        (uint8_t*)ctx->crop_wscratch.p, (uint8_t*)ctx->crop_scratch.p, (uint8_t*)ctx->crop_hscratch.p,
                        (const uint8_t*)ctx->crop_luts.p, dev_out, 2, ctx->stream, 0, 0, rec_mode(ctx), g.tab_dev));
    slot_sync(ctx, ctx->stream);
}

extern "C" {

int bbocr_op_preprocess_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, uint8_t* dev_dst, int dh, int dw, double param) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_src || !dev_dst || H <= 0 || W <= 0 || dh <= 0 || dw <= 0) fail(BBOCR_ERR_ARG, "bad arguments");
        if (stage != 0 && (dh != H || dw != W)) fail(BBOCR_ERR_ARG, "only stage 0 changes the size");
        const size_t n = (size_t)H * W;
        if (stage == 0) {
            pp_resize(ctx, dev_src, H, W, dev_dst, dh, dw);
        } else if (stage == 1) {
            pp_gauss(ctx, dev_src, H, W, dev_dst, param);
        } else if (stage == 2 || stage == 3) {
            // pointwise PIL enhancers: the chain folds them into CLAHE's input LUT; stand-alone they are one lookup pass
            if (stage == 2) {
                ctx->pp_a.ensure(n);
                // mean of the input: the 3x3 smoothing kernel with taps (0, 256, 0) is the identity and sums its output
                pp_gauss(ctx, dev_src, H, W, (uint8_t*)ctx->pp_a.p, 0.0);
            }
            HIPCHK(launch_pp_lut(dev_src, dev_dst, pp_fold_lut(ctx, n, stage == 2 ? param : 0.0, stage == 3 ? param : 0.0), n, ctx->stream));
        } else if (stage == 4) {
            pp_clahe(ctx, dev_src, H, W, pp_fold_lut(ctx, n, 0.0, 0.0), dev_dst, param);
        } else if (stage == 5) {
            ctx->pp_b.ensure(n);
            ctx->pp_c.ensure(n);
            pp_unsharp(ctx, dev_src, H, W, dev_dst, (uint8_t*)ctx->pp_b.p, (uint8_t*)ctx->pp_c.p, (float)param, 30, 3);
        } else if (stage == 7) {
            ctx->pp_b.ensure(n);
            ctx->pp_c.ensure(n);
            pp_unsharp(ctx, dev_src, H, W, dev_dst, (uint8_t*)ctx->pp_b.p, (uint8_t*)ctx->pp_c.p, 1.0f, (int)param, 3);
        } else if (stage == 6) {
            // cv2.cvtColor(BGR2GRAY) on an interleaved 3-channel plane [H,W,3] (the gray plane reformat_input derives from arrays)
            HIPCHK(launch_gray(dev_src, dev_dst, n, ctx->stream));
        } else {
            fail(BBOCR_ERR_ARG, "unknown pre-processing stage");
        }
        slot_sync(ctx, ctx->stream);                            // every stage only enqueues
    });
}

// Which kernel a stage of bbocr_op_preprocess_stage takes for a plane of this size at pointers with these low two bits: the launchers' own
// decision functions (preproc.hip), so no device and no context.  The stage's scratch planes are the library's allocations (aligned).
static bool pp_route_args(int H, int W, int a, int b) { return H > 0 && W > 0 && a >= 0 && a <= 3 && b >= 0 && b <= 3; }
int bbocr_host_pp_resize_route(int H, int W, int dh, int dw) {
    if (H <= 0 || W <= 0 || dh <= 0 || dw <= 0) return BBOCR_ERR_ARG;
    return (int)pp_resize_route(H, W, dh, dw);
}
int bbocr_host_pp_resize_dword_rows(int dw, int dst_bits) {
    if (dw <= 0 || dst_bits < 0 || dst_bits > 3) return BBOCR_ERR_ARG;
    return pp_resize_dword_rows(dw, (unsigned)dst_bits) ? 1 : 0;
}
int bbocr_host_pp_gauss_route(int H, int W, int src_bits, int dst_bits) {
    if (!pp_route_args(H, W, src_bits, dst_bits)) return BBOCR_ERR_ARG;
    return (int)pp_gauss_route(H, W, (unsigned)src_bits, (unsigned)dst_bits);
}
int bbocr_host_pp_clahe_hist_route(int H, int W, int src_bits) {
    int th = 0, tw = 0;
    if (!pp_route_args(H, W, src_bits, 0) || !pp_clahe_tiles(H, W, &th, &tw)) return BBOCR_ERR_ARG;
    return (int)pp_clahe_hist_route(H, W, (unsigned)src_bits);
}
int bbocr_host_pp_clahe_apply_route(int H, int W, int src_bits, int dst_bits) {
    int th = 0, tw = 0;
    if (!pp_route_args(H, W, src_bits, dst_bits) || !pp_clahe_tiles(H, W, &th, &tw)) return BBOCR_ERR_ARG;
    return (int)pp_clahe_apply_route(H, W, th, (unsigned)src_bits, (unsigned)dst_bits);
}
int bbocr_host_pp_box_route(int H, int W, int r, int src_bits, int dst_bits) {
    if (!pp_route_args(H, W, src_bits, dst_bits) || r < 0) return BBOCR_ERR_ARG;
    return (int)pp_box_route(H, W, r, (unsigned)src_bits, (unsigned)dst_bits);
}
int bbocr_host_pp_unsharp_route(int H, int W, double radius, int src_bits, int dst_bits) {
    if (!pp_route_args(H, W, src_bits, dst_bits) || !(radius > 0)) return BBOCR_ERR_ARG;
    return (int)pp_unsharp_route(H, W, pp_unsharp_box_r((float)radius), (unsigned)src_bits, 0u, (unsigned)dst_bits);
}
int bbocr_host_pp_unsharp_box_radius(double radius) { return radius > 0 ? pp_unsharp_box_r((float)radius) : BBOCR_ERR_ARG; }
static_assert(BBOCR_PP_ROUTE_COUNT == (int)PP_ROUTE_COUNT && BBOCR_PP_GAUSS_BYTE == (int)PP_GAUSS_BYTE && BBOCR_PP_HIST_BYTE == (int)PP_HIST_BYTE &&
                  BBOCR_PP_APPLY_CELL_2 == (int)PP_APPLY_CELL_2 && BBOCR_PP_APPLY_BYTE == (int)PP_APPLY_BYTE && BBOCR_PP_BOX0_X4 == (int)PP_BOX0_X4 &&
                  BBOCR_PP_UNSHARP_FUSED == (int)PP_UNSHARP_FUSED && BBOCR_PP_UNSHARP_PASSES_BYTE == (int)PP_UNSHARP_PASSES_BYTE &&
                  BBOCR_PP_RESIZE_TILED32 == (int)PP_RESIZE_TILED32 && BBOCR_PP_RESIZE_PIXEL == (int)PP_RESIZE_PIXEL,
              "BBOCR_PP_* mirrors PpRoute");

int bbocr_host_cpu_share(void) { return host_cpu_share(); }

int bbocr_host_component_polys(const int* comps, const int* rowext, int n, int w, int h, double ratio, int* polys_out) {
    if (!comps || !rowext || !polys_out || n < 0 || w <= 0 || h <= 0 || !(ratio > 0)) return BBOCR_ERR_ARG;
    try {
        for (int i = 0; i < n; ++i) {
            const int* q = comps + (size_t)i * 7;
            bbocr::Component cc{q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
            float box[4][2];
            bbocr::component_box(cc, rowext + (size_t)cc.row_off * 2, w, h, box);
            bbocr::box_to_poly(box, 1.0 / ratio, 1.0 / ratio, polys_out + (size_t)i * 8);
        }
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

int bbocr_host_group_boxes(const int* polys, int n, const bbocr_params* p, bbocr_boxlist** out) {
    if ((!polys && n > 0) || n < 0 || !out) return BBOCR_ERR_ARG;
    try {
        bbocr_params pp;
        bbocr_default_params(&pp);
        if (p) pp = *p;
        HostBoxes hb;
        hb.polys.assign(1, {});
        hb.hori.assign(1, {});
        hb.freeb.assign(1, {});
        for (int i = 0; i < n; ++i) {
            std::array<int, 8> a;
            memcpy(a.data(), polys + (size_t)i * 8, 32);
            hb.polys[0].push_back(a);
        }
        bbocr::GroupParams gp{pp.slope_ths, pp.ycenter_ths, pp.height_ths, pp.width_ths, pp.add_margin, pp.min_size};
        bbocr::group_text_box(hb.polys[0], gp, hb.hori[0], hb.freeb[0]);
        *out = export_boxes(hb);
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

int bbocr_host_ctc_beam(const float* probs, int n, int T, int C, int cs, int beam_width, int* text_off, int* text_idx) {
    if (!probs || !text_off || !text_idx || n <= 0 || T <= 0 || C <= 0 || C > cs || beam_width <= 0) return BBOCR_ERR_ARG;
    try {
        std::vector<int> seqs;
        for (int i = 0; i < n; ++i) { seqs.push_back(i * T); seqs.push_back(T); }
        std::vector<std::vector<int>> texts;
        ctc_beam_search_batch(probs, seqs.data(), n, C, cs, beam_width, texts);
        int o = 0;
        for (int i = 0; i < n; ++i) {
            text_off[i] = o;
            for (int v : texts[i]) text_idx[o++] = v;
        }
        text_off[n] = o;
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

int bbocr_host_crop_plan(int H, int W, const int* hori, int n_hori, const double* free_q, int n_free, int* taken, int* geom, double* minv) {
    if (H <= 0 || W <= 0 || n_hori < 0 || n_free < 0 || (n_hori > 0 && !hori) || (n_free > 0 && !free_q) || !taken || !geom || !minv) return BBOCR_ERR_ARG;
    try {
        for (int i = 0; i < n_hori + n_free; ++i) {
            BoxJob j;
            memset(&j.d, 0, sizeof(j.d));
            if (i < n_hori) {
                std::array<int, 4> b;
                memcpy(b.data(), hori + (size_t)i * 4, 16);
                taken[i] = plan_horizontal(b, 0, H, W, j);
            } else {
                std::array<double, 8> f;
                memcpy(f.data(), free_q + (size_t)(i - n_hori) * 8, 64);
                taken[i] = plan_free(f, 0, j);
            }
            if (!taken[i]) memset(&j.d, 0, sizeof(j.d));
            const CropDesc& d = j.d;
            const int v[9] = {d.sx0, d.sy0, d.sw, d.sh, d.rw, d.rh, d.fw, d.imgW, d.warp};
            std::copy(v, v + 9, geom + (size_t)i * 9);
            std::copy(d.Minv, d.Minv + 9, minv + (size_t)i * 9);
        }
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

// ---------------------------------------------------------------------------------------- single-operator entry points
// bbocr_conv_route is ConvRoute (kernels.h) under its public name: the same ints in the same order
static_assert(sizeof(bbocr_conv_route) == sizeof(ConvRoute) && offsetof(bbocr_conv_route, id) == offsetof(ConvRoute, id) &&
                  offsetof(bbocr_conv_route, piter) == offsetof(ConvRoute, piter) && offsetof(bbocr_conv_route, resw) == offsetof(ConvRoute, resw) &&
                  offsetof(bbocr_conv_route, OH) == offsetof(ConvRoute, OH) && offsetof(bbocr_conv_route, lean) == offsetof(ConvRoute, lean) &&
                  offsetof(bbocr_conv_route, grid) == offsetof(ConvRoute, grid) && offsetof(bbocr_conv_route, lds_bytes) == offsetof(ConvRoute, lds_bytes) &&
                  offsetof(bbocr_conv_route, split_off) == offsetof(ConvRoute, split_off),
              "bbocr_conv_route mirrors ConvRoute");
static_assert(BBOCR_ROUTE_COUNT == (int)CONV_ROUTE_COUNT && BBOCR_ROUTE_GEN64_P4 == (int)CONV_ROUTE_GEN64_P4 && BBOCR_ROUTE_GEN128_P16 == (int)CONV_ROUTE_GEN128_P16 &&
                  BBOCR_ROUTE_DMA64_FUSE1 == (int)CONV_ROUTE_DMA64_FUSE1 && BBOCR_ROUTE_RESW_2CH == (int)CONV_ROUTE_RESW_2CH &&
                  BBOCR_ROUTE_DMA64_448 == (int)CONV_ROUTE_DMA64_448 && BBOCR_ROUTE_DMA128_448 == (int)CONV_ROUTE_DMA128_448 &&
                  BBOCR_ROUTE_DMA2X2_128 == (int)CONV_ROUTE_DMA2X2_128 && BBOCR_ROUTE_DMA1X1_ADDUP == (int)CONV_ROUTE_DMA1X1_ADDUP,
              "BBOCR_ROUTE_* mirror ConvRouteId");

// The ConvPlan and the ConvArgs of one bbocr_op_conv2d call: the launch and the dry run of bbocr_host_conv_route both start here.  The
// pointers decide routes only by being null or not (a dry run passes stand-ins); the weights are uploaded by the caller that launches.
static ConvArgs op_conv_setup(ConvPlan& p, int el, const uint16_t* in, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int dil,
                              int relu_in, int relu_out, int out_f32, void* out, int pool_mode, int pool_relu, uint16_t* pool_out, const void* zero) {
    if (!in || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 31) || Cout <= 0 || KH <= 0 || KW <= 0) fail(BBOCR_ERR_ARG, "bad conv arguments");
    if (pool_mode < 0 || pool_mode > 2 || (pool_mode ? (!pool_out || out_f32) : !out)) fail(BBOCR_ERR_ARG, "bad conv output arguments");
    p = make_plan(Cin, Cout, KH, KW, pad, dil, el);
    const int store = cdiv(Cout, 16) * 16;
    ConvArgs a = conv_args(p, Act{(uint16_t*)in, N, H, W, Cin});
    a.relu_in0 = relu_in != 0; a.relu_out = relu_out != 0; a.out_f32 = out_f32 != 0;
    a.out = out; a.out_cs = store; a.cout_store = store;
    a.pool_mode = pool_mode; a.pool_relu = pool_relu != 0; a.store_full = (pool_mode && out) ? 1 : 0; a.pool_cs = store; a.pool_out = pool_out;
    a.zero = zero;
    return a;
}

int bbocr_op_conv2d(bbocr_ctx* ctx, const uint16_t* dev_in, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout, int KH,
                    int KW, int pad, int dil, int relu_in, int relu_out, int out_f32, void* dev_out, int pool_mode, int pool_relu,
                    uint16_t* dev_pool_out) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!w) fail(BBOCR_ERR_ARG, "bad conv arguments");
        {
            std::lock_guard<std::mutex> lk(ctx->root->pool_mu);
            ctx->root->op_conv_route = ConvRoute{};
        }
        ConvPlan p;
        ConvArgs a = op_conv_setup(p, det_el(ctx), dev_in, N, H, W, Cin, Cout, KH, KW, pad, dil, relu_in, relu_out, out_f32, dev_out, pool_mode,
                                   pool_relu, dev_pool_out, ctx->zero_page);     // element type of the context's precision (bf16 / fp16)
        std::vector<float> wv(w, w + (size_t)Cout * Cin * KH * KW), bv(Cout, 0.f);
        if (bias) std::copy(bias, bias + Cout, bv.begin());
        const size_t owned0 = ctx->owned.size();
        upload_plan(ctx, p, wv, bv);
        ConvRoute route{};
        const hipError_t e = launch_conv(p, a, ctx->stream, &route);
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        while (ctx->owned.size() > owned0) { (void)hipFree(ctx->owned.back()); ctx->owned.pop_back(); ctx->owned_bytes.pop_back(); }
        {
            std::lock_guard<std::mutex> lk(ctx->root->pool_mu);
            ctx->root->op_conv_route = route;
        }
        HIPCHK(e);
        HIPCHK(e2);
    }, /*exclusive=*/true);      // uploads a temporary plan into the root's weight list
}

int bbocr_op_conv2d_route(bbocr_ctx* ctx, bbocr_conv_route* out) {
    if (!ctx || !out) return BBOCR_ERR_ARG;
    bbocr_ctx* root = ctx->root ? ctx->root : ctx;
    std::lock_guard<std::mutex> lk(root->pool_mu);
    memcpy(out, &root->op_conv_route, sizeof(*out));
    return BBOCR_OK;
}

int bbocr_host_conv_route(int el, int N, int H, int W, int Cin, int Cout, int KH, int KW, int pad, int dil, int relu_in, int relu_out, int out_f32,
                          int pool_mode, int pool_relu, int store_full, bbocr_conv_route* out) {
    if (!out || (el != 0 && el != 1)) return BBOCR_ERR_ARG;
    memset(out, 0, sizeof(*out));
    try {
        // stand-ins for the device pointers of the call: the dispatch only asks whether they are there
        static uint16_t here[8];
        const bool full = !pool_mode || store_full;
        ConvPlan p;
        ConvArgs a = op_conv_setup(p, el, here, N, H, W, Cin, Cout, KH, KW, pad, dil, relu_in, relu_out, out_f32, full ? (void*)here : nullptr, pool_mode,
                                   pool_relu, pool_mode ? here : nullptr, here);
        ConvRoute route{};
        const hipError_t e = launch_conv(p, a, nullptr, &route, /*dry=*/true);
        memcpy(out, &route, sizeof(*out));
        return e == hipSuccess ? BBOCR_OK : BBOCR_ERR_HIP;      // what bbocr_op_conv2d returns for the refusal; out->status has the HIP code
    } catch (const StatusError& se) {
        return se.code;
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
}

int bbocr_crnn_logits(bbocr_ctx* ctx, const uint16_t* dev_crops, int n, int imgW, float* dev_logits) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!ctx->crnn_loaded) fail(BBOCR_ERR_STATE, "recogniser weights not loaded");
        if (!dev_crops || !dev_logits || n <= 0 || imgW < 64 || (imgW & 63)) fail(BBOCR_ERR_ARG, "bad crop batch");
        // what a recognition pass runs: the n crops planned as one part, side by side in its wide image with REC_GAP zero columns between
        // them (a cleared buffer: 0 is the padding value, and the padding code of the exact mode), conv stack over the wide image with the
        // gaps cleared after every layer, gathered 3-row mean, the part's LSTM tile table, sequence stage
        std::vector<BoxJob> jobs(n);
        std::vector<int> all(n);
        for (int i = 0; i < n; ++i) { jobs[i].d = CropDesc{}; jobs[i].d.imgW = imgW; all[i] = i; }
        RecPart part;
        rec_plan_part(jobs, all, 0, 0, part);
        const size_t rows = part.rows, rows_pad = align_up(rows, 256);
        ctx->seq_v.ensure(rows_pad * 256 * 2 * (rec_split(ctx) ? 2 : 1));
        const size_t cs = (size_t)rec_cs(ctx);
        if (rec_wide(ctx) && rows_pad * cs * 4 > ((size_t)1 << 30)) fail(BBOCR_ERR_ARG, "crop batch too large: the logits of a wide model are kept at or below 1 GiB");
        ctx->seq_logits.ensure(rows_pad * cs * 4);
        const CropDesc* dd = rec_upload_descs(ctx, part, ctx->crop_desc);
        uint16_t* wide = rec_wide_image(ctx, part);
        HIPCHK(hipMemsetAsync(wide, 0, 64 * part.cols * 2, ctx->stream));
        for (int i = 0; i < n; ++i)
            HIPCHK(hipMemcpy2DAsync(wide + part.descs[i].slot, part.cols * 2, dev_crops + (size_t)i * 64 * imgW, (size_t)imgW * 2, (size_t)imgW * 2, 64,
                                    hipMemcpyDeviceToDevice, ctx->stream));
        crnn_features_wide(ctx, part, dd, wide);
        RecRun run;
        rec_add_tables(run, part, lstm_tile_seqs(rec_mode(ctx)));
        rec_seq_tiles(ctx, run);
        ctx->seq_tables.ensure((run.tiles.size() + run.seqs.size()) * 4);
        int* tiles_dev = (int*)ctx->seq_tables.p;
        int* seqs_dev = tiles_dev + run.tiles.size();
        HIPCHK(hipMemcpyAsync(tiles_dev, run.tiles.data(), run.tiles.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(seqs_dev, run.seqs.data(), run.seqs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        crnn_sequence(ctx, rows, rows_pad, tiles_dev, (int)(run.tiles.size() / 4), seqs_dev, (int)(run.seqs.size() / 2), (float*)ctx->seq_logits.p);
        HIPCHK(hipMemcpyAsync(dev_logits, ctx->seq_logits.p, rows * cs * 4, hipMemcpyDeviceToDevice, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

// the segment table of the two rec_quant entry points: pairs {first row, T} that tile [0, rows) in order; uploaded behind `ahead` ints
static const int* q8_op_seqs(bbocr_ctx* ctx, const int* seqs, int nseq, int rows, const std::vector<int>& ahead) {
    if (!rec_quant(ctx)) fail(BBOCR_ERR_STATE, "this context was not created with rec_quant = 1");
    if (!ctx->crnn_loaded) fail(BBOCR_ERR_STATE, "recogniser weights not loaded");
    if (!seqs || nseq <= 0 || rows <= 0) fail(BBOCR_ERR_ARG, "bad segment table");
    long long at = 0;
    for (int i = 0; i < nseq; ++i) {
        if (seqs[2 * i] != at || seqs[2 * i + 1] <= 0) fail(BBOCR_ERR_ARG, "the segments must tile the rows in order");
        at += seqs[2 * i + 1];
    }
    if (at != rows) fail(BBOCR_ERR_ARG, "the segments must tile the rows in order");
    ctx->seq_tables.ensure((ahead.size() + (size_t)nseq * 2) * 4);
    int* d = (int*)ctx->seq_tables.p;
    if (!ahead.empty()) HIPCHK(hipMemcpyAsync(d, ahead.data(), ahead.size() * 4, hipMemcpyHostToDevice, ctx->stream));     // (the callers end synchronised)
    HIPCHK(hipMemcpyAsync(d + ahead.size(), seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
    return d + ahead.size();
}

int bbocr_op_qlinear(bbocr_ctx* ctx, const float* dev_x, int rows, const int* seqs, int nseq, int layer, float* dev_out, uint8_t* dev_codes,
                     float* seg_params) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_x || !dev_out || !dev_codes || !seg_params || layer < 0 || layer > 4) fail(BBOCR_ERR_ARG, "bad qlinear arguments");
        const int* seqs_dev = q8_op_seqs(ctx, seqs, nseq, rows, {});
        const bbocr_ctx::Q8Layer& L = layer < 2 ? ctx->q_ih[layer] : (layer < 4 ? ctx->q_lin[layer - 2] : ctx->q_pred);
        const int K = (layer == 2 || layer == 3) ? 512 : 256, N = layer < 2 ? 2048 : (layer < 4 ? 256 : rec_cs(ctx));
        const size_t rows_pad = align_up((size_t)rows, 256);
        ctx->seq_q8.ensure(rows_pad * 512);
        ctx->seq_rowp.ensure(rows_pad * 16);
        ctx->seq_xp.ensure(rows_pad * 2048 * 4);
        ctx->seq_lin.ensure((size_t)nseq * 8);
        HIPCHK(launch_q8_quantize(dev_x, 0, K, (size_t)rows, rows_pad, seqs_dev, nseq, (float*)ctx->seq_rowp.p, (int8_t*)ctx->seq_q8.p, dev_codes,
                                  (float*)ctx->seq_lin.p, ctx->stream));
        HIPCHK(launch_q8_gemm((const int8_t*)ctx->seq_q8.p, rows_pad, K, L.w, N, (const float*)ctx->seq_rowp.p, L.scale, L.bias, (float*)ctx->seq_xp.p, N,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(dev_out, ctx->seq_xp.p, (size_t)rows * N * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(seg_params, ctx->seq_lin.p, (size_t)nseq * 8, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_qlstm(bbocr_ctx* ctx, const float* dev_g, int rows, const int* seqs, int nseq, int layer, float* dev_h, float* dev_c, uint8_t* dev_hcodes,
                   float* dev_hparams) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_g || !dev_h || !dev_c || !dev_hcodes || !dev_hparams || layer < 0 || layer > 1) fail(BBOCR_ERR_ARG, "bad qlstm arguments");
        RecRun run;
        if (seqs && nseq > 0) run.seqs.assign(seqs, seqs + (size_t)nseq * 2);
        rec_seq_tiles(ctx, run);
        const int* seqs_dev = q8_op_seqs(ctx, seqs, nseq, rows, run.tiles);
        const bbocr_ctx::Q8Layer& L = ctx->q_hh[layer];
        HIPCHK(launch_lstm_q8(dev_g, L.w, L.scale, L.bias, dev_h, seqs_dev, (const int*)ctx->seq_tables.p, (int)(run.tiles.size() / 4), dev_c, dev_hcodes,
                              dev_hparams, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

// classes a CTC entry point takes on this context: beyond 128 only where the context itself is that wide (bbocr_config::rec_classes) -- on
// an english_g2 context a wider C stays the argument error it always was
static int op_ctc_max_classes(const bbocr_ctx* ctx) { return rec_wide(ctx) ? BBOCR_REC_CLASSES_MAX : 128; }

// the host class mask of a CTC entry point over more than 128 classes -> the slot's device words (ceil(C / 32)); null: no mask, or C <= 128
// (launch_ctc takes its four words by value).  The callers end synchronised.
static const unsigned int* op_wide_mask(bbocr_ctx* ctx, int C, const unsigned int* host_words) {
    if (C <= 128 || !host_words) return nullptr;
    const size_t bytes = (size_t)(C + 31) / 32 * 4;
    ctx->ctc_mask.ensure(bytes);
    HIPCHK(hipMemcpyAsync(ctx->ctc_mask.p, host_words, bytes, hipMemcpyHostToDevice, ctx->stream));
    return (const unsigned int*)ctx->ctc_mask.p;
}

int bbocr_op_ctc(bbocr_ctx* ctx, const float* dev_logits, int n, int T, int C, int cs, int* text_off, int* text_idx, double* conf,
                 const unsigned int* ignore_mask, int beam_width) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_logits || !text_off || !text_idx || !conf || n <= 0 || T <= 0 || C <= 0 || C > cs || C > op_ctc_max_classes(ctx)) fail(BBOCR_ERR_ARG, "bad ctc arguments");
        const size_t rows = (size_t)n * T;
        const unsigned int* mask_dev = op_wide_mask(ctx, C, ignore_mask);
        std::vector<int> seqs;
        for (int i = 0; i < n; ++i) { seqs.push_back(i * T); seqs.push_back(T); }
        const int route = ctc_route(beam_width, C, seqs.data(), n, false, rec_beam_wide(ctx));       // as rec_finish routes a recognition pass
        const bool dev_beam = route == CTC_BEAM_DEVICE || route == CTC_BEAM_DEVICE_WIDE;
        ctc_size(ctx, rows, n, cs, route);
        ctx->seq_tables.ensure(seqs.size() * 4);
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs.data(), seqs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (C > 128)
            HIPCHK(launch_ctc_wide(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, n, (int*)ctx->ctc_idx.p, (float*)ctx->ctc_pmax.p,
                                   (int*)ctx->ctc_out_idx.p, (CtcOut*)ctx->ctc_out.p, ctx->stream, mask_dev,
                                   route != CTC_GREEDY ? (float*)ctx->ctc_probs.p : nullptr));
        else
            HIPCHK(launch_ctc(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, n, (int*)ctx->ctc_idx.p, (float*)ctx->ctc_pmax.p,
                              (int*)ctx->ctc_out_idx.p, (CtcOut*)ctx->ctc_out.p, ctx->stream, ignore_mask,
                              route != CTC_GREEDY ? (float*)ctx->ctc_probs.p : nullptr));
        std::vector<int> oidx(rows), blen(dev_beam ? n : 0);
        std::vector<CtcOut> oo(n);
        std::vector<float> probs(route == CTC_BEAM_HOST ? rows * cs : 0);
        std::vector<std::vector<int>> beam_texts;
        HIPCHK(hipMemcpyAsync(oo.data(), ctx->ctc_out.p, oo.size() * sizeof(CtcOut), hipMemcpyDeviceToHost, ctx->stream));
        if (dev_beam) {            // the search's text takes the place of the greedy classes
            if (route == CTC_BEAM_DEVICE_WIDE)
                HIPCHK(launch_ctc_beam_wide((const float*)ctx->ctc_probs.p, rows, C, cs, (const int*)ctx->seq_tables.p, n, T, beam_width,
                                            (int*)ctx->ctc_cand_n.p, (int*)ctx->ctc_cand.p, (int*)ctx->ctc_beam_idx.p, (int*)ctx->ctc_beam_len.p, ctx->stream));
            else
                HIPCHK(launch_ctc_beam((const float*)ctx->ctc_probs.p, rows, C, cs, (const int*)ctx->seq_tables.p, n, T, beam_width,
                                       (int*)ctx->ctc_beam_idx.p, (int*)ctx->ctc_beam_len.p, ctx->stream));
            HIPCHK(hipMemcpyAsync(oidx.data(), ctx->ctc_beam_idx.p, oidx.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(blen.data(), ctx->ctc_beam_len.p, blen.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            HIPCHK(hipMemcpyAsync(oidx.data(), ctx->ctc_out_idx.p, oidx.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (route == CTC_BEAM_HOST)
                HIPCHK(hipMemcpyAsync(probs.data(), ctx->ctc_probs.p, probs.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        }
        slot_sync(ctx, ctx->stream);
        if (route == CTC_BEAM_HOST) ctc_beam_search_batch(probs.data(), seqs.data(), n, C, cs, beam_width, beam_texts, &host_pool(ctx));
        if (route == CTC_BEAM_DEVICE_WIDE)
            ctc_beam_wide_fallback(ctx, ctx->stream, (const float*)ctx->ctc_probs.p, seqs.data(), n, C, cs, beam_width, blen.data(), beam_texts);
        std::vector<int> text;
        int o = 0;
        for (int i = 0; i < n; ++i) {
            text_off[i] = o;
            if (route == CTC_BEAM_HOST || (route == CTC_BEAM_DEVICE_WIDE && blen[i] < 0)) conf[i] = ctc_decode(oo[i], beam_texts[i].data(), (int)beam_texts[i].size(), text);
            else conf[i] = ctc_decode(oo[i], oidx.data() + (size_t)i * T, dev_beam ? std::clamp(blen[i], 0, T) : oo[i].len, text);
            for (int v : text) text_idx[o++] = v;
        }
        text_off[n] = o;
    });
}

int bbocr_op_ctc_probs(bbocr_ctx* ctx, const float* dev_logits, size_t rows, int C, int cs, const unsigned int* ignore_mask, float* dev_probs_out) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_logits || !dev_probs_out || rows == 0 || rows > (size_t)INT32_MAX || C <= 0 || C > op_ctc_max_classes(ctx) || C > cs) fail(BBOCR_ERR_ARG, "bad ctc arguments");
        const unsigned int* mask_dev = op_wide_mask(ctx, C, ignore_mask);
        // launch_ctc with one sequence over all rows: the rows kernel is per row, the collapse's output is not read
        ctc_size(ctx, rows, 1, cs, CTC_GREEDY);
        const int seq[2] = {0, (int)rows};
        ctx->seq_tables.ensure(sizeof(seq));
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seq, sizeof(seq), hipMemcpyHostToDevice, ctx->stream));
        if (C > 128)
            HIPCHK(launch_ctc_wide(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, 1, (int*)ctx->ctc_idx.p, (float*)ctx->ctc_pmax.p,
                                   (int*)ctx->ctc_out_idx.p, (CtcOut*)ctx->ctc_out.p, ctx->stream, mask_dev, dev_probs_out));
        else
            HIPCHK(launch_ctc(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, 1, (int*)ctx->ctc_idx.p, (float*)ctx->ctc_pmax.p,
                              (int*)ctx->ctc_out_idx.p, (CtcOut*)ctx->ctc_out.p, ctx->stream, ignore_mask, dev_probs_out));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_ctc_rows(bbocr_ctx* ctx, const float* dev_logits, size_t rows, int C, int cs, const unsigned int* ignore_mask, const int* seqs, int nseq,
                      float* dev_probs_out, int* dev_idx, float* dev_pmax, int* dev_out_idx, int* dev_ctc_out) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_logits || !dev_idx || !dev_pmax || !dev_out_idx || !dev_ctc_out || !seqs || nseq <= 0 || rows == 0 || rows > (size_t)INT32_MAX || C <= 0 ||
            C > op_ctc_max_classes(ctx) || C > cs)
            fail(BBOCR_ERR_ARG, "bad ctc arguments");
        for (int i = 0; i < nseq; ++i) {
            const long long first = seqs[2 * i], T = seqs[2 * i + 1];
            if (first < 0 || T < 0 || first + T > (long long)rows) fail(BBOCR_ERR_ARG, "a sequence lies outside the rows");
        }
        const unsigned int* mask_dev = op_wide_mask(ctx, C, ignore_mask);
        ctx->seq_tables.ensure((size_t)nseq * 8);
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
        if (C > 128)
            HIPCHK(launch_ctc_wide(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, nseq, dev_idx, dev_pmax, dev_out_idx, (CtcOut*)dev_ctc_out,
                                   ctx->stream, mask_dev, dev_probs_out));
        else
            HIPCHK(launch_ctc(dev_logits, rows, C, cs, (const int*)ctx->seq_tables.p, nseq, dev_idx, dev_pmax, dev_out_idx, (CtcOut*)dev_ctc_out, ctx->stream,
                              ignore_mask, dev_probs_out));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_pred(bbocr_ctx* ctx, const uint16_t* dev_x, size_t rows, float* dev_logits) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!ctx->crnn_loaded) fail(BBOCR_ERR_STATE, "recogniser weights not loaded");
        if (rec_split(ctx) || rec_quant(ctx)) fail(BBOCR_ERR_STATE, "bbocr_op_pred takes the 16-bit recogniser modes");
        const size_t rows_pad = align_up(rows, 256), cs = (size_t)rec_cs(ctx);
        if (!dev_x || !dev_logits || rows == 0 || rows_pad * cs * 4 > ((size_t)1 << 30)) fail(BBOCR_ERR_ARG, "bad pred arguments");
        // as a sequence pass holds them: x in seq_v, padded with zero rows to whole 256-row tiles; logits in seq_logits
        ctx->seq_v.ensure(rows_pad * 256 * 2);
        ctx->seq_logits.ensure(rows_pad * cs * 4);
        HIPCHK(hipMemsetAsync(ctx->seq_v.p, 0, rows_pad * 256 * 2, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->seq_v.p, dev_x, rows * 256 * 2, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->arena.dry = false;
        crnn_seq_pred(ctx, (const uint16_t*)ctx->seq_v.p, rows_pad, (float*)ctx->seq_logits.p);
        HIPCHK(hipMemcpyAsync(dev_logits, ctx->seq_logits.p, rows * cs * 4, hipMemcpyDeviceToDevice, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_pred_ctc(bbocr_ctx* ctx, const uint16_t* dev_x, size_t rows, const uint32_t* dev_mask_words, int n_words, int* dev_idx, float* dev_pmax) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!ctx->crnn_loaded) fail(BBOCR_ERR_STATE, "recogniser weights not loaded");
        if (!ctx->pred_wide) fail(BBOCR_ERR_STATE, "the fused Prediction + CTC kernel serves contexts of more than 128 classes in a 16-bit precision");
        const int C = rec_classes(ctx), max_words = (C + 31) / 32;
        if (!dev_x || !dev_idx || !dev_pmax || rows == 0 || rows > (size_t)INT32_MAX || n_words < 0 || n_words > max_words || (n_words > 0 && !dev_mask_words))
            fail(BBOCR_ERR_ARG, "bad pred_ctc arguments");
        // the kernel reads ceil(C / 32) words: the caller's, with zeros behind them
        ctx->ctc_mask.ensure((size_t)max_words * 4);
        HIPCHK(hipMemsetAsync(ctx->ctc_mask.p, 0, (size_t)max_words * 4, ctx->stream));
        if (n_words > 0) HIPCHK(hipMemcpyAsync(ctx->ctc_mask.p, dev_mask_words, (size_t)n_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(launch_pred_ctc(rec_el(ctx), dev_x, rows, ctx->pred_wide, ctx->pred_wide_b, C, (const unsigned int*)ctx->ctc_mask.p, dev_idx, dev_pmax, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_ctc_beam(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width, int* text_off,
                      int* text_idx) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_probs || !seqs || !text_off || !text_idx || nseq <= 0 || rows > (size_t)INT32_MAX || C <= 0 || C > 128 || cs < C || beam_width < 1 ||
            beam_width > BBOCR_BEAM_DEVICE_MAX)
            fail(BBOCR_ERR_ARG, "bad beam-search arguments");
        int max_T = 0;
        for (int i = 0; i < nseq; ++i) {
            const long long first = seqs[2 * i], T = seqs[2 * i + 1];
            if (first < 0 || T < 0 || first + T > (long long)rows) fail(BBOCR_ERR_ARG, "a sequence lies outside the rows");
            max_T = std::max(max_T, (int)T);
        }
        if (!ctc_beam_on_device(beam_width, C, max_T)) fail(BBOCR_ERR_ARG, "the longest sequence does not fit the device search at this width");
        ctx->seq_tables.ensure((size_t)nseq * 8);
        ctx->ctc_beam_idx.ensure(std::max<size_t>(rows, 1) * 4);
        ctx->ctc_beam_len.ensure((size_t)nseq * 4);
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_ctc_beam(dev_probs, rows, C, cs, (const int*)ctx->seq_tables.p, nseq, max_T, beam_width, (int*)ctx->ctc_beam_idx.p,
                               (int*)ctx->ctc_beam_len.p, ctx->stream));
        std::vector<int> bidx(rows), blen(nseq);
        if (rows) HIPCHK(hipMemcpyAsync(bidx.data(), ctx->ctc_beam_idx.p, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(blen.data(), ctx->ctc_beam_len.p, (size_t)nseq * 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        int o = 0;
        for (int i = 0; i < nseq; ++i) {
            text_off[i] = o;
            const int n = std::clamp(blen[i], 0, seqs[2 * i + 1]);
            for (int k = 0; k < n; ++k) text_idx[o++] = bidx[(size_t)seqs[2 * i] + k];
        }
        text_off[nseq] = o;
    });
}

int bbocr_op_ctc_beam_wide(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width, int* text_off,
                           int* text_idx, int* n_host) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_probs || !seqs || !text_off || !text_idx || nseq <= 0 || rows > (size_t)INT32_MAX || C <= 128 || C > op_ctc_max_classes(ctx) || cs < C ||
            beam_width < 1 || beam_width > BBOCR_BEAM_DEVICE_MAX)
            fail(BBOCR_ERR_ARG, "bad beam-search arguments");
        int max_T = 0;
        for (int i = 0; i < nseq; ++i) {
            const long long first = seqs[2 * i], T = seqs[2 * i + 1];
            if (first < 0 || T < 0 || first + T > (long long)rows) fail(BBOCR_ERR_ARG, "a sequence lies outside the rows");
            max_T = std::max(max_T, (int)T);
        }
        if (!ctc_beam_wide_on_device(beam_width, C, max_T)) fail(BBOCR_ERR_ARG, "the longest sequence does not fit the device search at this width");
        ctx->seq_tables.ensure((size_t)nseq * 8);
        ctx->ctc_beam_idx.ensure(std::max<size_t>(rows, 1) * 4);
        ctx->ctc_beam_len.ensure((size_t)nseq * 4);
        ctx->ctc_cand.ensure(std::max<size_t>(rows, 1) * (size_t)kBeamWideCand * 8);
        ctx->ctc_cand_n.ensure(std::max<size_t>(rows, 1) * 4);
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_ctc_beam_wide(dev_probs, rows, C, cs, (const int*)ctx->seq_tables.p, nseq, max_T, beam_width, (int*)ctx->ctc_cand_n.p,
                                    (int*)ctx->ctc_cand.p, (int*)ctx->ctc_beam_idx.p, (int*)ctx->ctc_beam_len.p, ctx->stream));
        std::vector<int> bidx(rows), blen(nseq);
        if (rows) HIPCHK(hipMemcpyAsync(bidx.data(), ctx->ctc_beam_idx.p, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(blen.data(), ctx->ctc_beam_len.p, (size_t)nseq * 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        std::vector<std::vector<int>> host_texts;
        const int nh = ctc_beam_wide_fallback(ctx, ctx->stream, dev_probs, seqs, nseq, C, cs, beam_width, blen.data(), host_texts);
        int o = 0;
        for (int i = 0; i < nseq; ++i) {
            text_off[i] = o;
            if (blen[i] < 0) {
                for (int v : host_texts[i]) text_idx[o++] = v;
                continue;
            }
            const int n = std::min(blen[i], seqs[2 * i + 1]);
            for (int k = 0; k < n; ++k) text_idx[o++] = bidx[(size_t)seqs[2 * i] + k];
        }
        text_off[nseq] = o;
        if (n_host) *n_host = nh;
    });
}

int bbocr_host_ctc_route(int beam_wide, int beam_width, int C, const int* seqs, int nseq) {
    if ((nseq > 0 && !seqs) || nseq < 0) return BBOCR_ERR_ARG;
    return ctc_route(beam_width, C, seqs, nseq, false, beam_wide == 1 && C > 128);
}

int bbocr_op_resize_u8(bbocr_ctx* ctx, const uint8_t* dev_src, int N, int sh, int sw, int C, uint8_t* dev_dst, int dh, int dw) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_src || !dev_dst || N <= 0 || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || C <= 0) fail(BBOCR_ERR_ARG, "bad resize arguments");
        HIPCHK(launch_resize_u8(dev_src, N, sh, sw, C, dev_dst, dh, dw, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_op_ycc_to_rgb(bbocr_ctx* ctx, const uint8_t* dev_ycc, size_t npix, int pixel_stride, uint8_t* dev_rgb, uint8_t* dev_gray) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_ycc || !dev_rgb || npix == 0 || (pixel_stride != 3 && pixel_stride != 4)) fail(BBOCR_ERR_ARG, "bad colour-conversion arguments");
        HIPCHK(launch_ycc_to_rgb_gray(dev_ycc, pixel_stride, dev_rgb, dev_gray, npix, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_upload_pages(bbocr_ctx* root, const void* const* host_pages, int n, size_t bytes_each, void* dev_dst) {
    // NOT a call slot's work: an upload stage feeding two calls in flight must not wait for one of them to return.  Every page is checked
    // before the first copy is queued: a refused call has touched nothing.
    return lane_guarded(root, &bbocr_ctx::upload_lane, false, [&](hipStream_t st) {
        if (!host_pages || !dev_dst || n <= 0 || bytes_each == 0) fail(BBOCR_ERR_ARG, "bad upload arguments");
        for (int k = 0; k < n; ++k)
            if (!host_pages[k]) fail(BBOCR_ERR_ARG, "null page");
        for (int k = 0; k < n; ++k)
            HIPCHK(hipMemcpyAsync((unsigned char*)dev_dst + (size_t)k * bytes_each, host_pages[k], bytes_each, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    });
}

int bbocr_op_crops(bbocr_ctx* ctx, const uint8_t* dev_gray, int H, int W, const int* hori, int n_hori, const double* free_q, int n_free, int imgW,
                   float contrast, uint16_t* dev_out, int* n_out, int mode) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_gray) fail(BBOCR_ERR_ARG, "bad crop arguments");
        const int hori_off[2] = {0, n_hori}, free_off[2] = {0, n_free};
        op_crops(ctx, GrayPages{dev_gray, H, W}, 1, hori, hori_off, free_q, free_off, imgW, contrast, dev_out, n_out, mode);
    });
}

int bbocr_op_crops_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, const int* hori, const int* hori_off, const double* free_q,
                         const int* free_off, int imgW, float contrast, uint16_t* dev_out, int* n_out, int mode) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!pages || n <= 0 || n > 65535 || !hori_off || !free_off) fail(BBOCR_ERR_ARG, "bad crop arguments");
        // the page table: offsets from the first page's plane (the pages are allocations of their own; the kernels add a signed offset)
        std::vector<CropPage> tab(n);
        for (int k = 0; k < n; ++k) {
            const bbocr_page& g = pages[k];
            const long long pitch = g.gray_pitch ? g.gray_pitch : (long long)g.W;
            if (!g.dev_gray || g.H <= 0 || g.W <= 0 || (long long)g.H * g.W >= (1LL << 30) || pitch < g.W) fail(BBOCR_ERR_ARG, "bad gray page");
            tab[k] = CropPage{(long long)(g.dev_gray - pages[0].dev_gray), pitch, g.H, g.W};
        }
        ctx->pg_tab.ensure(tab.size() * sizeof(CropPage));
        HIPCHK(hipMemcpyAsync(ctx->pg_tab.p, tab.data(), tab.size() * sizeof(CropPage), hipMemcpyHostToDevice, ctx->stream));   // (op_crops ends synchronised)
        op_crops(ctx, GrayPages{pages[0].dev_gray, 0, 0, tab.data(), (const CropPage*)ctx->pg_tab.p}, n, hori, hori_off, free_q, free_off, imgW, contrast,
                 dev_out, n_out, mode);
    });
}

}  // extern "C"
