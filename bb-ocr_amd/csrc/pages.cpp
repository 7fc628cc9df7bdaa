// Pages of mixed shapes in one call (include/bbocr.h: bbocr_readtext_pages and its plan / stage entries): the plan of a page list, the
// page tables of csrc/pages.hip and of the crop kernels, and the pipeline call -- bbocr_readtext_batch's sub-batch loop with a pass being
// (shape group, pages of it) and ONE recognition over the crops of all pages.
#include "ctx.h"

namespace {

struct PageGroup {
    int H, W;
    std::vector<int> pages;                  // the caller's indices, in the caller's order (= slot order)
    long long rgb_base, gray_base;           // the group's blocks [nb][H][W][3] / [nb][H][W] in the two staging buffers
};
struct PagesPlan {
    std::vector<int> group_of_page, slot_in_group;
    std::vector<long long> rgb_off, gray_off;
    std::vector<PageGroup> groups;           // numbered by first appearance
    long long rgb_bytes = 0, gray_bytes = 0;
};

inline long long rgb_pitch(const bbocr_page& g) { return g.rgb_pitch ? g.rgb_pitch : 3LL * g.W; }
inline long long gray_pitch(const bbocr_page& g) { return g.gray_pitch ? g.gray_pitch : (long long)g.W; }

// the one planning function: bbocr_host_pages_plan returns it, bbocr_readtext_pages and bbocr_op_pack_pages run on it
PagesPlan plan_pages(const bbocr_page* pages, int n, const bbocr_params& p) {
    if (!pages || n <= 0) fail(BBOCR_ERR_ARG, "pages: a list of n > 0 pages expected");
    if (n > 65535) fail(BBOCR_ERR_ARG, "pages: at most 65535 pages per call");
    PagesPlan plan;
    plan.group_of_page.resize(n); plan.slot_in_group.resize(n); plan.rgb_off.resize(n); plan.gray_off.resize(n);
    std::map<std::pair<int, int>, int> by_shape;
    for (int i = 0; i < n; ++i) {
        const bbocr_page& g = pages[i];
        const std::string at = "page " + std::to_string(i) + ": ";
        if (!g.dev_rgb) fail(BBOCR_ERR_ARG, at + "null dev_rgb");
        if (g.H <= 0 || g.W <= 0) fail(BBOCR_ERR_ARG, at + "bad page shape");
        if ((long long)g.H * g.W >= (1LL << 30)) fail(BBOCR_ERR_ARG, at + "page too large");
        if (rgb_pitch(g) < 3LL * g.W || (g.dev_gray && gray_pitch(g) < (long long)g.W)) fail(BBOCR_ERR_ARG, at + "row pitch smaller than a row");
        const DetDims d = det_dims(g.H, g.W, p.canvas_size, p.mag_ratio);
        if (d.th <= 0 || d.tw <= 0) fail(BBOCR_ERR_ARG, at + "page collapses to zero size");
        auto it = by_shape.find({g.H, g.W});
        if (it == by_shape.end()) {
            it = by_shape.emplace(std::make_pair(g.H, g.W), (int)plan.groups.size()).first;
            plan.groups.push_back(PageGroup{g.H, g.W, {}, 0, 0});
        }
        plan.group_of_page[i] = it->second;
        plan.slot_in_group[i] = (int)plan.groups[it->second].pages.size();
        plan.groups[it->second].pages.push_back(i);
    }
    for (PageGroup& gr : plan.groups) {
        const long long px = (long long)gr.H * gr.W;
        gr.rgb_base = plan.rgb_bytes;
        gr.gray_base = plan.gray_bytes;
        for (size_t k = 0; k < gr.pages.size(); ++k) {
            plan.rgb_off[gr.pages[k]] = gr.rgb_base + (long long)k * px * 3;
            plan.gray_off[gr.pages[k]] = gr.gray_base + (long long)k * px;
        }
        plan.rgb_bytes = (long long)align_up((size_t)(gr.rgb_base + (long long)gr.pages.size() * px * 3), 256);
        plan.gray_bytes = (long long)align_up((size_t)(gr.gray_base + (long long)gr.pages.size() * px), 256);
    }
    return plan;
}

// The two device tables of a call, uploaded by ONE copy queued on the compute stream: PackPage [n] (what launch_pack_pages reads) and
// CropPage [n] (what the crop kernels index with CropDesc::img), both in the order `inner` (inner[k] = the caller's index of the page
// with table index k).  crop_host receives the second table; returns the tile count of the pack launch.  The staging pointers are the
// ones that launch will write: a page's 16-byte path is chosen from the addresses it really touches.
struct PageTables { const PackPage* pack; const CropPage* crop; int ntiles; };
PageTables upload_page_tables(bbocr_ctx* c, const bbocr_page* pages, const PagesPlan& plan, const std::vector<int>& inner, std::vector<CropPage>& crop_host,
                              const uint8_t* rgb_staging, const uint8_t* gray_staging) {
    const size_t n = inner.size();
    const size_t crop_at = align_up(n * sizeof(PackPage), 256), bytes = crop_at + n * sizeof(CropPage);
    c->pg_pin.ensure(bytes);
    c->pg_tab.ensure(bytes);
    PackPage* pk = (PackPage*)c->pg_pin.p;
    CropPage* cp = (CropPage*)((char*)c->pg_pin.p + crop_at);
    crop_host.resize(n);
    long long tiles = 0;
    for (size_t k = 0; k < n; ++k) {
        const int i = inner[k];
        const bbocr_page& g = pages[i];
        PackPage& q = pk[k];
        q.rgb = g.dev_rgb; q.gray = g.dev_gray;
        q.rgb_pitch = rgb_pitch(g); q.gray_pitch = g.dev_gray ? gray_pitch(g) : 0;
        q.rgb_off = plan.rgb_off[i]; q.gray_off = plan.gray_off[i];
        q.H = g.H; q.W = g.W;
        q.tile0 = (int)tiles;
        q.vec = pack_page_vec(q, rgb_staging, gray_staging);
        tiles += ((long long)g.H * g.W + PK_TILE_PX - 1) / PK_TILE_PX;
        if (tiles > PK_MAX_TILES) fail(BBOCR_ERR_ARG, "pages: too many pixels in one call (the pack launch holds fewer than 2^24 tiles)");
        cp[k] = crop_host[k] = CropPage{plan.gray_off[i], (long long)g.W, g.H, g.W};
    }
    HIPCHK(hipMemcpyAsync(c->pg_tab.p, c->pg_pin.p, bytes, hipMemcpyHostToDevice, c->stream));
    return PageTables{(const PackPage*)c->pg_tab.p, (const CropPage*)((const char*)c->pg_tab.p + crop_at), (int)tiles};
}

}  // namespace

extern "C" {

int bbocr_host_pages_plan(const bbocr_page* pages, int n, const bbocr_params* p, int* group_of_page, int* slot_in_group, long long* rgb_off,
                          long long* gray_off, int* n_groups, long long* staging_bytes) {
    try {
        bbocr_params pp;
        bbocr_default_params(&pp);
        if (p) pp = *p;
        const PagesPlan plan = plan_pages(pages, n, pp);
        for (int i = 0; i < n; ++i) {
            if (group_of_page) group_of_page[i] = plan.group_of_page[i];
            if (slot_in_group) slot_in_group[i] = plan.slot_in_group[i];
            if (rgb_off) rgb_off[i] = plan.rgb_off[i];
            if (gray_off) gray_off[i] = plan.gray_off[i];
        }
        if (n_groups) *n_groups = (int)plan.groups.size();
        if (staging_bytes) { staging_bytes[0] = plan.rgb_bytes; staging_bytes[1] = plan.gray_bytes; }
    } catch (const StatusError& se) {
        return se.code;
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

int bbocr_op_pack_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, uint8_t* dev_rgb_staging, uint8_t* dev_gray_staging) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        bbocr_params pp;
        bbocr_default_params(&pp);
        const PagesPlan plan = plan_pages(pages, n, pp);
        if (!dev_rgb_staging || !dev_gray_staging) fail(BBOCR_ERR_ARG, "null staging buffer");
        std::vector<int> inner(n);
        for (int i = 0; i < n; ++i) inner[i] = i;
        std::vector<CropPage> crop_host;
        const PageTables t = upload_page_tables(ctx, pages, plan, inner, crop_host, dev_rgb_staging, dev_gray_staging);
        HIPCHK(launch_pack_pages(t.pack, n, t.ntiles, dev_rgb_staging, dev_gray_staging, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

int bbocr_readtext_pages(bbocr_ctx* ctx, const bbocr_page* pages, int n, const bbocr_params* p, bbocr_result** out) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        bbocr_params pp;
        bbocr_default_params(&pp);
        if (p) pp = *p;
        if (!out) fail(BBOCR_ERR_ARG, "null pointer");
        const PagesPlan plan = plan_pages(pages, n, pp);                  // every argument check: nothing is queued yet
        memset(ctx->times, 0, sizeof(ctx->times));
        auto t_all = clk::now();
        // Pass order: shape group by shape group, the group with the fewest canvas pixels last -- only the last pass's box extraction is
        // exposed, everything before it overlaps the next pass.  (Results do not depend on the order.)
        const int G = (int)plan.groups.size();
        std::vector<int> order(G);
        std::vector<double> canvas_px(G);
        for (int g = 0; g < G; ++g) {
            const DetDims d = det_dims(plan.groups[g].H, plan.groups[g].W, pp.canvas_size, pp.mag_ratio);
            canvas_px[g] = (double)plan.groups[g].pages.size() * d.H32 * d.W32;
            order[g] = g;
        }
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return canvas_px[x] > canvas_px[y]; });
        // Every buffer of the detector side is sized HERE, before the first pass is queued: the arena and the resized pages for the
        // largest pass of any group, the heat-maps of all groups side by side, the CCL buffers for the largest pass, the staging buffers.
        std::vector<DetPlan> dp;
        std::vector<size_t> heat_off(G);
        std::vector<int> first(G);                                        // table index of the group's first page
        std::vector<int> inner;                                           // table index -> the caller's index: pages in pass order
        size_t arena = 0, resized = 0, heat_floats = 0, ccl_npx = 0;
        int ccl_comps = 0;
        for (int k = 0; k < G; ++k) {
            const PageGroup& gr = plan.groups[order[k]];
            dp.push_back(det_plan(ctx, (int)gr.pages.size(), gr.H, gr.W, pp, /*overlapped=*/k == G - 1));
            const DetDims& d = dp[k].d;
            arena = std::max(arena, dp[k].arena_bytes);
            resized = std::max(resized, dp[k].resized_bytes);
            heat_off[k] = heat_floats;
            heat_floats += gr.pages.size() * (size_t)d.h * d.w * 2;
            for (const int nb : dp[k].passes) {
                ccl_npx = std::max(ccl_npx, (size_t)nb * d.h * d.w);
                ccl_comps = std::max(ccl_comps, ccl_cap_comps(nb, d.h, d.w));
            }
            first[k] = (int)inner.size();
            inner.insert(inner.end(), gr.pages.begin(), gr.pages.end());
        }
        det_size(ctx, arena, resized);
        ctx->heat.ensure(heat_floats * sizeof(float));
        ccl_size(ctx, ccl_npx, ccl_comps);
        ctx->pg_rgb.ensure((size_t)plan.rgb_bytes);
        ctx->gray.ensure((size_t)plan.gray_bytes);
        std::vector<CropPage> crop_host;
        const PageTables tabs = upload_page_tables(ctx, pages, plan, inner, crop_host, (const uint8_t*)ctx->pg_rgb.p, (const uint8_t*)ctx->gray.p);
        HIPCHK(launch_pack_pages(tabs.pack, n, tabs.ntiles, (uint8_t*)ctx->pg_rgb.p, (uint8_t*)ctx->gray.p, ctx->stream));
        const GrayPages gp{(const uint8_t*)ctx->gray.p, 0, 0, crop_host.data(), tabs.crop};
        // the whole detector is queued, group after group, with no host wait: one event per pass
        struct Pass { int k, b0, nb; };
        std::vector<Pass> subs;
        if (!ctx->det_t0) { HIPCHK(hipEventCreate(&ctx->det_t0)); HIPCHK(hipEventCreate(&ctx->det_t1)); }
        HIPCHK(hipEventRecord(ctx->det_t0, ctx->stream));
        for (int k = 0; k < G; ++k)
            det_run(ctx, dp[k], (const uint8_t*)ctx->pg_rgb.p + plan.groups[order[k]].rgb_base, (float*)ctx->heat.p + heat_off[k], [&](int b0, int nb) {
                if (subs.size() >= ctx->sub_events.size()) {
                    hipEvent_t e;
                    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    ctx->sub_events.push_back(e);
                }
                HIPCHK(hipEventRecord(ctx->sub_events[subs.size()], ctx->stream));
                subs.push_back(Pass{k, b0, nb});
            });
        HIPCHK(hipEventRecord(ctx->det_t1, ctx->stream));
        HostBoxes hb;                                                     // indexed like the tables: pages in pass order
        hb.polys.resize(n); hb.hori.resize(n); hb.freeb.resize(n);
        RecEarly early;
        for (size_t s = 0; s < subs.size(); ++s) {
            const Pass& ps = subs[s];
            const DetDims& d = dp[ps.k].d;
            HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->sub_events[s], 0));
            HostBoxes part;
            boxes_impl(ctx, (const float*)ctx->heat.p + heat_off[ps.k] + (size_t)ps.b0 * d.h * d.w * 2, ps.nb, d.h, d.w, d.ratio, pp, part, ctx->stream2);
            const int at = first[ps.k] + ps.b0;
            for (int i = 0; i < ps.nb; ++i) {
                hb.polys[at + i] = std::move(part.polys[i]);
                hb.hori[at + i] = std::move(part.hori[i]);
                hb.freeb[at + i] = std::move(part.freeb[i]);
            }
            // as in bbocr_readtext_batch: the crops of every page but the last pass's go through the recogniser's conv stack while the
            // last pass's CCL + host geometry run
            if (subs.size() >= 2 && s + 2 == subs.size() && pp.rotation_info[0] == 0 && ctx->crnn_loaded)
                rec_early_begin(ctx, gp, at + ps.nb, n, hb, pp, early);
        }
        HIPCHK(hipEventSynchronize(ctx->det_t1));
        float det_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&det_ms, ctx->det_t0, ctx->det_t1));
        ctx->times[0] = det_ms;                                           // GPU span of the detector over all groups
        std::vector<BoxJob> jobs;
        std::vector<int> off;
        recognize_impl(ctx, gp, n, hb, pp, jobs, off, &early);
        prof_collect(ctx);
        // back to the caller's order
        std::vector<int> index_of(n);
        for (int k = 0; k < n; ++k) index_of[inner[k]] = k;
        std::vector<BoxJob> jobs2;
        std::vector<int> off2(n + 1, 0);
        jobs2.reserve(jobs.size());
        for (int i = 0; i < n; ++i) {
            const int k = index_of[i];
            for (int j = off[k]; j < off[k + 1]; ++j) jobs2.push_back(std::move(jobs[j]));
            off2[i + 1] = (int)jobs2.size();
        }
        *out = export_result(n, jobs2, off2);
        ctx->times[7] = (float)ms_since(t_all);
    });
}

}  // extern "C"
