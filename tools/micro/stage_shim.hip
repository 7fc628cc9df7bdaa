// Test-only shim (tests/test_gpu_stages.py): runs ONE stage of the detector / recogniser (fast modes, and the exact mode's split-fp16 stages)
// with the production plans and packed side tables of a live context, so that each fused launch can be compared with an fp64 reference of its own operation (tests/stage_ref.py).
// stage_rec_features runs any range of the stages of the recogniser's conv stack (crnn_features_stages, the function a recognition pass runs).
// stage_crops_wide runs the crop stage of a recognition pass into the wide layout (rec_launch_crops, the call rec_launch_part makes).
// stage_ctc_greedy runs the greedy CTC stage over a ragged sequence table (launch_ctc, the call rec_finish makes) into caller-owned tensors.
// No kernels of its own.  Built by the test as a shared object against the in-tree library:
//   hipcc -O2 -std=c++20 -shared -fPIC --offload-arch=gfx950 -Ibb-ocr_amd/csrc -Iinclude tools/micro/stage_shim.hip -Lbb-ocr_amd -lbbocr -o stage_shim.so
// Every function takes the bbocr_ctx* of a Reader, device pointers of caller-owned tensors with their element counts (checked against the
// shapes before anything is launched), runs on c->stream, waits for it and returns the hipError_t as an int (0 = success); a StatusError of the
// library comes back as SHIM_STATUS + |code|, anything else as SHIM_UNKNOWN, with the text in stage_shim_error().
#include "ctx.h"

namespace {
constexpr int SHIM_STATUS = 10000, SHIM_UNKNOWN = 19999, SHIM_BAD_ARGS = 20000;
std::string g_err;

template <typename F> int run_stage(bbocr_ctx* c, F&& f) {
    g_err.clear();
    if (!c) { g_err = "null context"; return SHIM_BAD_ARGS; }
    try {
        hipError_t e = hipSetDevice(c->cfg.device);
        if (e != hipSuccess) return (int)e;
        c->cur = c->stream;                       // the layer helpers launch on c->cur; outside a guarded() call nothing has set it
        e = f();
        const hipError_t s = hipStreamSynchronize(c->stream);
        return (int)(e != hipSuccess ? e : s);
    } catch (const StatusError& se) {
        g_err = se.msg;
        (void)hipStreamSynchronize(c->stream);
        return SHIM_STATUS + std::abs(se.code);
    } catch (const std::exception& ex) {
        g_err = ex.what();
        (void)hipStreamSynchronize(c->stream);
        return SHIM_UNKNOWN;
    } catch (...) {
        g_err = "unknown failure";
        (void)hipStreamSynchronize(c->stream);
        return SHIM_UNKNOWN;
    }
}

bool fast_detector(const bbocr_ctx* c) { return c->craft_loaded && !det_split(c); }
bool exact_detector(const bbocr_ctx* c) { return c->craft_loaded && det_split(c); }
size_t px(int N, int H, int W) { return (size_t)N * H * W; }
bool dims_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 26); }
#define NEED(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { g_err = "bad arguments: " #cond; return SHIM_BAD_ARGS; } \
    } while (0)

// what a stage carves from the context's arena: dry pass, arena.buf.ensure, real pass (as a detector pass does)
template <typename F> auto in_arena(bbocr_ctx* c, F&& stage) {
    c->arena.begin(true);
    (void)stage();
    c->arena.buf.ensure(c->arena.off);
    c->arena.begin(false);
    return stage();
}
// helper-allocated outputs live in the arena: a copy out
template <typename F> hipError_t with_arena(bbocr_ctx* c, uint16_t* out, size_t out_elems, F&& stage) {
    const Act o = in_arena(c, stage);
    if ((size_t)o.N * o.H * o.W * o.C != out_elems) fail(BBOCR_ERR_INTERNAL, "stage shim: output size differs from the caller's tensor");
    return hipMemcpyAsync(out, o.p, out_elems * 2, hipMemcpyDeviceToDevice, c->stream);
}

// the n crops of the given padded widths planned as one part, as bbocr_crnn_logits and a recognition pass plan theirs
bool rec_widths_ok(const int* widths, int n) {
    if (!widths || n <= 0 || n > 4096) return false;
    long long cols = 0;
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 64 || (widths[i] & 63) || widths[i] > 2560) return false;
        cols += widths[i] + REC_GAP;
    }
    return cols < (1LL << 20);
}
void rec_part_of(const int* widths, int n, RecPart& part) {
    std::vector<BoxJob> jobs(n);
    std::vector<int> all(n);
    for (int i = 0; i < n; ++i) { jobs[i].d = CropDesc{}; jobs[i].d.imgW = widths[i]; all[i] = i; }
    rec_plan_part(jobs, all, 0, 0, part);
}
// host only; 0 or the shim's status of what rec_plan_part threw (nothing crosses the extern "C" boundary)
int plan_part(const int* widths, int n, RecPart& part) {
    try {
        rec_part_of(widths, n, part);
        return 0;
    } catch (const StatusError& se) {
        g_err = se.msg;
        return SHIM_STATUS + std::abs(se.code);
    } catch (const std::exception& ex) {
        g_err = ex.what();
        return SHIM_UNKNOWN;
    } catch (...) {
        g_err = "unknown failure";
        return SHIM_UNKNOWN;
    }
}
size_t act_elems(const Act& a) { return (size_t)a.N * a.H * a.W * a.C; }

// the boxes of ONE H x W page (hori [n_hori][4], then free_q [n_free][4][2]) planned as a recognition pass plans them: plan_horizontal /
// plan_free (a skipped box leaves no job; box[i] = position of job i in the caller's list), scratch offsets, all of them one part
struct CropPlan {
    std::vector<BoxJob> jobs;
    std::vector<int> box;
    RecPart part;
    size_t a_total = 0, w_total = 0;
};
bool crop_boxes_ok(int H, int W, const int* hori, int n_hori, const double* free_q, int n_free) {
    return dims_ok(1, H, W) && n_hori >= 0 && n_free >= 0 && n_hori + n_free > 0 && n_hori + n_free <= 4096 && (hori || !n_hori) && (free_q || !n_free);
}
int plan_crops(int H, int W, const int* hori, int n_hori, const double* free_q, int n_free, CropPlan& p) {
    try {
        for (int i = 0; i < n_hori + n_free; ++i) {
            BoxJob j;
            bool taken;
            if (i < n_hori) {
                std::array<int, 4> b;
                memcpy(b.data(), hori + (size_t)i * 4, 16);
                taken = plan_horizontal(b, 0, H, W, j);
            } else {
                std::array<double, 8> f;
                memcpy(f.data(), free_q + (size_t)(i - n_hori) * 8, 64);
                taken = plan_free(f, 0, j);
            }
            if (!taken) continue;
            p.jobs.push_back(j);
            p.box.push_back(i);
        }
        rec_layout_scratch(p.jobs, 0, p.a_total, p.w_total);
        std::vector<int> all(p.jobs.size());
        for (size_t i = 0; i < all.size(); ++i) all[i] = (int)i;
        rec_plan_part(p.jobs, all, 0, 0, p.part);
        return 0;
    } catch (const StatusError& se) {
        g_err = se.msg;
        return SHIM_STATUS + std::abs(se.code);
    } catch (const std::exception& ex) {
        g_err = ex.what();
        return SHIM_UNKNOWN;
    } catch (...) {
        g_err = "unknown failure";
        return SHIM_UNKNOWN;
    }
}
}  // namespace

extern "C" {

const char* stage_shim_error() { return g_err.c_str(); }
int stage_shim_det_el(bbocr_ctx* c) { return c ? det_el(c) : -1; }
int stage_shim_rec_el(bbocr_ctx* c) { return c ? rec_el(c) : -1; }
int stage_shim_xproj_channel(int dir, int gate, int unit) { return lstm8_xproj_channel(dir, gate, unit); }
int stage_shim_tile_seqs(bbocr_ctx* c) { return c ? lstm_tile_seqs(rec_mode(c)) : -1; }

// normalise + conv1_1 + ReLU produced in conv1_2's prologue, conv1_2 + BN + ReLU, 2x2 max-pool: rgb uint8 [N, Himg, Wimg, 3] on the zero
// canvas H32 x W32 -> out [N, H32/2, W32/2, 64]
int stage_c11_conv1_2_pool(bbocr_ctx* c, const uint8_t* rgb, size_t rgb_elems, int N, int Himg, int Wimg, int H32, int W32, uint16_t* out, size_t out_elems) {
    NEED(c && fast_detector(c) && rgb && out && dims_ok(N, H32, W32) && Himg > 0 && Wimg > 0 && Himg <= H32 && Wimg <= W32 && H32 % 32 == 0 && W32 % 32 == 0);
    NEED(rgb_elems == px(N, Himg, Wimg) * 3 && out_elems == px(N, H32 / 2, W32 / 2) * 64);
    return run_stage(c, [&] {
        return with_arena(c, out, out_elems, [&] {
            const Act canvas{nullptr, N, H32, W32, 64};
            const RgbSource src{rgb, Himg, Wimg};
            return conv_pool_act(c, c->conv1_2, canvas, false, true, 64, 1, false, nullptr, &src);
        });
    });
}

// upconv1's 1x1 over the virtual concat [fc7 (1024) | relu5_3 (512)] + BN + ReLU -> out [N, H, W, 512]
int stage_up1a(bbocr_ctx* c, const uint16_t* f7, size_t f7_elems, const uint16_t* s4, size_t s4_elems, int N, int H, int W, uint16_t* out, size_t out_elems) {
    NEED(c && fast_detector(c) && f7 && s4 && out && dims_ok(N, H, W));
    NEED(f7_elems == px(N, H, W) * 1024 && s4_elems == px(N, H, W) * 512 && out_elems == px(N, H, W) * 512);
    return run_stage(c, [&] {
        return with_arena(c, out, out_elems, [&] {
            const Act a0{(uint16_t*)f7, N, H, W, 1024}, a1{(uint16_t*)s4, N, H, W, 512};
            return conv_act(c, c->up1a, a0, false, &a1, false, true, 512);
        });
    });
}

// fc6 -> fc7 -> upconv1's 1x1 over cat[fc7, relu5_3] + BN + ReLU as the folded stage (craft_fc_stage: the dilated 3x3 512 -> 512 into z, then the
// skip half of the 1x1 with z added in its epilogue): p5 [N, H, W, 512] (the pooled relu5_3), s4 [N, H, W, 512] -> out [N, H, W, 512]
int stage_fc_fold(bbocr_ctx* c, const uint16_t* p5, size_t p5_elems, const uint16_t* s4, size_t s4_elems, int N, int H, int W, uint16_t* out, size_t out_elems) {
    NEED(c && fast_detector(c) && p5 && s4 && out && dims_ok(N, H, W));
    NEED(p5_elems == px(N, H, W) * 512 && s4_elems == p5_elems && out_elems == p5_elems);
    return run_stage(c, [&] {
        const Act a{(uint16_t*)p5, N, H, W, 512}, k{(uint16_t*)s4, N, H, W, 512};
        in_arena(c, [&] {
            const Act z{c->arena.alloc<uint16_t>(px(N, H, W) * 512), N, H, W, 512};
            craft_fc_stage(c, a, k, z.p, out);
            return z;
        });
        return hipSuccess;
    });
}

// the second launch of craft_fc_stage alone: s4 [N, H, W, 512], z [N, H, W, 512] -> out [N, H, W, 512] = ReLU(z + W_s s4 + b')
int stage_addsame(bbocr_ctx* c, const uint16_t* s4, size_t s4_elems, const uint16_t* z, size_t z_elems, int N, int H, int W, uint16_t* out, size_t out_elems) {
    NEED(c && fast_detector(c) && s4 && z && out && dims_ok(N, H, W));
    NEED(s4_elems == px(N, H, W) * 512 && z_elems == s4_elems && out_elems == s4_elems);
    return run_stage(c, [&] {
        c->arena.begin(false);                    // run_conv is a no-op in a dry pass; nothing is carved from the arena here
        const Act sk{(uint16_t*)s4, N, H, W, 512}, zz{(uint16_t*)z, N, H, W, 512};
        run_conv(c, c->up1s, sk, false, nullptr, false, true, out, 512, 512, false, nullptr, &zz);
        return hipSuccess;
    });
}

// Dry run of that launch (launch_conv's dispatch up to its terminal, nothing is launched and no pointer is followed) with an addend declared as
// [N, zH, zW, zC]: returns the hipError_t of the dispatch -- hipErrorInvalidValue unless z is N * H * W x 512 -- and the route it reports
// (id and the `addup` field of ConvRoute).
int stage_addsame_route(bbocr_ctx* c, int N, int H, int W, int zH, int zW, int zC, int* route_id, int* route_addup) {
    g_err.clear();
    NEED(c && fast_detector(c) && dims_ok(N, H, W) && zH > 0 && zW > 0 && zC > 0 && route_id && route_addup);
    uint16_t* const nowhere = (uint16_t*)c->zero_page;       // a dry run only tests pointers for null
    const Act sk{nowhere, N, H, W, 512}, zz{nowhere, N, zH, zW, zC};
    ConvArgs a = conv_args(c->up1s, sk, nullptr, nullptr, &zz);
    a.relu_out = 1; a.out = nowhere; a.out_cs = 512; a.cout_store = 512; a.zero = c->zero_page;
    ConvRoute r{};
    const hipError_t e = launch_conv(c->up1s, a, c->stream, &r, true);
    *route_id = r.id;
    *route_addup = r.addup;
    return (int)e;
}

// the skip half of a U-net 1x1 with up(z) added in its epilogue (craft_up_stage's second launch; level 4: the first launch of
// craft_up4's two-launch path): skip [N, H, W, Cs], z [N, H/2, W/2, cout] -> out [N, H, W, cout] = ReLU(up(z) + W_s skip + b)
int stage_addup(bbocr_ctx* c, int level, const uint16_t* skip, size_t skip_elems, const uint16_t* z, size_t z_elems, int N, int H, int W, uint16_t* out,
                size_t out_elems) {
    NEED(c && fast_detector(c) && skip && z && out && dims_ok(N, H, W) && H % 2 == 0 && W % 2 == 0 && level >= 2 && level <= 4);
    const ConvPlan& ps = level == 2 ? c->up2s : (level == 3 ? c->up3s : c->up4s);
    const int Cs = ps.Cin, cout = ps.Cout;
    NEED(skip_elems == px(N, H, W) * Cs && z_elems == px(N, H / 2, W / 2) * cout && out_elems == px(N, H, W) * cout);
    return run_stage(c, [&] {
        c->arena.begin(false);                    // run_conv is a no-op in a dry pass; nothing is carved from the arena here
        const Act sk{(uint16_t*)skip, N, H, W, Cs}, zz{(uint16_t*)z, N, H / 2, W / 2, cout};
        run_conv(c, ps, sk, false, nullptr, false, true, out, cout, cout, false, &zz);
        return hipSuccess;
    });
}

// upconv3's 3x3 + BN + ReLU with z = W_y u3b (upconv4's y-half 1x1) applied in the epilogue: u3a [N, H, W, 128] -> z [N, H, W, 64]
int stage_up3b_post(bbocr_ctx* c, const uint16_t* u3a, size_t u3a_elems, int N, int H, int W, uint16_t* z, size_t z_elems) {
    NEED(c && fast_detector(c) && c->up4y_post && u3a && z && dims_ok(N, H, W));
    NEED(u3a_elems == px(N, H, W) * 128 && z_elems == px(N, H, W) * 64);
    return run_stage(c, [&] {
        // hipErrorNotSupported: the fused launch was declined and the two launches ran (through u3b in the arena), as in a detector pass
        const Act a{(uint16_t*)u3a, N, H, W, 128};
        return in_arena(c, [&] { return craft_up3b_post(c, a, c->arena.alloc<uint16_t>(px(N, H, W) * 64), z); }) ? hipSuccess : hipErrorNotSupported;
    });
}

// upconv4 as one launch: s1 [N, H, W, 128], z [N, H/2, W/2, 64] -> u4b [N, H, W, 32]
int stage_up4_fused(bbocr_ctx* c, const uint16_t* s1, size_t s1_elems, const uint16_t* z, size_t z_elems, int N, int H, int W, uint16_t* u4b, size_t u4b_elems) {
    NEED(c && fast_detector(c) && s1 && z && u4b && dims_ok(N, H, W) && H % 2 == 0 && W % 2 == 0);
    NEED(s1_elems == px(N, H, W) * 128 && z_elems == px(N, H / 2, W / 2) * 64 && u4b_elems == px(N, H, W) * 32);
    return run_stage(c, [&] {
        const Act a{(uint16_t*)s1, N, H, W, 128};
        return in_arena(c, [&] { return craft_up4(c, a, z, u4b); }) ? hipSuccess : hipErrorNotSupported;      // as above
    });
}

// conv_cls.4 (3x3 32 -> 16 + ReLU) with conv_cls.6 / .8 in its epilogue: c2 [N, H, W, 32] -> heat fp32 [N, H, W, 2]
int stage_cls_tail(bbocr_ctx* c, const uint16_t* c2, size_t c2_elems, int N, int H, int W, float* heat, size_t heat_elems) {
    NEED(c && fast_detector(c) && c->cls_tail && c->cls_tail_frag && c2 && heat && dims_ok(N, H, W));
    NEED(c2_elems == px(N, H, W) * 32 && heat_elems == px(N, H, W) * 2);
    return run_stage(c, [&] {
        c->arena.begin(false);                    // nothing is carved from the arena here
        craft_cls_tail(c, Act{(uint16_t*)c2, N, H, W, 32}, heat);
        return hipSuccess;
    });
}

// pool5 = MaxPool2d(3, 1, 1) without ReLU: in [N, H, W, 512] -> out [N, H, W, 512]
int stage_pool5(bbocr_ctx* c, const uint16_t* in, size_t in_elems, int N, int H, int W, uint16_t* out, size_t out_elems) {
    NEED(c && in && out && dims_ok(N, H, W) && in_elems == px(N, H, W) * 512 && out_elems == in_elems);
    return run_stage(c, [&] {
        return with_arena(c, out, out_elems, [&] {
            const Act a{(uint16_t*)in, N, H, W, 512};
            return pool_act(c, a, 3, 3, 1, 1, 1, 1, false);
        });
    });
}

// ------------------------------------------------------------------------------------------------ exact mode (split-fp16 plans, pair tensors)
// The stage functions and the conv table of craft_forward_exact (detector.cpp) on a live exact context.  Pair tensors [.., C | C] are passed
// with BOTH halves counted in their element counts.
int stage_exact_rows() { return craft_exact_rows(); }
// row of the table: name (up to 15 characters) and {logical Cin, relu_out, store, pool mode, pool_relu, keep_full, K, dilation}
int stage_exact_row_info(bbocr_ctx* c, int row, char* name16, int* info8) {
    g_err.clear();
    NEED(c && exact_detector(c) && name16 && info8 && row >= 0 && row < craft_exact_rows());
    const ExactConvRow& r = craft_exact_row(row);
    const ConvPlan& p = c->*(r.plan);
    NEED(p.split && p.KH == p.KW);
    snprintf(name16, 16, "%s", r.name);
    const int v[8] = {p.Cin / 3, r.relu_out, r.store, r.pool_mode, r.pool_relu, r.keep_full, p.KH, p.dil};
    std::copy(v, v + 8, info8);
    return 0;
}

// row `row` on the pair tensor in [N, H, W, Cin | Cin] -> out: the row's (pooled, if it pools) output pair; full: the un-pooled pair of a
// row that keeps it (null / 0 otherwise)
int stage_exact_conv(bbocr_ctx* c, int row, const uint16_t* in, size_t in_elems, int N, int H, int W, uint16_t* out, size_t out_elems, uint16_t* full,
                     size_t full_elems) {
    NEED(c && exact_detector(c) && in && out && dims_ok(N, H, W) && row >= 0 && row < craft_exact_rows());
    const ExactConvRow& r = craft_exact_row(row);
    const ConvPlan& p = c->*(r.plan);
    NEED(p.split && in_elems == px(N, H, W) * 2 * (size_t)(p.Cin / 3));
    const int OH = H + 2 * p.pad_h - (p.KH - 1) * p.dil, OW = W + 2 * p.pad_w - (p.KW - 1) * p.dil;
    NEED(OH > 0 && OW > 0 && (!r.pool_mode || (OH % 2 == 0 && OW % 2 == 0)));
    NEED(out_elems == (r.pool_mode ? px(N, OH / 2, OW / 2) : px(N, OH, OW)) * 2 * (size_t)r.store);
    NEED(r.keep_full ? (full && full_elems == px(N, OH, OW) * 2 * (size_t)r.store) : (!full && !full_elems));
    return run_stage(c, [&] {
        Act f{};
        const Act a{(uint16_t*)in, N, H, W, 2 * (p.Cin / 3)};
        const hipError_t e = with_arena(c, out, out_elems, [&] { return craft_exact_conv(c, row, a, r.keep_full ? &f : nullptr); });
        if (e != hipSuccess || !r.keep_full) return e;
        if (act_elems(f) != full_elems) fail(BBOCR_ERR_INTERNAL, "stage shim: full output size differs from the caller's tensor");
        return hipMemcpyAsync(full, f.p, full_elems * 2, hipMemcpyDeviceToDevice, c->stream);
    });
}

// normalise + conv1_1 + BN + ReLU in fp32: rgb uint8 [N, Himg, Wimg, 3] on the zero canvas H32 x W32 -> out pair [N, H32, W32, 64 | 64]
int stage_exact_conv1_1(bbocr_ctx* c, const uint8_t* rgb, size_t rgb_elems, int N, int Himg, int Wimg, int H32, int W32, uint16_t* out, size_t out_elems) {
    NEED(c && exact_detector(c) && rgb && out && dims_ok(N, H32, W32) && Himg > 0 && Wimg > 0 && Himg <= H32 && Wimg <= W32);
    NEED(rgb_elems == px(N, Himg, Wimg) * 3 && out_elems == px(N, H32, W32) * 128);
    return run_stage(c, [&] { return with_arena(c, out, out_elems, [&] { return craft_exact_conv1_1(c, rgb, N, Himg, Wimg, H32, W32); }); });
}

// ReLU on the pair values: in / out [N, H, W, C | C]
int stage_exact_relu(bbocr_ctx* c, const uint16_t* in, size_t in_elems, int N, int H, int W, int C, uint16_t* out, size_t out_elems) {
    NEED(c && exact_detector(c) && in && out && dims_ok(N, H, W) && C > 0 && C % 8 == 0 && in_elems == px(N, H, W) * 2 * (size_t)C && out_elems == in_elems);
    return run_stage(c, [&] { return with_arena(c, out, out_elems, [&] { return craft_exact_relu(c, Act{(uint16_t*)in, N, H, W, 2 * C}); }); });
}

// MaxPool2d(3, 1, 1) on the pair values: in / out [N, H, W, C | C]
int stage_exact_pool5(bbocr_ctx* c, const uint16_t* in, size_t in_elems, int N, int H, int W, int C, uint16_t* out, size_t out_elems) {
    NEED(c && exact_detector(c) && in && out && dims_ok(N, H, W) && C > 0 && C % 8 == 0 && in_elems == px(N, H, W) * 2 * (size_t)C && out_elems == in_elems);
    return run_stage(c, [&] { return with_arena(c, out, out_elems, [&] { return craft_exact_pool5(c, Act{(uint16_t*)in, N, H, W, 2 * C}); }); });
}

// cat([interpolate(y), skip]): y pair [N, yh, yw, Cy | Cy] (the skip's size, or half of it), skip pair [N, H, W, Cs | Cs] -> out pair [N, H, W, Cy + Cs | Cy + Cs]
int stage_exact_upcat(bbocr_ctx* c, const uint16_t* y, size_t y_elems, int yh, int yw, int Cy, const uint16_t* skip, size_t skip_elems, int Cs, int N, int H,
                      int W, uint16_t* out, size_t out_elems) {
    NEED(c && exact_detector(c) && y && skip && out && dims_ok(N, H, W) && Cy > 0 && Cs > 0 && Cy % 8 == 0 && Cs % 8 == 0);
    NEED((yh == H && yw == W) || (2 * yh == H && 2 * yw == W));
    NEED(y_elems == px(N, yh, yw) * 2 * (size_t)Cy && skip_elems == px(N, H, W) * 2 * (size_t)Cs && out_elems == px(N, H, W) * 2 * (size_t)(Cy + Cs));
    return run_stage(c, [&] {
        return with_arena(c, out, out_elems, [&] { return craft_exact_upcat(c, Act{(uint16_t*)y, N, yh, yw, 2 * Cy}, Act{(uint16_t*)skip, N, H, W, 2 * Cs}); });
    });
}

// conv_cls.6 + ReLU + conv_cls.8 in fp32: c3 pair [N, H, W, 16 | 16] -> heat fp32 [N, H, W, 2]
int stage_exact_cls_tail(bbocr_ctx* c, const uint16_t* c3, size_t c3_elems, int N, int H, int W, float* heat, size_t heat_elems) {
    NEED(c && exact_detector(c) && c3 && heat && dims_ok(N, H, W) && c3_elems == px(N, H, W) * 32 && heat_elems == px(N, H, W) * 2);
    return run_stage(c, [&] {
        c->arena.begin(false);                    // nothing is carved from the arena here
        craft_exact_cls_tail(c, Act{(uint16_t*)c3, N, H, W, 32}, heat);
        return hipSuccess;
    });
}

// One GEMM of the sequence half (crnn_sequence's own helpers) on a live exact context, rows_pad rows (a multiple of 256):
// which 0: xproj[layer], x pair [rows_pad, 256 | 256] -> fp32 [rows_pad, 2048];  1: lin[layer], h pair [rows_pad, 512 | 512] with the lo
// half UNSCALED -> pair [rows_pad, 256 | 256];  2: pred, x pair [rows_pad, 256 | 256] -> fp32 [rows_pad, 112]
int stage_exact_seq_gemm(bbocr_ctx* c, int which, int layer, const uint16_t* in, size_t in_elems, size_t rows_pad, void* out, size_t out_elems) {
    NEED(c && c->crnn_loaded && rec_split(c) && !rec_quant(c) && which >= 0 && which <= 2 && (layer == 0 || layer == 1) && in && out);
    NEED(rows_pad > 0 && rows_pad % 256 == 0 && rows_pad < ((size_t)1 << 22));
    NEED(in_elems == rows_pad * (which == 1 ? 1024 : 512) && out_elems == rows_pad * (which == 0 ? 2048 : (which == 1 ? 512 : 112)));
    return run_stage(c, [&] {
        c->arena.begin(false);                    // run_conv is a no-op in a dry pass; nothing is carved from the arena here
        if (which == 0) crnn_seq_xproj(c, layer, in, rows_pad, out);
        else if (which == 1) crnn_seq_lin(c, layer, in, rows_pad, (uint16_t*)out);
        else crnn_seq_pred(c, in, rows_pad, (float*)out);
        return hipSuccess;
    });
}

// BiLSTM recurrence of layer l over a tile table given on the HOST (int4 {first row, sequences, T, 0} per workgroup): xproj [rows_pad, 2048]
// in the permuted channel order, out [rows_pad, 512] (fwd | bwd).  rows_pad: a multiple of 256, as the sequence stage allocates.
// Exact mode: xproj is FP32 [rows_pad, 2048] and out the pair [rows_pad, 512 | 512] with the lo half unscaled (twice the bytes each).
int stage_lstm(bbocr_ctx* c, int layer, const void* xproj, uint16_t* out, size_t rows_pad, const int* tiles_host, int ntiles) {
    NEED(c && c->crnn_loaded && !rec_quant(c) && (layer == 0 || layer == 1) && c->whh[layer] && xproj && out && tiles_host && ntiles > 0 && ntiles <= 65535);
    NEED(rows_pad > 0 && rows_pad % 256 == 0 && rows_pad < ((size_t)1 << 24));
    const int cap = lstm_tile_seqs(rec_mode(c));
    for (int i = 0; i < ntiles; ++i) {
        const int row0 = tiles_host[4 * i], n = tiles_host[4 * i + 1], T = tiles_host[4 * i + 2];
        NEED(row0 >= 0 && n >= 1 && n <= cap && T >= 1 && (size_t)row0 + (size_t)n * T <= rows_pad);
    }
    return run_stage(c, [&] {
        int* tiles_dev = nullptr;
        HIPCHK(hipMalloc((void**)&tiles_dev, (size_t)ntiles * 16));
        hipError_t e = hipMemcpy(tiles_dev, tiles_host, (size_t)ntiles * 16, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_lstm(xproj, c->whh[layer], out, tiles_dev, ntiles, rec_mode(c), c->whh_scale[layer], c->stream);
        const hipError_t s = hipStreamSynchronize(c->stream);
        (void)hipFree(tiles_dev);
        return e != hipSuccess ? e : s;
    });
}

// rec_plan_part on n crops of the given padded widths (host only).  Per descriptor k of the plan: its first column in the wide image, its
// first pooled row, and the position in `widths` of the crop it stands for; cols / rows: the part's totals.
int stage_rec_plan(const int* widths, int n, int* slot_out, int* row0_out, int* order_out, int* cols, int* rows) {
    g_err.clear();
    NEED(rec_widths_ok(widths, n) && slot_out && row0_out && order_out && cols && rows);
    RecPart part;
    if (const int rc = plan_part(widths, n, part)) return rc;
    NEED((int)part.descs.size() == n && (int)part.order.size() == n);
    for (int k = 0; k < n; ++k) {
        slot_out[k] = part.descs[k].slot;
        row0_out[k] = part.descs[k].pad_;
        order_out[k] = part.order[k];
    }
    *cols = (int)part.cols;
    *rows = (int)part.rows;
    return 0;
}

// Stages first..last of the recogniser's conv stack (crnn_features_stages) over the part planned from `widths`: `in` is the input of stage
// `first` in the wide layout (crnn_stage_shape; stage 0: [64][cols] element-type pixels, exact mode: codes 1 + grey; gap columns zero),
// `out` receives the output of stage `last`.  After stage 7 that is seq_v: `out` is [R][256 * m] with R >= the part's rows, its content goes
// into seq_v first and all R rows come back, so rows the gather did not write keep what the caller put there.
int stage_rec_features(bbocr_ctx* c, const int* widths, int n, int first, int last, const uint16_t* in, size_t in_elems, uint16_t* out, size_t out_elems) {
    g_err.clear();
    NEED(c && c->crnn_loaded && in && out && rec_widths_ok(widths, n) && first >= 0 && first <= last && last < REC_STAGES);
    RecPart part;
    if (const int rc = plan_part(widths, n, part)) return rc;
    const bool to_seq = last == REC_STAGES - 1;
    const Act ia = crnn_stage_shape(c, part, first), oa = crnn_stage_shape(c, part, last + 1);
    NEED(in_elems == act_elems(ia));
    NEED(to_seq ? (out_elems >= act_elems(oa) && out_elems % (size_t)oa.C == 0 && out_elems < ((size_t)1 << 28)) : out_elems == act_elems(oa));
    return run_stage(c, [&] {
        const CropDesc* dd = rec_upload_descs(c, part, c->crop_desc);
        if (to_seq) {
            c->seq_v.ensure(align_up(out_elems / (size_t)oa.C, 256) * (size_t)oa.C * 2);
            HIPCHK(hipMemcpyAsync(c->seq_v.p, out, out_elems * 2, hipMemcpyDeviceToDevice, c->stream));
        }
        Act a = ia;
        a.p = (uint16_t*)in;
        const Act o = in_arena(c, [&] { return crnn_features_stages(c, part, dd, a, first, last); });
        if (!to_seq && act_elems(o) != out_elems) fail(BBOCR_ERR_INTERNAL, "stage shim: output size differs from the caller's tensor");
        return hipMemcpyAsync(out, o.p, out_elems * 2, hipMemcpyDeviceToDevice, c->stream);
    });
}

// The wide layout of the crops of one page's boxes (host only).  Per descriptor k of the part, in the order they stand in the wide image: the
// position of its box in the caller's list (hori, then free_q), its first column and its padded width; n: descriptors (boxes not skipped);
// cols: columns of the wide image.  The three arrays hold n_hori + n_free entries.
int stage_crops_wide_plan(int H, int W, const int* hori, int n_hori, const double* free_q, int n_free, int* box_out, int* slot_out, int* imgw_out, int* n,
                          int* cols) {
    g_err.clear();
    NEED(crop_boxes_ok(H, W, hori, n_hori, free_q, n_free) && box_out && slot_out && imgw_out && n && cols);
    CropPlan p;
    if (const int rc = plan_crops(H, W, hori, n_hori, free_q, n_free, p)) return rc;
    for (size_t k = 0; k < p.part.descs.size(); ++k) {
        box_out[k] = p.box[p.part.order[k]];
        slot_out[k] = p.part.descs[k].slot;
        imgw_out[k] = p.part.descs[k].imgW;
    }
    *n = (int)p.part.descs.size();
    *cols = (int)p.part.cols;
    return 0;
}

// The crop stage of a recognition pass over that plan: gray uint8 [H][W] -> stage A (gather / warp + cv2 resize) into the context's crop
// scratch, contrast > 0: adjust_contrast_grey's LUTs as the contrast retry derives them, stage B (AlignCollate) into `wide` [64][cols] in the
// context's recogniser mode.  Only the columns of the crops and the REC_GAP columns after each are written.
int stage_crops_wide(bbocr_ctx* c, const uint8_t* gray, size_t gray_elems, int H, int W, const int* hori, int n_hori, const double* free_q, int n_free,
                     double contrast, uint16_t* wide, size_t wide_elems) {
    g_err.clear();
    NEED(c && c->crnn_loaded && gray && wide && crop_boxes_ok(H, W, hori, n_hori, free_q, n_free) && gray_elems == px(1, H, W) && contrast >= 0);
    CropPlan p;
    if (const int rc = plan_crops(H, W, hori, n_hori, free_q, n_free, p)) return rc;
    NEED(!p.part.descs.empty() && p.part.cols < ((size_t)1 << 20) && wide_elems == (size_t)64 * p.part.cols);
    std::vector<uint8_t> luts;                    // the source of an asynchronous copy: lives until run_stage has waited for the stream
    return run_stage(c, [&] {
        c->crop_scratch.ensure(std::max<size_t>(p.a_total, 16));
        c->crop_hscratch.ensure(std::max<size_t>(p.a_total, 16));
        c->crop_wscratch.ensure(std::max<size_t>(p.w_total, 16));
        c->crop_luts.ensure(256);
        const GrayPages g{gray, H, W};
        const CropDesc* dd = rec_upload_descs(c, p.part, c->crop_desc);
        rec_launch_crops(c, g, p.part, dd, nullptr, 1);
        if (contrast > 0 && !crop_contrast_luts(c, dd, p.part.descs, contrast, luts).empty()) {
            c->crop_luts.ensure(luts.size());
            HIPCHK(hipMemcpyAsync(c->crop_luts.p, luts.data(), luts.size(), hipMemcpyHostToDevice, c->stream));
            dd = rec_upload_descs(c, p.part, c->crop_desc);          // the descriptors with their lut_off (the first upload has been waited for)
        }
        rec_launch_crops(c, g, p.part, dd, wide, 2);
        return hipSuccess;
    });
}

// The greedy CTC stage as a recognition pass launches it (rec_finish): the ragged table seqs_host = nseq x {first row, T} goes into the
// context's seq_tables, then ONE launch_ctc over logits fp32 [rows, cs] (C classes per row) on c->stream.  Everything it writes is the caller's:
// idx / pmax / out_idx [rows], ctc_out int32 [>= 4 * nseq] (CtcOut = {len, cnt, prod, pad} per sequence), probs [rows, cs] or null (the
// greedy route keeps no probabilities).  mask4: the 4 x 32-bit class mask or null.  T = 0 is a sequence; one that leaves [0, rows) is refused
// before anything is queued.  C > 128 is launch_ctc's own refusal (hipErrorInvalidValue, nothing launched).
int stage_ctc_greedy(bbocr_ctx* c, const float* logits, size_t logits_elems, int rows, int C, int cs, const int* seqs_host, int nseq,
                     const unsigned int* mask4, int* idx, size_t idx_elems, float* pmax, size_t pmax_elems, int* out_idx, size_t out_idx_elems, int* ctc_out,
                     size_t ctc_out_elems, float* probs, size_t probs_elems) {
    g_err.clear();
    NEED(c && logits && seqs_host && idx && pmax && out_idx && ctc_out && rows > 0 && rows < (1 << 24) && nseq > 0 && nseq < (1 << 20) && C > 0 && C <= cs && cs <= 4096);
    NEED(logits_elems == (size_t)rows * cs && idx_elems == (size_t)rows && pmax_elems == (size_t)rows && out_idx_elems == (size_t)rows);
    NEED(ctc_out_elems >= (size_t)nseq * (sizeof(CtcOut) / 4) && (probs ? probs_elems == (size_t)rows * cs : probs_elems == 0));
    for (int i = 0; i < nseq; ++i) {
        const long long first = seqs_host[2 * i], T = seqs_host[2 * i + 1];
        NEED(first >= 0 && T >= 0 && first + T <= rows);
    }
    return run_stage(c, [&] {
        c->seq_tables.ensure((size_t)nseq * 8);
        int* seqs_dev = (int*)c->seq_tables.p;
        HIPCHK(hipMemcpyAsync(seqs_dev, seqs_host, (size_t)nseq * 8, hipMemcpyHostToDevice, c->stream));     // run_stage waits for the stream
        return launch_ctc(logits, (size_t)rows, C, cs, seqs_dev, nseq, idx, pmax, out_idx, (CtcOut*)ctc_out, c->stream, mask4, probs);
    });
}

// the confidence a recognition pass derives from one CtcOut (ctc_decode: the host pow)
double stage_ctc_decode(int len, int cnt, float prod) {
    const CtcOut o{len, cnt, prod, 0};
    std::vector<int> text;
    return ctc_decode(o, nullptr, 0, text);
}

}  // extern "C"
