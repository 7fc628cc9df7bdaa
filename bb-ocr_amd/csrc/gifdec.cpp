// GIF decoding, host side: the plan (gif_parse.h's walk, which de-frames the payload), a batch's admission, its one staged blob -- file
// descriptors, payloads, tables -- and the launch sequence of gifdec.hip.  A batch runs on the decode lane's stream of the root context,
// outside the call slots, with the lane's buffers (the contract of bbocr_jpeg_decode): files decode while two OCR calls run.
#include "ctx.h"
#include "gif_parse.h"
#include "gifdec.h"

namespace {

using namespace gif_host;

struct GifJob {                                // one admitted file of a batch
    GifParsed ps;
    int k = 0;                                 // its index in the caller's arrays
    uint8_t *rgb = nullptr, *gray = nullptr;   // null: no planes (the stage entry point, which does not run the output launch)
    long long pitch_rgb = 0, pitch_gray = 0;
    size_t cap = 0, o_payload = 0, o_table = 0, w_head = 0, w_lengths = 0, w_errors = 0, w_offsets = 0, w_stream = 0;
};

size_t frame_bytes(const bbocr_gif_plan& pl) { return (size_t)pl.width * (size_t)pl.height; }
size_t canvas_pixels(const bbocr_gif_plan& pl) { return (size_t)pl.canvas_w * (size_t)pl.canvas_h; }

// The decode of the admitted jobs up to `launches` launches (1: scan .. 5: output) on the lane's stream.  Fills dev_status[i] (the
// GIFL_ERR_* bits of job i; before the offsets launch: the scan's) and, for the stage entry point, the descriptors.  Everything queued is
// finished on return.
// launch_ms (bbocr_gif_decode_timed): the five launches' times between events on the stream.
void gif_run(bbocr_ctx* root, hipStream_t st, std::vector<GifJob>& jobs, int launches, std::vector<int>& dev_status, std::vector<GdDesc>* descs_out = nullptr,
             float* launch_ms = nullptr) {
    const int n = (int)jobs.size();
    const size_t status_bytes = align_up(4 * (size_t)n, 256);
    const size_t desc_bytes = align_up(sizeof(GdDesc) * (size_t)n, 256);
    Carve in{desc_bytes}, work{status_bytes};
    unsigned long long max_pixels = 1;
    size_t max_cap = 1;
    for (GifJob& j : jobs) {
        const bbocr_gif_plan& pl = j.ps.plan;
        j.cap = gifl_piece_room((uint64_t)pl.payload_bytes, pl.min_code);
        j.o_payload = in.add(j.ps.payload.size() + 8);
        j.o_table = in.add(768);
        j.w_head = work.add(16 + sizeof(GiflPiece) * j.cap);         // the piece table behind its head: one piece of memory for stage 0
        j.w_lengths = work.add(4 * j.cap);
        j.w_errors = work.add(4 * j.cap);
        j.w_offsets = work.add(4 * (j.cap + 1));
        j.w_stream = work.add(frame_bytes(pl));
        max_pixels = std::max(max_pixels, (unsigned long long)canvas_pixels(pl));
        max_cap = std::max(max_cap, j.cap);
    }
    root->jd_pin.ensure(in.off);
    root->jd_in.ensure(in.off);
    root->jd_work.ensure(work.off);
    char* hb = (char*)root->jd_pin.p;
    char* db = (char*)root->jd_in.p;
    char* wb = (char*)root->jd_work.p;
    GdDesc* descs = (GdDesc*)hb;
    for (int i = 0; i < n; ++i) {
        GifJob& j = jobs[i];
        const bbocr_gif_plan& pl = j.ps.plan;
        if (!j.ps.payload.empty()) std::memcpy(hb + j.o_payload, j.ps.payload.data(), j.ps.payload.size());
        std::memcpy(hb + j.o_table, pl.table, 768);
        GdDesc d{};
        d.payload = (const uint8_t*)(db + j.o_payload);
        d.table = (const uint8_t*)(db + j.o_table);
        d.head = (uint32_t*)(wb + j.w_head);
        d.pieces = (GiflPiece*)(wb + j.w_head + 16);
        d.lengths = (uint32_t*)(wb + j.w_lengths);
        d.errors = (int*)(wb + j.w_errors);
        d.offsets = (uint32_t*)(wb + j.w_offsets);
        d.stream = (uint8_t*)(wb + j.w_stream);
        d.rgb = j.rgb;
        d.gray = j.gray;
        d.pitch_rgb = j.pitch_rgb;
        d.pitch_gray = j.pitch_gray;
        d.status = (int*)wb + i;
        d.nbits = 8ull * (unsigned long long)j.ps.payload.size();
        d.cap = (uint32_t)j.cap;
        d.need = (uint32_t)frame_bytes(pl);
        d.m = pl.min_code;
        d.x0 = pl.x0;
        d.y0 = pl.y0;
        d.w = pl.width;
        d.h = pl.height;
        d.cw = pl.canvas_w;
        d.ch = pl.canvas_h;
        d.interlace = pl.interlace;
        d.background = pl.transparency >= 0 ? pl.transparency : 0;
        d.mode_l = pl.mode_l;
        descs[i] = d;
    }
    if (descs_out) descs_out->assign(descs, descs + n);
    HIPCHK(hipMemcpyAsync(db, hb, in.off, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(wb, 0, status_bytes, st));
    const GdDesc* dd = (const GdDesc*)db;
    struct Events {                            // the timed path's: destroyed however the function is left
        hipEvent_t ev[6] = {};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } events;
    hipEvent_t* ev = events.ev;
    auto mark = [&](int i) {
        if (!launch_ms) return;
        HIPCHK(hipEventCreate(&ev[i]));
        HIPCHK(hipEventRecord(ev[i], st));
    };
    mark(0);
    HIPCHK(launch_gd_scan(dd, n, st));
    mark(1);
    if (launches >= 2) HIPCHK(launch_gd_lengths(dd, n, max_cap, st));
    mark(2);
    if (launches >= 3) HIPCHK(launch_gd_offsets(dd, n, st));
    mark(3);
    if (launches >= 4) HIPCHK(launch_gd_decode(dd, n, max_cap, st));
    mark(4);
    if (launches >= 5) HIPCHK(launch_gd_output(dd, n, max_pixels, st));                  // (only with destinations: bbocr_gif_decode)
    mark(5);
    dev_status.assign((size_t)n, 0);
    if (launches >= 3) {
        HIPCHK(hipMemcpyAsync(dev_status.data(), wb, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    } else {
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(&dev_status[i], descs[i].head + 1, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (launch_ms)
        for (int i = 0; i < 5; ++i) HIPCHK(hipEventElapsedTime(&launch_ms[i], ev[i], ev[i + 1]));
}

// a file the decoder takes: planned here, so that the caller's claim is never trusted
bool gif_admit(const uint8_t* file, size_t bytes, GifJob& j) {
    if (!file || bytes >= ((size_t)1 << 31)) return false;
    if (gif_parse(file, bytes, j.ps) != BBOCR_GIF_OK) return false;
    return j.ps.payload.size() < ((size_t)1 << 28);                   // (a piece's code count and a 32-bit bit position's low word)
}

}  // namespace

extern "C" {

int bbocr_host_gif_plan(const void* file, size_t bytes, bbocr_gif_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    GifParsed ps;
    gif_parse((const uint8_t*)file, bytes, ps);
    *plan = ps.plan;
    return BBOCR_OK;
}

size_t bbocr_gif_piece_room(long long payload_bytes, int min_code) {
    return payload_bytes < 0 || min_code < 2 || min_code > 8 ? 0 : gifl_piece_room((uint64_t)payload_bytes, min_code);
}

int bbocr_gif_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status) {
    return bbocr_gif_decode_timed(ctx, files, bytes, n, dst_rgb, pitch_rgb, dst_gray, pitch_gray, status, nullptr);
}

int bbocr_gif_decode_timed(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                           uint8_t* const* dst_gray, const long long* pitch_gray, int* status, float* launch_ms) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!files || !bytes || !dst_rgb || !pitch_rgb || !dst_gray || !pitch_gray || !status || n < 1) fail(BBOCR_ERR_ARG, "bad decode arguments");
        std::vector<GifJob> jobs;
        jobs.reserve((size_t)n);
        for (int k = 0; k < n; ++k) {
            status[k] = BBOCR_ERR_ARG;
            GifJob j;
            if (!gif_admit(files[k], bytes[k], j)) continue;
            const bbocr_gif_plan& pl = j.ps.plan;
            if (!dst_rgb[k] || !dst_gray[k] || pitch_rgb[k] < 3LL * pl.canvas_w || pitch_gray[k] < (long long)pl.canvas_w) continue;
            j.k = k;
            j.rgb = dst_rgb[k];
            j.gray = dst_gray[k];
            j.pitch_rgb = pitch_rgb[k];
            j.pitch_gray = pitch_gray[k];
            jobs.push_back(std::move(j));
        }
        if (jobs.empty()) return;
        std::vector<int> ds;
        gif_run(ctx, st, jobs, 5, ds, nullptr, launch_ms);
        for (size_t i = 0; i < jobs.size(); ++i) status[jobs[i].k] = ds[i] ? BBOCR_ERR_DATA : BBOCR_OK;
    });
}

int bbocr_op_gif_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!file || !dev_dst || stage < 0 || stage > 2) fail(BBOCR_ERR_ARG, "bad stage arguments");
        std::vector<GifJob> jobs(1);
        if (!gif_admit(file, bytes, jobs[0])) fail(BBOCR_ERR_ARG, "the plan refuses this file");
        const bbocr_gif_plan& pl = jobs[0].ps.plan;
        const size_t cap = gifl_piece_room((uint64_t)pl.payload_bytes, pl.min_code);
        const size_t need = stage == 0 ? 16 + sizeof(GiflPiece) * cap : (stage == 1 ? 4 * (cap + 1) : frame_bytes(pl));
        if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
        std::vector<int> ds;
        std::vector<GdDesc> descs;
        gif_run(ctx, st, jobs, stage == 0 ? 1 : (stage == 1 ? 3 : 4), ds, &descs);
        if (file_status) *file_status = ds[0] ? BBOCR_ERR_DATA : BBOCR_OK;
        const void* from = stage == 0 ? (const void*)descs[0].head : (stage == 1 ? (const void*)descs[0].offsets : (const void*)descs[0].stream);
        HIPCHK(hipMemcpyAsync(dev_dst, from, need, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    });
}

}  // extern "C"
