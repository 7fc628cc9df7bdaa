// PNG decoding, host side: the plan (png_parse.h's chunk walk), a batch's admission, its one staged blob -- descriptors, the files' IDAT
// payloads back to back, palettes -- and the launch sequence of pngdec.hip.  A batch runs on the decode lane's stream of the root
// context, outside the call slots, with the lane's buffers (the contract of bbocr_jpeg_decode): files decode while two OCR calls run.
#include "ctx.h"
#include "png_parse.h"
#include "pngdec.h"

namespace {

using namespace png_host;

struct PngJob {                                // one admitted file of a batch
    PngParsed ps;
    const uint8_t* file = nullptr;
    int k = 0;                                 // its index in the caller's arrays
    uint8_t *rgb = nullptr, *gray = nullptr;   // null: into the batch's own planes (the stage entry point)
    long long pitch_rgb = 0, pitch_gray = 0;
    size_t o_z = 0, o_pal = 0, w_raw = 0, w_rgb = 0, w_gray = 0;
};

size_t raw_bytes(const bbocr_png_plan& pl) { return (size_t)pl.height * (size_t)(pl.row_bytes + 1); }

// The decode of the admitted jobs up to `stages` launches (1: inflate, 2: + unfilter, 3: + output) on the lane's stream.  Fills
// dev_status[i] (the PNGI_ERR_* / PD_ERR_* bits of job i) and, for the stage entry point, the descriptors.  Everything queued is finished
// on return.
void png_run(bbocr_ctx* root, hipStream_t st, std::vector<PngJob>& jobs, int stages, std::vector<int>& dev_status, std::vector<PdDesc>* descs_out = nullptr) {
    const int n = (int)jobs.size();
    Carve in{align_up(sizeof(PdDesc) * (size_t)n, 256)}, work{align_up(4 * (size_t)n, 256)};
    unsigned long long max_pixels = 1;
    for (PngJob& j : jobs) {
        const bbocr_png_plan& pl = j.ps.plan;
        j.o_z = in.add((size_t)pl.idat_bytes + 8);
        j.o_pal = in.add(768);
        j.w_raw = work.add(raw_bytes(pl));
        if (!j.rgb) {
            j.w_rgb = work.add((size_t)pl.height * pl.width * 3);
            j.w_gray = work.add((size_t)pl.height * pl.width);
        }
        max_pixels = std::max(max_pixels, (unsigned long long)pl.height * (unsigned long long)pl.width);
    }
    root->jd_pin.ensure(in.off);
    root->jd_in.ensure(in.off);
    root->jd_work.ensure(work.off);
    char* hb = (char*)root->jd_pin.p;
    char* db = (char*)root->jd_in.p;
    char* wb = (char*)root->jd_work.p;
    PdDesc* descs = (PdDesc*)hb;
    for (int i = 0; i < n; ++i) {
        PngJob& j = jobs[i];
        const bbocr_png_plan& pl = j.ps.plan;
        png_gather(j.file, j.ps, (uint8_t*)(hb + j.o_z));
        std::memcpy(hb + j.o_pal, j.ps.palette, 768);
        PdDesc d{};
        d.z = (const uint8_t*)(db + j.o_z);
        d.raw = (uint8_t*)(wb + j.w_raw);
        d.palette = (const uint8_t*)(db + j.o_pal);
        d.rgb = j.rgb ? j.rgb : (uint8_t*)(wb + j.w_rgb);
        d.gray = j.gray ? j.gray : (uint8_t*)(wb + j.w_gray);
        d.pitch_rgb = j.rgb ? j.pitch_rgb : 3LL * pl.width;
        d.pitch_gray = j.gray ? j.pitch_gray : (long long)pl.width;
        d.status = (int*)wb + i;
        d.z_bytes = (unsigned)pl.idat_bytes;
        d.raw_bytes = (unsigned)raw_bytes(pl);
        d.W = pl.width;
        d.H = pl.height;
        d.depth = pl.bit_depth;
        d.color_type = pl.color_type;
        d.channels = pl.channels;
        d.bpp = pl.bpp;
        d.row_bytes = (int)pl.row_bytes;
        d.palette_entries = pl.palette_entries;
        descs[i] = d;
    }
    if (descs_out) descs_out->assign(descs, descs + n);
    HIPCHK(hipMemcpyAsync(db, hb, in.off, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(wb, 0, align_up(4 * (size_t)n, 256), st));
    const PdDesc* dd = (const PdDesc*)db;
    HIPCHK(launch_pd_inflate(dd, n, st));
    if (stages >= 2) HIPCHK(launch_pd_unfilter(dd, n, st));
    if (stages >= 3) HIPCHK(launch_pd_output(dd, n, max_pixels, st));
    dev_status.assign((size_t)n, 0);
    HIPCHK(hipMemcpyAsync(dev_status.data(), wb, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// a file the decoder takes: planned here, so that the caller's claim is never trusted
bool png_admit(const uint8_t* file, size_t bytes, PngJob& j) {
    if (!file || bytes >= ((size_t)1 << 31)) return false;
    if (png_parse(file, bytes, j.ps) != BBOCR_PNG_OK) return false;
    if (j.ps.plan.idat_bytes > 0x7FFFFFF0LL) return false;
    j.file = file;
    return true;
}

}  // namespace

extern "C" {

int bbocr_host_png_plan(const void* file, size_t bytes, bbocr_png_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    PngParsed ps;
    png_parse((const uint8_t*)file, bytes, ps);
    *plan = ps.plan;
    return BBOCR_OK;
}

int bbocr_png_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!files || !bytes || !dst_rgb || !pitch_rgb || !dst_gray || !pitch_gray || !status || n < 1) fail(BBOCR_ERR_ARG, "bad decode arguments");
        std::vector<PngJob> jobs;
        jobs.reserve((size_t)n);
        for (int k = 0; k < n; ++k) {
            status[k] = BBOCR_ERR_ARG;
            PngJob j;
            if (!png_admit(files[k], bytes[k], j)) continue;
            const bbocr_png_plan& pl = j.ps.plan;
            if (!dst_rgb[k] || !dst_gray[k] || pitch_rgb[k] < 3LL * pl.width || pitch_gray[k] < (long long)pl.width) continue;
            j.k = k;
            j.rgb = dst_rgb[k];
            j.gray = dst_gray[k];
            j.pitch_rgb = pitch_rgb[k];
            j.pitch_gray = pitch_gray[k];
            jobs.push_back(std::move(j));
        }
        if (jobs.empty()) return;
        std::vector<int> ds;
        png_run(ctx, st, jobs, 3, ds);
        for (size_t i = 0; i < jobs.size(); ++i) status[jobs[i].k] = ds[i] ? BBOCR_ERR_DATA : BBOCR_OK;
    });
}

int bbocr_op_png_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!file || !dev_dst || stage < 0 || stage > 2) fail(BBOCR_ERR_ARG, "bad stage arguments");
        std::vector<PngJob> jobs(1);
        if (!png_admit(file, bytes, jobs[0])) fail(BBOCR_ERR_ARG, "the plan refuses this file");
        const bbocr_png_plan& pl = jobs[0].ps.plan;
        const size_t px = (size_t)pl.height * (size_t)pl.width;
        const size_t need = stage < 2 ? raw_bytes(pl) : 4 * px;
        if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
        std::vector<int> ds;
        std::vector<PdDesc> descs;
        png_run(ctx, st, jobs, stage + 1, ds, &descs);
        if (file_status) *file_status = ds[0] ? BBOCR_ERR_DATA : BBOCR_OK;
        if (stage < 2) {
            HIPCHK(hipMemcpyAsync(dev_dst, descs[0].raw, need, hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(hipMemcpyAsync(dev_dst, descs[0].rgb, 3 * px, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync((char*)dev_dst + 3 * px, descs[0].gray, px, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipStreamSynchronize(st));
    });
}

}  // extern "C"
