// BMP decoding, host side: the plan (bmp_parse.h), a batch's admission, its one staged blob -- the file descriptors and the files from
// their tables to the end of their rows -- and the one launch of bmpdec.hip.  A batch runs on the decode lane's stream of the root context,
// outside the call slots, with the lane's buffers (the contract of bbocr_jpeg_decode).
#include "ctx.h"
#include "bmp_parse.h"
#include "bmpdec.h"

namespace {

struct BmpJob {                                // one admitted file of a batch
    bbocr_bmp_plan plan{};
    const uint8_t* file = nullptr;
    size_t bytes = 0, o_file = 0;
    int k = 0;                                 // its index in the caller's arrays
    uint8_t *rgb = nullptr, *gray = nullptr;
    long long pitch_rgb = 0, pitch_gray = 0;
};

}  // namespace

extern "C" {

int bbocr_host_bmp_plan(const void* file, size_t bytes, bbocr_bmp_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    bmp_host::bmp_parse((const uint8_t*)file, bytes, *plan);
    return BBOCR_OK;
}

int bbocr_bmp_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                     uint8_t* const* dst_gray, const long long* pitch_gray, int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!files || !bytes || !dst_rgb || !pitch_rgb || !dst_gray || !pitch_gray || !status || n < 1) fail(BBOCR_ERR_ARG, "bad decode arguments");
        std::vector<BmpJob> jobs;
        jobs.reserve((size_t)n);
        const size_t desc_bytes = align_up(sizeof(BdDesc) * (size_t)n, 256);
        Carve in{desc_bytes};
        int max_rows = 1;
        for (int k = 0; k < n; ++k) {
            status[k] = BBOCR_ERR_ARG;
            BmpJob j;
            // planned here, so that the caller's claim is never trusted
            if (!files[k] || bytes[k] >= ((size_t)1 << 31) || bmp_host::bmp_parse(files[k], bytes[k], j.plan) != BBOCR_BMP_OK) continue;
            const bbocr_bmp_plan& pl = j.plan;
            if (!dst_rgb[k] || !dst_gray[k] || pitch_rgb[k] < 3LL * pl.width || pitch_gray[k] < (long long)pl.width) continue;
            j.file = files[k];
            // what is read ends behind the rows -- or behind the table, in a file that keeps its rows in front of it
            j.bytes = std::max((size_t)pl.data_offset + (size_t)pl.row_stride * (size_t)pl.height, (size_t)pl.table_offset + (size_t)pl.table_entry * (size_t)pl.colors);
            j.o_file = in.add(j.bytes);
            j.k = k;
            j.rgb = dst_rgb[k];
            j.gray = dst_gray[k];
            j.pitch_rgb = pitch_rgb[k];
            j.pitch_gray = pitch_gray[k];
            max_rows = std::max(max_rows, pl.height);
            jobs.push_back(j);
        }
        if (jobs.empty()) return;
        ctx->jd_pin.ensure(in.off);
        ctx->jd_in.ensure(in.off);
        char* hb = (char*)ctx->jd_pin.p;
        char* db = (char*)ctx->jd_in.p;
        BdDesc* descs = (BdDesc*)hb;
        for (size_t i = 0; i < jobs.size(); ++i) {
            const BmpJob& j = jobs[i];
            const bbocr_bmp_plan& pl = j.plan;
            std::memcpy(hb + j.o_file, j.file, j.bytes);
            BdDesc d{};
            d.rows = (const uint8_t*)(db + j.o_file) + pl.data_offset;
            d.table = (const uint8_t*)(db + j.o_file) + pl.table_offset;
            d.rgb = j.rgb;
            d.gray = j.gray;
            d.pitch_rgb = j.pitch_rgb;
            d.pitch_gray = j.pitch_gray;
            d.stride = pl.row_stride;
            d.W = pl.width;
            d.H = pl.height;
            d.bits = pl.bits;
            d.mode = pl.mode;
            d.colors = pl.colors;
            d.entry = pl.table_entry;
            d.top_down = pl.top_down;
            d.r_at = pl.r_at;
            d.g_at = pl.g_at;
            d.b_at = pl.b_at;
            d.six_bit_green = pl.six_bit_green;
            descs[i] = d;
        }
        HIPCHK(hipMemcpyAsync(db, hb, in.off, hipMemcpyHostToDevice, st));
        HIPCHK(launch_bd_output((const BdDesc*)db, (int)jobs.size(), max_rows, st));
        HIPCHK(hipStreamSynchronize(st));
        for (const BmpJob& j : jobs) status[j.k] = BBOCR_OK;
    });
}

}  // extern "C"
