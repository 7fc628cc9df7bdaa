// TIFF decoding, host side: the plan (tiff_parse.h's IFD walk), a batch's admission, its one staged blob -- file and strip descriptors,
// the strips' stored bytes, palettes -- and the launch sequence of tiffdec.hip.  A batch runs on the decode lane's stream of the root
// context, outside the call slots, with the lane's buffers (the contract of bbocr_jpeg_decode): files decode while two OCR calls run.
#include "ctx.h"
#include "tiff_parse.h"
#include "tiffdec.h"

namespace {

using namespace tiff_host;

struct TiffJob {                               // one admitted file of a batch
    TiffParsed ps;
    bbocr_tiff_fax fax{};                      // scheme 0: a file of the plain plan
    const uint8_t* file = nullptr;
    int k = 0;                                 // its index in the caller's arrays
    uint8_t *rgb = nullptr, *gray = nullptr;   // null: into the batch's own planes (the stage entry point)
    long long pitch_rgb = 0, pitch_gray = 0;
    size_t o_pal = 0, w_stream = 0, w_rgb = 0, w_gray = 0;
    std::vector<size_t> o_strip;
};

size_t stream_bytes(const bbocr_tiff_plan& pl) { return (size_t)pl.height * (size_t)pl.row_bytes; }

// An uncompressed strip has no stream to enter: it is cut into pieces of kRawPiece bytes, each a "strip" of its own for td_strips, so that
// a file written as ONE strip (Pillow's raw writer) is copied by many wavefronts.  A stored strip that is short of its rows leaves its last
// pieces short of input: their status is the strip's.
constexpr size_t kRawPiece = 65536;

size_t strip_need(const bbocr_tiff_plan& pl, size_t s) { return (size_t)tiff_strip_rows(pl, (int)s) * (size_t)pl.row_bytes; }

size_t strip_pieces(const bbocr_tiff_plan& pl, size_t s) { return pl.compression == 1 ? std::max<size_t>(1, (strip_need(pl, s) + kRawPiece - 1) / kRawPiece) : 1; }

size_t job_pieces(const TiffJob& j) {
    size_t n = 0;
    for (size_t s = 0; s < j.ps.strips.size(); ++s) n += strip_pieces(j.ps.plan, s);
    return n;
}

int codec_of(int compression) {
    if (compression >= 2 && compression <= 4) return TD_FAX;       // (only a file admitted under the fax plan)
    return compression == 1 ? TD_RAW : (compression == 32773 ? TD_PACKBITS : (compression == 5 ? TD_LZW : TD_DEFLATE));
}

// The decode of the admitted jobs up to `stages` launches (1: strips, 2: + predictor, 3: + output) on the lane's stream.  Fills
// dev_status[i] (the error bits of job i: its strips' ORed) and, for the stage entry point, the descriptors.  Everything queued is
// finished on return.
void tiff_run(bbocr_ctx* root, hipStream_t st, std::vector<TiffJob>& jobs, int stages, std::vector<int>& dev_status, std::vector<TdDesc>* descs_out = nullptr) {
    const int n = (int)jobs.size();
    size_t total_strips = 0;
    for (const TiffJob& j : jobs) total_strips += job_pieces(j);
    const size_t status_bytes = align_up(4 * ((size_t)n + total_strips), 256);
    const size_t desc_bytes = align_up(sizeof(TdDesc) * (size_t)n, 256);
    Carve in{desc_bytes + align_up(sizeof(TdStrip) * total_strips, 256)}, work{status_bytes};
    unsigned long long max_pixels = 1;
    int max_pred_rows = 0;
    bool any_lzw = false, any_deflate = false;
    int fax_width = 0;                         // the widest CCITT file: it sizes the strip launch's line buffers
    for (TiffJob& j : jobs) {
        const bbocr_tiff_plan& pl = j.ps.plan;
        j.o_strip.clear();
        for (const auto& s : j.ps.strips) j.o_strip.push_back(in.add(s.second + 8));
        j.o_pal = in.add(768);
        j.w_stream = work.add(stream_bytes(pl));
        if (!j.rgb) {
            j.w_rgb = work.add((size_t)pl.height * pl.width * 3);
            j.w_gray = work.add((size_t)pl.height * pl.width);
        }
        max_pixels = std::max(max_pixels, (unsigned long long)pl.height * (unsigned long long)pl.width);
        if (pl.predictor == 2) max_pred_rows = std::max(max_pred_rows, pl.height);
        any_lzw |= pl.compression == 5;
        any_deflate |= pl.compression == 8 || pl.compression == 32946;
        if (j.fax.scheme) fax_width = std::max(fax_width, pl.width);
    }
    root->jd_pin.ensure(in.off);
    root->jd_in.ensure(in.off);
    root->jd_work.ensure(work.off);
    char* hb = (char*)root->jd_pin.p;
    char* db = (char*)root->jd_in.p;
    char* wb = (char*)root->jd_work.p;
    TdDesc* descs = (TdDesc*)hb;
    TdStrip* strips = (TdStrip*)(hb + desc_bytes);
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        TiffJob& j = jobs[i];
        const bbocr_tiff_plan& pl = j.ps.plan;
        std::memcpy(hb + j.o_pal, j.ps.palette, 768);
        TdDesc d{};
        d.stream = (uint8_t*)(wb + j.w_stream);
        d.palette = (const uint8_t*)(db + j.o_pal);
        d.rgb = j.rgb ? j.rgb : (uint8_t*)(wb + j.w_rgb);
        d.gray = j.gray ? j.gray : (uint8_t*)(wb + j.w_gray);
        d.pitch_rgb = j.rgb ? j.pitch_rgb : 3LL * pl.width;
        d.pitch_gray = j.gray ? j.pitch_gray : (long long)pl.width;
        d.status = (int*)wb + i;
        d.W = pl.width;
        d.H = pl.height;
        d.bits = pl.bits;
        d.samples = pl.samples;
        d.photometric = pl.photometric;
        d.predictor = pl.predictor;
        d.row_bytes = (int)pl.row_bytes;
        descs[i] = d;
        for (size_t s = 0; s < j.ps.strips.size(); ++s) {
            const size_t stored = j.ps.strips[s].second, need = strip_need(pl, s), pieces = strip_pieces(pl, s);
            std::memcpy(hb + j.o_strip[s], j.file + j.ps.strips[s].first, stored);
            for (size_t p = 0; p < pieces; ++p, ++at) {
                const size_t from = pieces > 1 ? p * kRawPiece : 0;           // (only a raw strip has more than one piece)
                TdStrip t{};
                t.src = (const uint8_t*)(db + j.o_strip[s]) + from;
                t.dst = d.stream + s * (size_t)pl.rows_per_strip * (size_t)pl.row_bytes + from;
                t.file_status = d.status;
                t.status = (int*)wb + n + at;
                t.src_bytes = (unsigned)(pieces > 1 ? (stored > from ? std::min(stored - from, kRawPiece) : 0) : stored);
                t.need = (unsigned)(pieces > 1 ? std::min(need - from, kRawPiece) : need);
                t.codec = codec_of(pl.compression);
                t.fax_width = pl.width;
                t.fax_mode = j.fax.scheme | (j.fax.t4_options & 255) << 8 | j.fax.fill_order << 16;
                strips[at] = t;
            }
        }
    }
    if (descs_out) descs_out->assign(descs, descs + n);
    HIPCHK(hipMemcpyAsync(db, hb, in.off, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(wb, 0, status_bytes, st));
    const TdDesc* dd = (const TdDesc*)db;
    HIPCHK(launch_td_strips((const TdStrip*)(db + desc_bytes), (int)total_strips, td_strips_lds(any_lzw, any_deflate, fax_width), st));
    if (stages >= 2 && max_pred_rows > 0) HIPCHK(launch_td_predictor(dd, n, max_pred_rows, st));
    if (stages >= 3) HIPCHK(launch_td_output(dd, n, max_pixels, st));
    dev_status.assign((size_t)n, 0);
    HIPCHK(hipMemcpyAsync(dev_status.data(), wb, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// a file the decoder takes: planned here, so that the caller's claim is never trusted.  fax: under the fax plan (CCITT files as well)
bool tiff_admit(const uint8_t* file, size_t bytes, TiffJob& j, bool fax = false) {
    if (!file || bytes >= ((size_t)1 << 31)) return false;
    if (fax ? !tiff_fax_parse(file, bytes, j.ps, j.fax) : tiff_parse(file, bytes, j.ps) != BBOCR_TIFF_OK) return false;
    j.file = file;
    return true;
}

int decode_batch(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                 uint8_t* const* dst_gray, const long long* pitch_gray, int* status, bool fax) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!files || !bytes || !dst_rgb || !pitch_rgb || !dst_gray || !pitch_gray || !status || n < 1) fail(BBOCR_ERR_ARG, "bad decode arguments");
        std::vector<TiffJob> jobs;
        jobs.reserve((size_t)n);
        size_t total_strips = 0;
        for (int k = 0; k < n; ++k) {
            status[k] = BBOCR_ERR_ARG;
            TiffJob j;
            if (!tiff_admit(files[k], bytes[k], j, fax)) continue;
            const bbocr_tiff_plan& pl = j.ps.plan;
            if (!dst_rgb[k] || !dst_gray[k] || pitch_rgb[k] < 3LL * pl.width || pitch_gray[k] < (long long)pl.width) continue;
            if (total_strips + job_pieces(j) > 0x7FFFFFFFu) continue;             // (one strip per workgroup of a one-dimensional grid)
            total_strips += job_pieces(j);
            j.k = k;
            j.rgb = dst_rgb[k];
            j.gray = dst_gray[k];
            j.pitch_rgb = pitch_rgb[k];
            j.pitch_gray = pitch_gray[k];
            jobs.push_back(std::move(j));
        }
        if (jobs.empty()) return;
        std::vector<int> ds;
        tiff_run(ctx, st, jobs, 3, ds);
        for (size_t i = 0; i < jobs.size(); ++i) status[jobs[i].k] = ds[i] ? BBOCR_ERR_DATA : BBOCR_OK;
    });
}

int decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status, bool fax) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        if (!file || !dev_dst || stage < 0 || stage > 2) fail(BBOCR_ERR_ARG, "bad stage arguments");
        std::vector<TiffJob> jobs(1);
        if (!tiff_admit(file, bytes, jobs[0], fax)) fail(BBOCR_ERR_ARG, "the plan refuses this file");
        const bbocr_tiff_plan& pl = jobs[0].ps.plan;
        const size_t px = (size_t)pl.height * (size_t)pl.width;
        const size_t need = stage < 2 ? stream_bytes(pl) : 4 * px;
        if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
        std::vector<int> ds;
        std::vector<TdDesc> descs;
        tiff_run(ctx, st, jobs, stage + 1, ds, &descs);
        if (file_status) *file_status = ds[0] ? BBOCR_ERR_DATA : BBOCR_OK;
        if (stage < 2) {
            HIPCHK(hipMemcpyAsync(dev_dst, descs[0].stream, need, hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(hipMemcpyAsync(dev_dst, descs[0].rgb, 3 * px, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync((char*)dev_dst + 3 * px, descs[0].gray, px, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipStreamSynchronize(st));
    });
}

}  // namespace

extern "C" {

int bbocr_host_tiff_plan(const void* file, size_t bytes, bbocr_tiff_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    TiffParsed ps;
    tiff_parse((const uint8_t*)file, bytes, ps);
    *plan = ps.plan;
    return BBOCR_OK;
}

int bbocr_host_tiff_fax_plan(const void* file, size_t bytes, bbocr_tiff_plan* plan, bbocr_tiff_fax* fax) {
    if (!file || !plan || !fax) return BBOCR_ERR_ARG;
    TiffParsed ps;
    tiff_fax_parse((const uint8_t*)file, bytes, ps, *fax);
    *plan = ps.plan;
    return BBOCR_OK;
}

int bbocr_tiff_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                      uint8_t* const* dst_gray, const long long* pitch_gray, int* status) {
    return decode_batch(ctx, files, bytes, n, dst_rgb, pitch_rgb, dst_gray, pitch_gray, status, false);
}

int bbocr_tiff_decode_fax(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dst_rgb, const long long* pitch_rgb,
                          uint8_t* const* dst_gray, const long long* pitch_gray, int* status) {
    return decode_batch(ctx, files, bytes, n, dst_rgb, pitch_rgb, dst_gray, pitch_gray, status, true);
}

int bbocr_op_tiff_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status) {
    return decode_stage(ctx, file, bytes, stage, dev_dst, dst_bytes, file_status, false);
}

int bbocr_op_tiff_fax_decode_stage(bbocr_ctx* ctx, const uint8_t* file, size_t bytes, int stage, void* dev_dst, size_t dst_bytes, int* file_status) {
    return decode_stage(ctx, file, bytes, stage, dev_dst, dst_bytes, file_status, true);
}

}  // extern "C"
