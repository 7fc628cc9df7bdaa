// The model-input JPEG encoder (enhanced_extractor.py:399-411), host side: the header Pillow writes in front of the scan, the capacity
// bound, and the launch sequence of jpegenc.hip.  Two lengths are only known on the device -- the scan's bits and its 0xFF bytes -- and
// each is read back once, so that the buffers behind them are sized by what the page produced, not by the bound.
#include "ctx.h"

namespace {

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                             13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                             38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kMaxComment = 65533;                              // a marker segment's length field counts itself
// SOI, APP0, the longest COM, two DQT, SOF0 of three components, the four DHT, SOS of three components
constexpr size_t kHeaderMax = 2 + 18 + (4 + kMaxComment) + 2 * 69 + 19 + 2 * (33 + 183) + 14;

void put_segment(std::vector<uint8_t>& o, int marker, const std::vector<uint8_t>& body) {
    o.push_back(0xFF);
    o.push_back((uint8_t)marker);
    o.push_back((uint8_t)((body.size() + 2) >> 8));
    o.push_back((uint8_t)((body.size() + 2) & 0xFF));
    o.insert(o.end(), body.begin(), body.end());
}

// what Pillow 12 (jcmarker.c behind JpegEncode.c) writes up to and including SOS for save(format="JPEG", quality=q) of an RGB or "L" image
std::vector<uint8_t> je_header(int H, int W, int components, int quality, const uint8_t* comment, int comment_bytes) {
    ThQuant q;
    bbocr_host_jpeg_qtables(quality, &q.q[0][0]);
    std::vector<uint8_t> o = {0xFF, 0xD8};
    put_segment(o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    if (comment_bytes > 0) put_segment(o, 0xFE, std::vector<uint8_t>(comment, comment + comment_bytes));
    for (int t = 0; t < (components == 1 ? 1 : 2); ++t) {
        std::vector<uint8_t> b = {(uint8_t)t};
        for (int k = 0; k < 64; ++k) b.push_back((uint8_t)q.q[t][kZigzag[k]]);
        put_segment(o, 0xDB, b);
    }
    std::vector<uint8_t> sof = {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, (uint8_t)components};
    for (int c = 0; c < components; ++c) sof.insert(sof.end(), {(uint8_t)(c + 1), (uint8_t)(c == 0 && components == 3 ? 0x22 : 0x11), (uint8_t)(c ? 1 : 0)});
    put_segment(o, 0xC0, sof);
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};            // JE_STD's order: DC 0, AC 0, DC 1, AC 1
    for (int t = 0; t < (components == 1 ? 2 : 4); ++t) {
        std::vector<uint8_t> b = {ids[t]};
        b.insert(b.end(), JE_STD[t].bits, JE_STD[t].bits + 16);
        b.insert(b.end(), JE_STD[t].vals, JE_STD[t].vals + JE_STD[t].n);
        put_segment(o, 0xC4, b);
    }
    std::vector<uint8_t> sos = {(uint8_t)components};
    for (int c = 0; c < components; ++c) sos.insert(sos.end(), {(uint8_t)(c + 1), (uint8_t)(c ? 0x11 : 0x00)});
    sos.insert(sos.end(), {0, 63, 0});
    put_segment(o, 0xDA, sos);
    return o;
}

bool je_shape_ok(int H, int W, int components) { return H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && (components == 1 || components == 3); }

size_t je_scan_bound(int H, int W, int components) {           // bytes of the unstuffed scan, at most
    return ((size_t)je_blocks(H, W, components) * JE_BLOCK_MAX_BITS + 7) / 8;
}

void je_check(const void* src, int H, int W, long long pitch, int layout, int components, int quality) {
    check_page({src, H, W, pitch, layout});
    if (!je_shape_ok(H, W, components)) fail(BBOCR_ERR_ARG, "H and W must be 1 .. 65535, components 1 or 3");
    if (components == 1 && layout != PAGE_GRAY) fail(BBOCR_ERR_ARG, "one component needs a gray page");
    if (quality < 1 || quality > 100) fail(BBOCR_ERR_ARG, "quality must be 1 .. 100");
}

struct JeRun {
    int n, tiles;                     // blocks, tiles of JE_TILE blocks
    short* coef;
    unsigned int* local;
    unsigned long long* tile_off;     // [tiles + 1]
    long long* offsets;               // stage 1 only: [n + 1]
    long long bits = 0, bytes = 0;    // the unstuffed scan
};

// Enqueues the coefficient and size passes and waits for the scan's bit count; buffers from the slot's arena
JeRun je_sizes(bbocr_ctx* c, const uint8_t* src, int H, int W, size_t pitch, int layout, int components, int quality, bool want_offsets) {
    JeRun r{};
    r.n = je_blocks(H, W, components);
    r.tiles = cdiv(r.n, JE_TILE);
    Carve cv;
    const size_t o_coef = cv.add((size_t)r.n * 128), o_local = cv.add((size_t)r.n * 4), o_tile = cv.add((size_t)(r.tiles + 1) * 8);
    const size_t o_off = cv.add(want_offsets ? (size_t)(r.n + 1) * 8 : 0);
    c->arena.buf.ensure(cv.off);
    r.coef = Carve::at<short>(c->arena.buf.p, o_coef);
    r.local = Carve::at<unsigned int>(c->arena.buf.p, o_local);
    r.tile_off = Carve::at<unsigned long long>(c->arena.buf.p, o_tile);
    r.offsets = Carve::at<long long>(c->arena.buf.p, o_off);
    ThQuant q;
    bbocr_host_jpeg_qtables(quality, &q.q[0][0]);
    HIPCHK(launch_je_coef(src, pitch, layout, components, H, W, q, r.coef, c->stream));
    HIPCHK(launch_je_sizes(r.coef, r.n, components, r.local, r.tile_off, c->stream));
    HIPCHK(launch_je_scan(r.tile_off, r.tiles, c->stream));
    if (want_offsets) HIPCHK(launch_je_offsets(r.local, r.tile_off, r.n, r.offsets, c->stream));
    unsigned long long bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, r.tile_off + r.tiles, 8, hipMemcpyDeviceToHost, c->stream));
    slot_sync(c, c->stream);
    r.bits = (long long)bits;
    r.bytes = (r.bits + 7) / 8;
    return r;
}

// Enqueues the packing pass: the unstuffed scan in c->je_scan (zero up to the end of its last stuffing tile), the stuffing counters behind it
unsigned long long* je_pack(bbocr_ctx* c, const JeRun& r, int components) {
    const size_t padded = align_up((size_t)r.bytes, JE_STUFF_TILE), stiles = padded / JE_STUFF_TILE;
    c->je_scan.ensure(padded + (stiles + 1) * 8);
    HIPCHK(hipMemsetAsync(c->je_scan.p, 0, padded, c->stream));
    HIPCHK(launch_je_pack(r.coef, r.n, components, r.local, r.tile_off, (uint32_t*)c->je_scan.p, c->stream));
    return (unsigned long long*)((char*)c->je_scan.p + padded);
}

}  // namespace

extern "C" {

size_t bbocr_jpeg_encode_bound(int H, int W, int components) {
    if (!je_shape_ok(H, W, components)) return 0;
    return kHeaderMax + 2 * je_scan_bound(H, W, components) + 2;
}

int bbocr_host_jpeg_header(int H, int W, int components, int quality, const uint8_t* comment, int comment_bytes, uint8_t* out, size_t capacity,
                           size_t* bytes) {
    if (!je_shape_ok(H, W, components) || quality < 1 || quality > 100 || comment_bytes < 0 || comment_bytes > kMaxComment ||
        (comment_bytes > 0 && !comment) || !out || !bytes)
        return BBOCR_ERR_ARG;
    const std::vector<uint8_t> h = je_header(H, W, components, quality, comment, comment_bytes);
    *bytes = h.size();
    if (capacity < h.size()) return BBOCR_ERR_ARG;
    std::memcpy(out, h.data(), h.size());
    return BBOCR_OK;
}

int bbocr_jpeg_encode(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int components, int quality,
                      const uint8_t* comment, int comment_bytes, uint8_t* host_out, size_t capacity, size_t* bytes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        je_check(dev_src, H, W, pitch, layout, components, quality);
        if (!host_out || !bytes) fail(BBOCR_ERR_ARG, "null pointer");
        if (comment_bytes < 0 || comment_bytes > kMaxComment || (comment_bytes > 0 && !comment)) fail(BBOCR_ERR_ARG, "bad comment");
        if (capacity < bbocr_jpeg_encode_bound(H, W, components)) fail(BBOCR_ERR_ARG, "capacity below bbocr_jpeg_encode_bound");
        const std::vector<uint8_t> head = je_header(H, W, components, quality, comment, comment_bytes);
        const JeRun r = je_sizes(ctx, dev_src, H, W, (size_t)pitch, layout, components, quality, false);
        unsigned long long* tile_ff = je_pack(ctx, r, components);
        const uint8_t* scan = (const uint8_t*)ctx->je_scan.p;
        const int stiles = (int)((r.bytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE);
        HIPCHK(launch_je_ff_count(scan, r.bytes, tile_ff, ctx->stream));
        HIPCHK(launch_je_scan(tile_ff, stiles, ctx->stream));
        unsigned long long ff = 0;
        HIPCHK(hipMemcpyAsync(&ff, tile_ff + stiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        const size_t stuffed = (size_t)r.bytes + (size_t)ff;
        if (head.size() + stuffed + 2 > capacity) fail(BBOCR_ERR_INTERNAL, "the scan exceeds its bound");
        ctx->je_out.ensure(stuffed);
        HIPCHK(launch_je_stuff(scan, r.bytes, tile_ff, (uint8_t*)ctx->je_out.p, ctx->stream));
        std::memcpy(host_out, head.data(), head.size());
        HIPCHK(hipMemcpyAsync(host_out + head.size(), ctx->je_out.p, stuffed, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        host_out[head.size() + stuffed] = 0xFF;
        host_out[head.size() + stuffed + 1] = 0xD9;
        *bytes = head.size() + stuffed + 2;
    });
}

int bbocr_op_jpeg_encode_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int components,
                               int quality, void* dev_dst, size_t dst_bytes, size_t* bytes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        je_check(dev_src, H, W, pitch, layout, components, quality);
        if (!dev_dst || !bytes || stage < 0 || stage > 2) fail(BBOCR_ERR_ARG, "bad arguments");
        const size_t n = (size_t)je_blocks(H, W, components);
        const size_t need = stage == 0 ? n * 128 : (stage == 1 ? (n + 1) * 8 : je_scan_bound(H, W, components));
        if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
        const JeRun r = je_sizes(ctx, dev_src, H, W, (size_t)pitch, layout, components, quality, stage == 1);
        const void* from = stage == 0 ? (const void*)r.coef : (const void*)r.offsets;
        *bytes = need;
        if (stage == 2) {
            je_pack(ctx, r, components);
            from = ctx->je_scan.p;
            *bytes = (size_t)r.bytes;
        }
        HIPCHK(hipMemcpyAsync(dev_dst, from, *bytes, hipMemcpyDeviceToDevice, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

}  // extern "C"
