// The device PNG writer, host side: the capacity bound, the launch sequence of pngenc.hip and the framing -- signature, IHDR, iCCP, one
// IDAT (zlib header, the compacted deflate blocks, the final empty block, Adler-32), IEND, each chunk's CRC-32.  The library links no
// zlib: the profile of an iCCP chunk is deflated as stored blocks, and both checksums are the few lines below.
#include "ctx.h"

namespace {

constexpr size_t kPngMax = 0x7FFFFFFF;                          // a PNG chunk's length field (and H, W)
constexpr size_t kFrame = 8 + 25 + 12 + 2 + 12;                 // signature, IHDR, IDAT's length/type/CRC, its zlib header, IEND
constexpr uint32_t kAdlerMod = 65521;

uint32_t crc32_of(const uint8_t* p, size_t n) {
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint32_t adler32_of(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) {
        a = (a + p[i]) % kAdlerMod;
        b = (b + a) % kAdlerMod;
    }
    return (b << 16) | a;
}

void put_be32(uint8_t* o, uint32_t v) {
    o[0] = (uint8_t)(v >> 24);
    o[1] = (uint8_t)(v >> 16);
    o[2] = (uint8_t)(v >> 8);
    o[3] = (uint8_t)v;
}

// length, type, CRC around `len` payload bytes already at at + 8; returns the position behind the chunk
size_t close_chunk(uint8_t* out, size_t at, const char* type, size_t len) {
    put_be32(out + at, (uint32_t)len);
    std::memcpy(out + at + 4, type, 4);
    put_be32(out + at + 8 + len, crc32_of(out + at + 4, 4 + len));
    return at + 12 + len;
}

size_t stream_bytes(int H, int W, int channels) { return (size_t)H * (1 + (size_t)W * (size_t)channels); }
size_t chunks_of(size_t n) { return (n + PNG_CHUNK - 1) / PNG_CHUNK; }
size_t deflate_bound(size_t n) { return 2 + chunks_of(n) * 5 + n + 2 + 4; }       // zlib header, a stored block per chunk, 03 00, Adler-32
size_t iccp_payload(size_t icc) { return 12 + 1 + 2 + (icc + 65534) / 65535 * 5 + icc + 4; }   // "ICC Profile\0", method, the zlib stream

struct PngRun {
    int chunks;
    uint32_t* hist;
    PngRec* rec;
    unsigned long long* off;          // [chunks + 1]: sizes, then (after the scan) offsets and the total
    uint32_t* adler;                  // [chunks][2]
};

// The scratch of stages B and C for a stream of n bytes, behind `base` bytes of the slot's arena (where the caller's filtered stream lies:
// *arena_stream)
PngRun png_plan(bbocr_ctx* c, size_t n, size_t base, uint8_t** arena_stream) {
    PngRun r{};
    r.chunks = (int)chunks_of(n);
    Carve cv;
    cv.off = align_up(base, 256);
    const size_t o_hist = cv.add((size_t)r.chunks * PNG_HIST_ROW * 4), o_rec = cv.add((size_t)r.chunks * sizeof(PngRec));
    const size_t o_off = cv.add((size_t)(r.chunks + 1) * 8), o_adler = cv.add((size_t)r.chunks * 8);
    c->arena.buf.ensure(cv.off);
    if (arena_stream) *arena_stream = Carve::at<uint8_t>(c->arena.buf.p, 0);
    r.hist = Carve::at<uint32_t>(c->arena.buf.p, o_hist);
    r.rec = Carve::at<PngRec>(c->arena.buf.p, o_rec);
    r.off = Carve::at<unsigned long long>(c->arena.buf.p, o_off);
    r.adler = Carve::at<uint32_t>(c->arena.buf.p, o_adler);
    return r;
}

// Stages B and C of a device byte stream: the token / code pass and the scan of the chunk sizes
void png_enqueue_codes(bbocr_ctx* c, const PngRun& r, const uint8_t* stream, size_t n) {
    HIPCHK(launch_png_codes(stream, n, r.chunks, r.hist, r.rec, r.off, r.adler, c->stream));
    HIPCHK(launch_je_scan(r.off, r.chunks, c->stream));
}

// Stages D and E + the zlib framing: header 78 01, the chunks' blocks, the final empty fixed block 03 00, the Adler-32 of the n stream
// bytes combined from the chunks' sums.  Returns the bytes written at `out` (the caller has checked its capacity against deflate_bound).
size_t png_zlib_stream(bbocr_ctx* c, const PngRun& r, const uint8_t* stream, size_t n, uint8_t* out) {
    c->pe_out.ensure(std::max<size_t>(deflate_bound(n), 256));
    HIPCHK(launch_png_pack(stream, n, r.chunks, r.rec, r.off, (uint8_t*)c->pe_out.p, c->stream));
    unsigned long long total = 0;
    std::vector<uint32_t> sums((size_t)r.chunks * 2);
    HIPCHK(hipMemcpyAsync(&total, r.off + r.chunks, 8, hipMemcpyDeviceToHost, c->stream));
    if (r.chunks) HIPCHK(hipMemcpyAsync(sums.data(), r.adler, sums.size() * 4, hipMemcpyDeviceToHost, c->stream));
    slot_sync(c, c->stream);
    if (total > (unsigned long long)r.chunks * 5 + n) fail(BBOCR_ERR_INTERNAL, "the deflate blocks exceed their bound");
    out[0] = 0x78;
    out[1] = 0x01;
    if (total) HIPCHK(hipMemcpyAsync(out + 2, c->pe_out.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    uint32_t a = 1, b = 0;
    for (int k = 0; k < r.chunks; ++k) {                       // a chunk of m bytes with sums (A, B) from a zero state: b += m * a + B, a += A
        const size_t m = std::min<size_t>(PNG_CHUNK, n - (size_t)k * PNG_CHUNK);
        b = (uint32_t)((b + (unsigned long long)m * a + sums[2 * k + 1]) % kAdlerMod);
        a = (a + sums[2 * k]) % kAdlerMod;
    }
    slot_sync(c, c->stream);
    size_t at = 2 + (size_t)total;
    out[at++] = 0x03;
    out[at++] = 0x00;
    put_be32(out + at, (b << 16) | a);
    return at + 4;
}

unsigned png_layouts() { return page_set(PAGE_GRAY) | page_set(PAGE_BGR) | page_set(PAGE_RGB); }

}  // namespace

extern "C" {

size_t bbocr_png_encode_bound(int H, int W, int channels, size_t icc_bytes) {
    if (H < 1 || W < 1 || (channels != 1 && channels != 3) || icc_bytes > kPngMax) return 0;
    const size_t stream = stream_bytes(H, W, channels);
    if (stream > kPngMax || deflate_bound(stream) > kPngMax || (icc_bytes && iccp_payload(icc_bytes) > kPngMax)) return 0;   // a chunk's length is a 31-bit field
    return kFrame + (icc_bytes ? 12 + iccp_payload(icc_bytes) : 0) + chunks_of(stream) * 5 + stream + 2 + 4;
}

int bbocr_png_encode(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, const uint8_t* icc, size_t icc_bytes,
                     uint8_t* host_out, size_t capacity, size_t* bytes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        check_page({dev_src, H, W, pitch, layout}, png_layouts());
        if (!host_out || !bytes || (icc_bytes > 0 && !icc)) fail(BBOCR_ERR_ARG, "null pointer");
        const int channels = layout == PAGE_GRAY ? 1 : 3;
        const size_t bound = bbocr_png_encode_bound(H, W, channels, icc_bytes);
        if (bound == 0) fail(BBOCR_ERR_ARG, "the page or the profile is too large for a PNG file");
        if (capacity < bound) fail(BBOCR_ERR_ARG, "capacity below bbocr_png_encode_bound");
        const size_t n = stream_bytes(H, W, channels);
        uint8_t* stream = nullptr;
        const PngRun r = png_plan(ctx, n, n, &stream);
        HIPCHK(launch_png_filter(dev_src, (size_t)pitch, layout, H, W, stream, ctx->stream));
        png_enqueue_codes(ctx, r, stream, n);
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        std::memcpy(host_out, sig, 8);
        size_t at = 8;
        uint8_t* p = host_out + at + 8;
        put_be32(p, (uint32_t)W);
        put_be32(p + 4, (uint32_t)H);
        p[8] = 8;                                              // bit depth
        p[9] = channels == 1 ? 0 : 2;                          // colour type
        p[10] = p[11] = p[12] = 0;                             // deflate, adaptive filtering, no interlace
        at = close_chunk(host_out, at, "IHDR", 13);
        if (icc_bytes) {
            p = host_out + at + 8;
            std::memcpy(p, "ICC Profile", 12);                 // with its terminating zero
            p[12] = 0;                                         // compression method
            size_t q = 13;
            p[q++] = 0x78;
            p[q++] = 0x01;
            for (size_t done = 0; done < icc_bytes;) {
                const size_t m = std::min<size_t>(65535, icc_bytes - done);
                p[q++] = done + m == icc_bytes ? 1 : 0;        // BFINAL, BTYPE 00
                p[q++] = (uint8_t)(m & 255);
                p[q++] = (uint8_t)(m >> 8);
                p[q++] = (uint8_t)(~m & 255);
                p[q++] = (uint8_t)((~m >> 8) & 255);
                std::memcpy(p + q, icc + done, m);
                q += m;
                done += m;
            }
            put_be32(p + q, adler32_of(icc, icc_bytes));
            at = close_chunk(host_out, at, "iCCP", q + 4);
        }
        const size_t z = png_zlib_stream(ctx, r, stream, n, host_out + at + 8);
        at = close_chunk(host_out, at, "IDAT", z);
        at = close_chunk(host_out, at, "IEND", 0);
        if (at > capacity) fail(BBOCR_ERR_INTERNAL, "the file exceeds its bound");
        *bytes = at;
    });
}

int bbocr_op_deflate(bbocr_ctx* ctx, const uint8_t* dev_bytes, size_t n, uint8_t* host_out, size_t capacity, size_t* bytes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if ((n > 0 && !dev_bytes) || !host_out || !bytes) fail(BBOCR_ERR_ARG, "null pointer");
        if (n > kPngMax) fail(BBOCR_ERR_ARG, "at most 2^31 - 1 bytes");
        if (capacity < deflate_bound(n)) fail(BBOCR_ERR_ARG, "capacity below 2 + ceil(n / 16384) * 5 + n + 6");
        const PngRun r = png_plan(ctx, n, 0, nullptr);
        png_enqueue_codes(ctx, r, dev_bytes, n);
        *bytes = png_zlib_stream(ctx, r, dev_bytes, n, host_out);
    });
}

int bbocr_op_png_stage(bbocr_ctx* ctx, int stage, const uint8_t* dev_src, int H, int W, long long pitch, int layout, size_t n, void* dev_dst,
                       size_t dst_bytes, size_t* bytes) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_dst || !bytes || stage < 0 || stage > 3) fail(BBOCR_ERR_ARG, "bad arguments");
        if (stage == 0) {
            check_page({dev_src, H, W, pitch, layout}, png_layouts());
            const int channels = layout == PAGE_GRAY ? 1 : 3;
            if (bbocr_png_encode_bound(H, W, channels, 0) == 0) fail(BBOCR_ERR_ARG, "the page is too large for a PNG file");
            const size_t need = stream_bytes(H, W, channels);
            if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
            ctx->arena.buf.ensure(need);
            uint8_t* stream = (uint8_t*)ctx->arena.buf.p;
            HIPCHK(launch_png_filter(dev_src, (size_t)pitch, layout, H, W, stream, ctx->stream));
            HIPCHK(hipMemcpyAsync(dev_dst, stream, need, hipMemcpyDeviceToDevice, ctx->stream));
            slot_sync(ctx, ctx->stream);
            *bytes = need;
            return;
        }
        if ((n > 0 && !dev_src) || n > kPngMax) fail(BBOCR_ERR_ARG, "bad byte stream");
        const size_t chunks = chunks_of(n);
        const size_t need = stage == 1 ? chunks * PNG_HIST_ROW * 4 : (stage == 2 ? chunks * sizeof(PngRec) : (chunks + 1) * 8);
        if (dst_bytes < need) fail(BBOCR_ERR_ARG, "destination too small for the stage");
        const PngRun r = png_plan(ctx, n, 0, nullptr);
        png_enqueue_codes(ctx, r, dev_src, n);
        const void* from = stage == 1 ? (const void*)r.hist : (stage == 2 ? (const void*)r.rec : (const void*)r.off);
        if (need) HIPCHK(hipMemcpyAsync(dev_dst, from, need, hipMemcpyDeviceToDevice, ctx->stream));
        slot_sync(ctx, ctx->stream);
        *bytes = need;
    });
}

}  // extern "C"
