// The chunk walk behind bbocr_host_png_plan and the device PNG decoder's admission (pngdec.cpp): host only, no HIP, so that
// tools/pngdec_hostcheck.cpp compiles it as it stands.  One pass over the chunks; no compressed bit is decoded.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "bbocr.h"

namespace png_host {

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline uint32_t crc32_of(const uint8_t* p, size_t n) {
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

struct PngParsed {
    bbocr_png_plan plan{};
    std::vector<std::pair<size_t, size_t>> idat;   // (offset, length) of every IDAT payload, in file order
    uint8_t palette[768] = {0};
};

constexpr long long kPngStreamMax = 0x7FFFFFFFLL;
constexpr long long kPngMaxPixels = 2LL * 89478485LL;   // above it Pillow's decode raises (twice Image.MAX_IMAGE_PIXELS): the file keeps the host path and its error

// -> the BBOCR_PNG_* reason (also in ps.plan.reason; plan.supported = 1 for BBOCR_PNG_OK)
inline int png_parse(const uint8_t* f, size_t n, PngParsed& ps) {
    bbocr_png_plan& pl = ps.plan;
    pl = bbocr_png_plan{};
    ps.idat.clear();
    auto refuse = [&](int reason) {
        pl.supported = 0;
        pl.reason = reason;
        return reason;
    };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || std::memcmp(f, sig, 8) != 0) return refuse(BBOCR_PNG_NOT_PNG);
    size_t at = 8;
    bool first = true, seen_idat = false, last_idat = false, seen_plte = false, seen_end = false;
    while (!seen_end) {
        if (n - at < 12) return refuse(BBOCR_PNG_TRUNCATED);
        const uint32_t len = be32(f + at);
        if (len > 0x7FFFFFFFu || (size_t)len > n - at - 12) return refuse(BBOCR_PNG_TRUNCATED);
        const uint8_t* type = f + at + 4;
        const uint8_t* data = f + at + 8;
        auto is = [&](const char* t) { return std::memcmp(type, t, 4) == 0; };
        // every chunk's CRC-32, the ancillary ones included: Pillow, whose decode the device replaces, refuses the file for any of them
        if (crc32_of(type, 4 + (size_t)len) != be32(data + len)) return refuse(BBOCR_PNG_CRC);
        if (first) {
            if (!is("IHDR") || len != 13) return refuse(BBOCR_PNG_HEADER);
            first = false;
            const uint32_t w = be32(data), h = be32(data + 4);
            const int depth = data[8], ct = data[9];
            pl.bit_depth = depth;
            pl.color_type = ct;
            if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return refuse(BBOCR_PNG_DIMENSIONS);
            pl.width = (int)w;
            pl.height = (int)h;
            if (ct != 0 && ct != 2 && ct != 3 && ct != 4 && ct != 6) return refuse(BBOCR_PNG_HEADER);
            const bool pow2 = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
            const bool legal = pow2 && (ct == 0 || (ct == 3 && depth <= 8) || ((ct == 2 || ct == 4 || ct == 6) && depth >= 8));
            if (!legal || depth == 16) return refuse(BBOCR_PNG_DEPTH);
            pl.channels = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
            pl.bpp = depth == 8 ? pl.channels : 1;
            pl.row_bytes = ((long long)w * pl.channels * depth + 7) / 8;
            if (data[10] != 0 || data[11] != 0 || data[12] > 1) return refuse(BBOCR_PNG_HEADER);
            if (data[12] == 1) return refuse(BBOCR_PNG_INTERLACE);
            if (pl.row_bytes + 1 > kPngStreamMax / (long long)h || (long long)w * (long long)h > kPngMaxPixels) return refuse(BBOCR_PNG_DIMENSIONS);
        } else if (is("IHDR")) {
            return refuse(BBOCR_PNG_HEADER);
        } else if (is("PLTE")) {
            if (seen_idat || seen_plte || len == 0 || len > 768 || len % 3) return refuse(BBOCR_PNG_PALETTE);
            seen_plte = true;
            pl.palette_entries = (int)(len / 3);
            std::memcpy(ps.palette, data, len);
        } else if (is("acTL")) {
            return refuse(BBOCR_PNG_APNG);
        } else if (is("IDAT")) {
            if (seen_idat && !last_idat) return refuse(BBOCR_PNG_IDAT_ORDER);
            if (pl.color_type == 3 && !seen_plte) return refuse(BBOCR_PNG_PALETTE);
            seen_idat = true;
            ps.idat.emplace_back((size_t)(data - f), (size_t)len);
            pl.idat_chunks += 1;
            pl.idat_bytes += len;
        } else if (is("IEND")) {
            seen_end = true;
        }
        last_idat = is("IDAT");
        at += 12 + (size_t)len;
    }
    if (!seen_idat) return refuse(BBOCR_PNG_HEADER);
    if (pl.idat_bytes < 2) return refuse(BBOCR_PNG_ZLIB);
    uint8_t z[2];
    int got = 0;
    for (size_t k = 0; k < ps.idat.size() && got < 2; ++k)
        for (size_t i = 0; i < ps.idat[k].second && got < 2; ++i) z[got++] = f[ps.idat[k].first + i];
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || (z[1] & 0x20) || ((z[0] << 8) | z[1]) % 31) return refuse(BBOCR_PNG_ZLIB);
    pl.supported = 1;
    pl.reason = BBOCR_PNG_OK;
    return BBOCR_PNG_OK;
}

// the IDAT payloads back to back at dst[0 .. plan.idat_bytes)
inline void png_gather(const uint8_t* f, const PngParsed& ps, uint8_t* dst) {
    for (const auto& c : ps.idat) {
        std::memcpy(dst, f + c.first, c.second);
        dst += c.second;
    }
}

}  // namespace png_host
