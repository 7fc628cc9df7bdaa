// The walk behind bbocr_host_bmp_plan and the device BMP decoder's admission (bmpdec.cpp): host only, no HIP.  Pillow's
// BmpImagePlugin._bitmap restated (bbocr.h; tests/bmp_decode_ref.py, whose walk checks in the same order: a file with two faults names the
// same one in both).  A file the plan supports has every byte the kernel reads -- the table, height rows of row_stride bytes from
// data_offset -- inside it.
#pragma once
#include <cstdint>
#include <cstring>

#include "bbocr.h"

namespace bmp_host {

constexpr long long kBmpMaxPixels = 2LL * 89478485LL;    // above it Pillow's open raises (twice Image.MAX_IMAGE_PIXELS)

// -> the BBOCR_BMP_* reason (also in pl.reason; pl.supported = 1 for BBOCR_BMP_OK)
inline int bmp_parse(const uint8_t* f, size_t n, bbocr_bmp_plan& pl) {
    pl = bbocr_bmp_plan{};
    auto refuse = [&](int reason) {
        pl.supported = 0;
        pl.reason = reason;
        return reason;
    };
    if (n < 2 || f[0] != 'B' || f[1] != 'M') return refuse(BBOCR_BMP_NOT_BMP);
    if (n < 18) return refuse(BBOCR_BMP_TRUNCATED);
    auto u16 = [&](size_t at) -> uint32_t { return (uint32_t)f[at] | ((uint32_t)f[at + 1] << 8); };
    auto u32 = [&](size_t at) -> uint32_t { return u16(at) | (u16(at + 2) << 16); };
    unsigned long long offset = u32(10);
    const uint32_t hs = u32(14);
    pl.header_size = (int)(hs > 0x7FFFFFFFu ? 0x7FFFFFFFu : hs);
    if (hs != 12 && hs != 40 && hs != 52 && hs != 56 && hs != 64 && hs != 108 && hs != 124) return refuse(BBOCR_BMP_HEADER);
    if (n < 14 + (size_t)hs) return refuse(BBOCR_BMP_TRUNCATED);
    size_t at = 14 + (size_t)hs;                     // Pillow's read position from here on
    unsigned long long w, h, colors;
    uint32_t bits, comp = 0;
    const unsigned entry = hs == 12 ? 3 : 4;
    if (hs == 12) {
        w = u16(18), h = u16(20), bits = u16(24), colors = 0;
    } else {
        w = u32(18), h = u32(22), bits = u16(28), comp = u32(30), colors = u32(46);
        if (f[25] == 0xFF) {
            h = (1ull << 32) - h;
            pl.top_down = 1;
        }
    }
    pl.bits = (int)bits;
    pl.compression = (int)(comp > 0x7FFFFFFFu ? 0x7FFFFFFFu : comp);
    if (w == 0 || h == 0 || w > 0x7FFFFFFFull || h > 0x7FFFFFFFull) return refuse(BBOCR_BMP_DIMENSIONS);
    pl.width = (int)w;
    pl.height = (int)h;
    if (w * h > (unsigned long long)kBmpMaxPixels) return refuse(BBOCR_BMP_PIXELS);
    if (!colors) colors = 1ull << (bits < 31 ? bits : 31);
    if (offset == 14ull + hs && bits <= 8) offset += entry * colors;     // the offset points AT the table: moved behind it
    if (bits != 1 && bits != 4 && bits != 8 && bits != 16 && bits != 24 && bits != 32) return refuse(BBOCR_BMP_DEPTH);
    pl.mode = 3;
    pl.r_at = 2, pl.g_at = 1, pl.b_at = 0;
    if (comp == 3) {
        uint32_t m[4] = {0, 0, 0, 0};
        if (hs >= 52) {
            m[0] = u32(54), m[1] = u32(58), m[2] = u32(62), m[3] = hs >= 56 ? u32(66) : 0;
        } else {
            if (n < at + 12) return refuse(BBOCR_BMP_TRUNCATED);
            m[0] = u32(at), m[1] = u32(at + 4), m[2] = u32(at + 8);
            at += 12;
        }
        // Pillow's SUPPORTED / MASK_MODES: (r, g, b, a) masks -> the bytes that hold R, G, B
        static const uint32_t k32[8][7] = {{0xFF0000, 0xFF00, 0xFF, 0, 2, 1, 0},          {0xFF000000u, 0xFF0000, 0xFF00, 0, 3, 2, 1},
                                           {0xFF000000u, 0xFF00, 0xFF, 0, 3, 1, 0},       {0xFF000000u, 0xFF0000, 0xFF00, 0xFF, 3, 2, 1},
                                           {0xFF, 0xFF00, 0xFF0000, 0xFF000000u, 0, 1, 2}, {0xFF0000, 0xFF00, 0xFF, 0xFF000000u, 2, 1, 0},
                                           {0xFF000000u, 0xFF00, 0xFF, 0xFF0000, 3, 1, 0}, {0, 0, 0, 0, 2, 1, 0}};
        bool ok = false;
        if (bits == 32) {
            for (const auto& k : k32)
                if (m[0] == k[0] && m[1] == k[1] && m[2] == k[2] && m[3] == k[3]) {
                    pl.r_at = (int)k[4], pl.g_at = (int)k[5], pl.b_at = (int)k[6];
                    ok = true;
                    break;
                }
        } else if (bits == 24) {
            ok = m[0] == 0xFF0000 && m[1] == 0xFF00 && m[2] == 0xFF;
        } else if (bits == 16) {
            ok = m[2] == 0x1F && ((m[0] == 0xF800 && m[1] == 0x7E0) || (m[0] == 0x7C00 && m[1] == 0x3E0));
            pl.six_bit_green = ok && m[1] == 0x7E0 ? 1 : 0;
        }
        if (!ok) return refuse(BBOCR_BMP_MASKS);
    } else if (comp == 1 || comp == 2) {
        return refuse(BBOCR_BMP_RLE);
    } else if (comp != 0) {
        return refuse(BBOCR_BMP_COMPRESSION);
    }
    if (bits <= 8) {
        if (colors > 65536) return refuse(BBOCR_BMP_PALETTE);
        pl.colors = (int)colors;
        pl.table_offset = (long long)at;
        pl.table_entry = (int)entry;
        if (n < at + entry * (size_t)colors) return refuse(BBOCR_BMP_TRUNCATED);
        bool gray = true;                            // black then white (two entries), else entry i = (i, i, i)
        for (size_t i = 0; i < (size_t)colors && gray; ++i) {
            const uint8_t v = colors == 2 ? (i ? 255 : 0) : (uint8_t)i;
            const uint8_t* e = f + at + entry * i;
            gray = e[0] == v && e[1] == v && e[2] == v;
        }
        at += entry * (size_t)colors;
        if (!gray) {
            if (colors > 256) return refuse(BBOCR_BMP_PALETTE);          // Pillow opens such a file and raises "invalid palette size" on load
            pl.mode = 0;
        } else if (bits == 1 && colors == 2) pl.mode = 1;
        else if (bits == 8 && colors != 2) pl.mode = 2;
        else return refuse(BBOCR_BMP_GRAY_TABLE);
    }
    pl.row_stride = (long long)(((w * bits + 31) >> 3) & ~3ull);
    pl.data_offset = (long long)(offset ? offset : (unsigned long long)at);
    if ((unsigned long long)n < (unsigned long long)pl.data_offset + (unsigned long long)pl.row_stride * h) return refuse(BBOCR_BMP_TRUNCATED);
    pl.supported = 1;
    pl.reason = BBOCR_BMP_OK;
    return BBOCR_BMP_OK;
}

}  // namespace bmp_host
