// The walk behind bbocr_host_gif_plan and the device GIF decoder's admission (gifdec.cpp): host only, no HIP, so that
// tools/gifdec_hostcheck.cpp compiles it as it stands.  One walk from the signature to the terminator of frame 0's data sub-blocks, which
// it de-frames into ps.payload; no code is decoded.  The order of the checks is the order of tests/gif_decode_ref.py's walk: a file with
// two faults names the same one in both.  Pillow's rules as restated: bbocr.h and the restatement's docstring.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "bbocr.h"

namespace gif_host {

struct GifParsed {
    bbocr_gif_plan plan{};
    std::vector<uint8_t> payload;                    // frame 0's data sub-blocks back to back
};

constexpr long long kGifMaxPixels = 2LL * 89478485LL;    // above it Pillow's open raises (twice Image.MAX_IMAGE_PIXELS)

inline bool gif_is_ramp(const uint8_t* t, int entries) {
    for (int i = 0; i < entries; ++i)
        if (t[3 * i] != i || t[3 * i + 1] != i || t[3 * i + 2] != i) return false;
    return true;
}

// -> the BBOCR_GIF_* reason (also in ps.plan.reason; plan.supported = 1 for BBOCR_GIF_OK)
inline int gif_parse(const uint8_t* f, size_t n, GifParsed& ps) {
    bbocr_gif_plan& pl = ps.plan;
    pl = bbocr_gif_plan{};
    pl.transparency = -1;
    ps.payload.clear();
    auto refuse = [&](int reason) {
        pl.supported = 0;
        pl.reason = reason;
        return reason;
    };
    if (n < 6 || (std::memcmp(f, "GIF87a", 6) != 0 && std::memcmp(f, "GIF89a", 6) != 0)) return refuse(BBOCR_GIF_NOT_GIF);
    if (n < 13) return refuse(BBOCR_GIF_TRUNCATED);
    auto u16 = [&](size_t at) -> int { return (int)f[at] | ((int)f[at + 1] << 8); };
    pl.screen_w = u16(6);
    pl.screen_h = u16(8);
    size_t at = 13;
    const uint8_t *table = nullptr, *global = nullptr;
    int tlen = 0, glen = 0;
    if (f[10] & 128) {
        tlen = glen = 2 << (f[10] & 7);
        if (n - at < 3 * (size_t)tlen) return refuse(BBOCR_GIF_TRUNCATED);
        table = global = f + at;
        at += 3 * (size_t)tlen;
    }
    for (;;) {                                       // the blocks before the first image descriptor
        if (at >= n) return refuse(BBOCR_GIF_TRUNCATED);
        const uint8_t tag = f[at++];
        if (tag == 0x3B) return refuse(BBOCR_GIF_NO_IMAGE);
        if (tag == 0x2C) break;
        if (tag != 0x21) return refuse(BBOCR_GIF_TRUNCATED);
        if (at >= n) return refuse(BBOCR_GIF_TRUNCATED);
        const uint8_t label = f[at++];
        bool first = true;
        for (;;) {
            if (at >= n) return refuse(BBOCR_GIF_TRUNCATED);
            const size_t size = f[at++];
            if (size == 0) break;
            if (n - at < size) return refuse(BBOCR_GIF_TRUNCATED);
            if (first && label == 0xF9) {            // graphic control: the last one that sets the flag counts
                if (size < 4) return refuse(BBOCR_GIF_TRUNCATED);
                if (f[at] & 1) pl.transparency = f[at + 3];
            }
            first = false;
            at += size;
        }
    }
    if (n - at < 9) return refuse(BBOCR_GIF_TRUNCATED);
    pl.x0 = u16(at);
    pl.y0 = u16(at + 2);
    pl.width = u16(at + 4);
    pl.height = u16(at + 6);
    const uint8_t flags = f[at + 8];
    at += 9;
    pl.interlace = (flags & 64) ? 1 : 0;
    if (flags & 128) {
        tlen = 2 << (flags & 7);
        if (n - at < 3 * (size_t)tlen) return refuse(BBOCR_GIF_TRUNCATED);
        table = f + at;
        at += 3 * (size_t)tlen;
        pl.local_table = 1;
    }
    pl.table_len = table ? tlen : 0;
    pl.canvas_w = pl.screen_w > pl.x0 + pl.width ? pl.screen_w : pl.x0 + pl.width;
    pl.canvas_h = pl.screen_h > pl.y0 + pl.height ? pl.screen_h : pl.y0 + pl.height;
    if (pl.width == 0 || pl.height == 0) return refuse(BBOCR_GIF_EMPTY);
    if ((long long)pl.canvas_w * (long long)pl.canvas_h > kGifMaxPixels) return refuse(BBOCR_GIF_PIXELS);
    pl.mode_l = (!table || gif_is_ramp(table, tlen)) ? 1 : 0;
    // the RGB plane's lookup (entries the table does not have: black); mode L: the ramp -- but behind a LOCAL ramp Pillow keeps a global
    // table that is none for convert("RGB"), while its gray plane stays the index
    if (!pl.mode_l) {
        std::memcpy(pl.table, table, 3 * (size_t)tlen);
    } else if (pl.local_table && global && !gif_is_ramp(global, glen)) {
        std::memcpy(pl.table, global, 3 * (size_t)glen);
    } else {
        for (int i = 0; i < 768; ++i) pl.table[i] = (uint8_t)(i / 3);
    }
    if (at >= n) return refuse(BBOCR_GIF_TRUNCATED);
    pl.min_code = f[at++];
    if (pl.min_code < 2 || pl.min_code > 8) return refuse(BBOCR_GIF_CODE_SIZE);
    for (;;) {
        if (at >= n) return refuse(BBOCR_GIF_TRUNCATED);
        const size_t size = f[at++];
        if (size == 0) break;
        if (n - at < size) return refuse(BBOCR_GIF_TRUNCATED);
        ps.payload.insert(ps.payload.end(), f + at, f + at + size);
        at += size;
    }
    pl.payload_bytes = (long long)ps.payload.size();
    pl.supported = 1;
    pl.reason = BBOCR_GIF_OK;
    return BBOCR_GIF_OK;
}

}  // namespace gif_host
