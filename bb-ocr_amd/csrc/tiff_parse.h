// The IFD walk behind bbocr_host_tiff_plan and the device TIFF decoder's admission (tiffdec.cpp): host only, no HIP, so that
// tools/tiffdec_hostcheck.cpp compiles it as it stands.  One walk over the header and the FIRST IFD (Pillow's frame 0); no strip is decoded.
// The order of the checks is the order of tests/tiff_decode_ref.py's walk: a file with two faults names the same one in both.
// tiff_fax_parse (bbocr_host_tiff_fax_plan, the admission of bbocr_tiff_decode_fax) is the same walk in its LENIENT mode -- it notes a CCITT
// compression and a fill order other than 1, goes on and finishes its checks -- followed by the checks of the CCITT decoder
// (tests/tiff_fax_ref.py's fax_walk).
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "bbocr.h"

namespace tiff_host {

struct TiffParsed {
    bbocr_tiff_plan plan{};
    std::vector<std::pair<size_t, size_t>> strips;   // (offset, stored bytes) of every strip, top to bottom
    uint8_t palette[768] = {0};                      // photometric 3: R G B per index, the ColorMap's high bytes
};

struct TiffLenient {                                 // what the lenient walk went past
    bool ccitt = false, fill = false;
    uint32_t fill_order = 1, options = 0;            // FillOrder as stored; tag 292 (compression 3) or 293 (compression 4)
    bool options_sound = true;                       // that tag is absent, or a BYTE / SHORT / LONG value inside the file
};

constexpr long long kTiffStreamMax = 0x7FFFFFFFLL;
constexpr long long kTiffMaxPixels = 2LL * 89478485LL;   // above it Pillow's decode raises (twice Image.MAX_IMAGE_PIXELS)

// -> the BBOCR_TIFF_* reason (also in ps.plan.reason; plan.supported = 1 for BBOCR_TIFF_OK)
inline int tiff_parse(const uint8_t* f, size_t n, TiffParsed& ps, TiffLenient* lenient = nullptr) {
    bbocr_tiff_plan& pl = ps.plan;
    pl = bbocr_tiff_plan{};
    pl.extra_sample = -1;
    ps.strips.clear();
    auto refuse = [&](int reason) {
        pl.supported = 0;
        pl.reason = reason;
        return reason;
    };
    if (n < 8) return refuse(BBOCR_TIFF_NOT_TIFF);
    const bool be = f[0] == 'M' && f[1] == 'M';
    if (!be && !(f[0] == 'I' && f[1] == 'I')) return refuse(BBOCR_TIFF_NOT_TIFF);
    pl.big_endian = be ? 1 : 0;
    auto u16 = [&](size_t at) -> uint32_t { return be ? ((uint32_t)f[at] << 8) | f[at + 1] : ((uint32_t)f[at + 1] << 8) | f[at]; };
    auto u32 = [&](size_t at) -> uint32_t { return be ? (u16(at) << 16) | u16(at + 2) : (u16(at + 2) << 16) | u16(at); };
    const uint32_t magic = u16(2);
    if (magic == 43) return refuse(BBOCR_TIFF_BIGTIFF);
    if (magic != 42) return refuse(BBOCR_TIFF_NOT_TIFF);
    const size_t ifd = u32(4);
    if (ifd > n || n - ifd < 2) return refuse(BBOCR_TIFF_TRUNCATED);
    const size_t entries = u16(ifd);
    if ((n - ifd - 2) / 12 < entries) return refuse(BBOCR_TIFF_TRUNCATED);

    // the tags read here; a tag that occurs twice counts as its last entry
    enum { T_WIDTH, T_HEIGHT, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_FILL, T_OFFSETS, T_SAMPLES, T_ROWS, T_COUNTS, T_PLANAR, T_PREDICTOR, T_COLORMAP,
           T_EXTRA, T_FORMAT, T_T4OPTIONS, T_T6OPTIONS, T_N };
    static const uint16_t ids[T_N] = {256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 320, 338, 339, 292, 293};
    long long at_entry[T_N];
    for (int t = 0; t < T_N; ++t) at_entry[t] = -1;
    bool tiles = false;
    for (size_t e = 0; e < entries; ++e) {
        const size_t at = ifd + 2 + 12 * e;
        const uint32_t tag = u16(at);
        if (tag >= 322 && tag <= 325) tiles = true;
        for (int t = 0; t < T_N; ++t)
            if (ids[t] == tag) at_entry[t] = (long long)at;
    }
    // the values of tag t -> v (0: absent; else the reason; v.size() >= 1 on success with *present)
    auto values = [&](int t, std::vector<uint32_t>& v, bool& present) -> int {
        v.clear();
        present = at_entry[t] >= 0;
        if (!present) return 0;
        const size_t at = (size_t)at_entry[t];
        const uint32_t type = u16(at + 2), count = u32(at + 4);
        const size_t size = type == 1 ? 1 : (type == 3 ? 2 : (type == 4 ? 4 : 0));
        if (!size || count == 0) return BBOCR_TIFF_HEADER;
        size_t from = at + 8;
        if ((unsigned long long)count * size > 4) {
            from = u32(at + 8);
            if (from > n || (n - from) / size < count) return BBOCR_TIFF_TRUNCATED;
        }
        v.resize(count);
        for (uint32_t i = 0; i < count; ++i) v[i] = size == 1 ? f[from + i] : (size == 2 ? u16(from + 2 * (size_t)i) : u32(from + 4 * (size_t)i));
        return 0;
    };
    std::vector<uint32_t> v, bits, extra, offs, counts, cmap;
    bool has = false;
    int r;
    auto scalar = [&](int t, uint32_t dflt, bool required, uint32_t& out) -> int {
        if ((r = values(t, v, has))) return r;
        if (!has && required) return BBOCR_TIFF_HEADER;
        out = has ? v[0] : dflt;
        return 0;
    };
    if (tiles) return refuse(BBOCR_TIFF_TILES);
    uint32_t w = 0, h = 0, comp = 1, phot = 0, fill = 1, samples = 1, rows = 0xFFFFFFFFu, planar = 1, pred = 1;
    if ((r = scalar(T_WIDTH, 0, true, w)) || (r = scalar(T_HEIGHT, 0, true, h))) return refuse(r);
    if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return refuse(BBOCR_TIFF_DIMENSIONS);
    pl.width = (int)w;
    pl.height = (int)h;
    if ((long long)w * (long long)h > kTiffMaxPixels) return refuse(BBOCR_TIFF_DIMENSIONS);
    if ((r = scalar(T_COMPRESSION, 1, false, comp))) return refuse(r);
    pl.compression = (int)comp;
    if (comp == 6 || comp == 7) return refuse(BBOCR_TIFF_JPEG);
    if (comp >= 2 && comp <= 4) {
        if (!lenient) return refuse(BBOCR_TIFF_CCITT);
        lenient->ccitt = true;
    } else if (comp != 1 && comp != 5 && comp != 8 && comp != 32946 && comp != 32773) return refuse(BBOCR_TIFF_COMPRESSION);
    if ((r = scalar(T_PLANAR, 1, false, planar))) return refuse(r);
    if (planar != 1) return refuse(BBOCR_TIFF_PLANAR);
    if ((r = scalar(T_FILL, 1, false, fill))) return refuse(r);
    if (fill != 1) {
        if (!lenient) return refuse(BBOCR_TIFF_FILL_ORDER);
        lenient->fill = true;
        lenient->fill_order = fill;
    }
    if ((r = scalar(T_SAMPLES, 1, false, samples))) return refuse(r);
    if (samples == 0 || samples > 64) return refuse(BBOCR_TIFF_SAMPLES);
    pl.samples = (int)samples;
    if ((r = values(T_BITS, bits, has))) return refuse(r);
    if (!has) bits.assign(1, 1);
    if (bits.size() != samples) return refuse(BBOCR_TIFF_HEADER);
    pl.bits = (int)bits[0];
    for (uint32_t b : bits)
        if (b != bits[0]) return refuse(BBOCR_TIFF_DEPTH);
    if ((r = values(T_FORMAT, v, has))) return refuse(r);
    if (has)
        for (uint32_t s : v)
            if (s != 1) return refuse(BBOCR_TIFF_DEPTH);
    if (bits[0] == 2 || bits[0] == 4) return refuse(BBOCR_TIFF_SUBBYTE);
    if (bits[0] != 1 && bits[0] != 8) return refuse(BBOCR_TIFF_DEPTH);
    if ((r = scalar(T_PHOTOMETRIC, 0, true, phot))) return refuse(r);
    pl.photometric = (int)phot;
    if (phot > 3) return refuse(BBOCR_TIFF_PHOTOMETRIC);
    if ((r = values(T_EXTRA, extra, has))) return refuse(r);
    if (phot <= 1) {
        if (samples == 2) return refuse(BBOCR_TIFF_GRAY_ALPHA);
        if (samples != 1) return refuse(BBOCR_TIFF_SAMPLES);
    } else if (phot == 2) {
        if (bits[0] != 8) return refuse(BBOCR_TIFF_DEPTH);
        if (samples == 4) {
            if (extra.size() != 1) return refuse(BBOCR_TIFF_SAMPLES);
            if (extra[0] == 1) return refuse(BBOCR_TIFF_ASSOC_ALPHA);
            if (extra[0] != 0 && extra[0] != 2) return refuse(BBOCR_TIFF_SAMPLES);
            pl.extra_sample = (int)extra[0];
        } else if (samples != 3) {
            return refuse(BBOCR_TIFF_SAMPLES);
        }
    } else {
        if (bits[0] != 8) return refuse(BBOCR_TIFF_DEPTH);
        if (samples != 1) return refuse(BBOCR_TIFF_SAMPLES);
        if ((r = values(T_COLORMAP, cmap, has)) == BBOCR_TIFF_TRUNCATED) return refuse(r);
        const bool shorts = has && !r && u16((size_t)at_entry[T_COLORMAP] + 2) == 3;
        if (!shorts || cmap.size() != 768) return refuse(BBOCR_TIFF_PALETTE);
        for (int i = 0; i < 256; ++i)
            for (int c = 0; c < 3; ++c) ps.palette[3 * i + c] = (uint8_t)(cmap[256 * c + i] >> 8);
    }
    pl.row_bytes = ((long long)w * samples * bits[0] + 7) / 8;
    if (pl.row_bytes > kTiffStreamMax / (long long)h) return refuse(BBOCR_TIFF_DIMENSIONS);
    if ((r = scalar(T_PREDICTOR, 1, false, pred))) return refuse(r);
    pl.predictor = (int)pred;
    if (pred != 1 && !(pred == 2 && bits[0] == 8 && (comp == 5 || comp == 8 || comp == 32946))) return refuse(BBOCR_TIFF_PREDICTOR);
    if ((r = scalar(T_ROWS, 0xFFFFFFFFu, false, rows))) return refuse(r);
    if (rows == 0) return refuse(BBOCR_TIFF_STRIPS);
    if (rows > h) rows = h;
    pl.rows_per_strip = rows;
    const uint32_t nstrips = (h + rows - 1) / rows;
    pl.strips = (int)nstrips;
    bool has_counts = false;
    if ((r = values(T_OFFSETS, offs, has)) == BBOCR_TIFF_TRUNCATED) return refuse(r);
    int r2;
    if ((r2 = values(T_COUNTS, counts, has_counts)) == BBOCR_TIFF_TRUNCATED) return refuse(r2);
    if (r || r2) return refuse(BBOCR_TIFF_HEADER);
    if (!has || !has_counts || offs.size() != nstrips || counts.size() != nstrips) return refuse(BBOCR_TIFF_STRIPS);
    for (uint32_t s = 0; s < nstrips; ++s) {
        if (offs[s] > n || counts[s] > n - offs[s]) return refuse(BBOCR_TIFF_TRUNCATED);
        ps.strips.emplace_back((size_t)offs[s], (size_t)counts[s]);
        pl.strip_bytes += counts[s];
    }
    if (comp == 5 && counts[0] >= 2 && f[offs[0]] == 0 && (f[offs[0] + 1] & 1)) return refuse(BBOCR_TIFF_OLD_LZW);
    if (lenient && (comp == 3 || comp == 4)) {
        lenient->options_sound = !values(comp == 3 ? T_T4OPTIONS : T_T6OPTIONS, v, has);
        lenient->options = has && lenient->options_sound ? v[0] : 0;
    }
    pl.supported = 1;
    pl.reason = BBOCR_TIFF_OK;
    return BBOCR_TIFF_OK;
}

// -> ps.plan.supported; ps.plan as for a supported file when the plain or the fax plan takes it, else with the plain walk's reason
inline bool tiff_fax_parse(const uint8_t* f, size_t n, TiffParsed& ps, bbocr_tiff_fax& fax) {
    fax = bbocr_tiff_fax{};
    fax.fill_order = 1;
    TiffLenient seen;
    const int r = tiff_parse(f, n, ps, &seen);
    bbocr_tiff_plan& pl = ps.plan;
    if (!seen.ccitt && !seen.fill) {
        fax.reason = r == BBOCR_TIFF_OK ? BBOCR_FAX_OK : BBOCR_FAX_PLAIN;
        return r == BBOCR_TIFF_OK;
    }
    fax.fill_order = (int)seen.fill_order;
    if (r != BBOCR_TIFF_OK) {
        fax.reason = BBOCR_FAX_PLAIN;
        return false;
    }
    fax.scheme = seen.ccitt ? pl.compression : 0;
    fax.t4_options = (int)seen.options;
    auto refuse = [&](int reason) {
        pl.supported = 0;
        pl.reason = seen.ccitt ? BBOCR_TIFF_CCITT : BBOCR_TIFF_FILL_ORDER;
        fax.reason = reason;
        return false;
    };
    if (!seen.options_sound) return refuse(BBOCR_FAX_OPTIONS);
    if ((seen.fill_order != 1 && seen.fill_order != 2) || !seen.ccitt) return refuse(BBOCR_FAX_FILL_ORDER);
    if (pl.bits != 1 || pl.samples != 1) return refuse(BBOCR_FAX_DEPTH);       // (one 1-bit sample: the walk has refused a photometric above 1)
    if (seen.options & (pl.compression == 3 ? ~5u : ~0u)) return refuse(BBOCR_FAX_OPTIONS);
    if (pl.width > BBOCR_FAX_MAX_WIDTH) return refuse(BBOCR_FAX_WIDTH);
    return true;
}

// rows of strip s
inline long long tiff_strip_rows(const bbocr_tiff_plan& pl, int s) {
    const long long left = (long long)pl.height - (long long)s * pl.rows_per_strip;
    return left < pl.rows_per_strip ? left : pl.rows_per_strip;
}

}  // namespace tiff_host
