// Host-side JPEG parsing, the whole of it: EXIF orientation, Huffman table specs and their derived form, the removal of stuffing; one
// marker walk in pieces (next_segment, take_header, check_frame, take_quant, frame_mcus) under the two walks that differ in their SOS
// handling -- bbocr_host_jpeg_plan's (jpeg_parse) and bbocr_host_jpeg_progressive_plan's (prog_parse); and the tables of a scan as the
// device reads them (cut_scan: unstuffed segments cut into subsequences; prog_fill_scan: a progressive scan for jpegprog.h's
// jp_decode_segment).  The zig-zag order is jpeg_spec.h's JPEG_ZZ.  No GPU call: tools/jpegprog_hostcheck.cpp builds it with the sanitisers.
#pragma once
#include "../../include/bbocr.h"
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>
#include "jpegprog.h"

namespace jpeg_host {

struct HuffSpec { bool have = false; unsigned char counts[16] = {0}; unsigned char vals[256] = {0}; int total = 0; };

// EXIF orientation as cv2.imread applies it: the first APP1 segment that starts with "Exif\0\0" before SOS, a TIFF header of either byte
// order, IFD0 only, tag 0x0112 as one SHORT or LONG of value 1 .. 8.  Anything else -- no such segment or tag, another type or count,
// another value, an IFD that does not lie inside the segment -- is 1.  Every read is checked against the segment.
inline int exif_orientation(const uint8_t* f, size_t n) {
    size_t p = 2;
    while (p + 4 <= n && f[p] == 0xFF) {
        const int m = f[p + 1];
        if (m == 0xFF) { ++p; continue; }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }
        if (m == 0xDA || m == 0xD9) break;
        const size_t L = ((size_t)f[p + 2] << 8) | f[p + 3];
        if (L < 2 || p + 2 + L > n) break;
        const uint8_t* s = f + p + 4;
        const size_t sl = L - 2;
        p += 2 + L;
        if (m != 0xE1 || sl < 6 || std::memcmp(s, "Exif\0\0", 6) != 0) continue;
        const uint8_t* t = s + 6;
        const size_t tl = sl - 6;
        if (tl < 8) return 1;
        const bool le = t[0] == 'I' && t[1] == 'I';
        if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
        auto u16 = [&](size_t o) { return le ? (unsigned)t[o] | ((unsigned)t[o + 1] << 8) : ((unsigned)t[o] << 8) | (unsigned)t[o + 1]; };
        auto u32 = [&](size_t o) { return le ? u16(o) | (u16(o + 2) << 16) : (u16(o) << 16) | u16(o + 2); };
        if (u16(2) != 42) return 1;
        const size_t ifd = u32(4);
        if (ifd > tl || tl - ifd < 2) return 1;
        const size_t cnt = u16(ifd);
        if ((tl - ifd - 2) / 12 < cnt) return 1;                  // the directory runs off the segment
        for (size_t i = 0; i < cnt; ++i) {
            const size_t e = ifd + 2 + 12 * i;
            if (u16(e) != 0x0112) continue;
            const unsigned type = u16(e + 2);
            if ((type != 3 && type != 4) || u32(e + 4) != 1) return 1;
            const unsigned v = type == 3 ? u16(e + 8) : u32(e + 8);
            return v >= 1 && v <= 8 ? (int)v : 1;
        }
        return 1;
    }
    return 1;
}

// The chroma layouts beside 4:2:0 that the decoder takes: luma (1,1), (2,1) or (1,2) over chroma (1,1), (1,1).  0: any other sampling.
inline int chroma_class_of(const int s[3][2]) {
    if (s[1][0] != 1 || s[1][1] != 1 || s[2][0] != 1 || s[2][1] != 1) return 0;
    const int h = s[0][0], v = s[0][1];
    return h == 1 && v == 1 ? BBOCR_JPEG_CHROMA_444 : (h == 2 && v == 1 ? BBOCR_JPEG_CHROMA_422 : (h == 1 && v == 2 ? BBOCR_JPEG_CHROMA_440 : 0));
}

// jdhuff.c::jpeg_make_d_derived_tbl; false where it raises JERR_BAD_HUFF_TABLE: behind the codes of a length the next code no longer has
// that length (the counts do not describe a prefix code, or they assign the code of all ones), or a DC table (dc) names a category above 15
inline bool derive_table(const HuffSpec& h, JpegHuff& t, bool dc = false) {
    std::memset(&t, 0, sizeof t);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = h.counts[l - 1];
        t.valoff[l] = k - code;
        if (cnt) {
            if (code + cnt > (1 << l)) return false;
            for (int i = 0; i < cnt; ++i, ++k, ++code)
                if (l <= 9)
                    for (int e = 0; e < (1 << (9 - l)); ++e) t.look[(code << (9 - l)) + e] = (unsigned short)((l << 8) | h.vals[k]);
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        if (code >= (1 << l)) return false;
        code <<= 1;
    }
    if (dc)
        for (int i = 0; i < h.total; ++i)
            if (h.vals[i] > 15) return false;
    t.maxcode[0] = t.maxcode[17] = -1;
    std::memcpy(t.val, h.vals, 256);
    return true;
}

// one DHT segment's tables into huff[class][id], ids below `ids`; false: malformed
inline bool read_dht(const uint8_t* s, size_t sl, HuffSpec (&huff)[2][4], int ids) {
    size_t q = 0;
    while (q < sl) {
        if (q + 17 > sl) return false;
        const int tc = s[q] >> 4, th = s[q] & 15;
        int tot = 0;
        for (int i = 0; i < 16; ++i) tot += s[q + 1 + i];
        if (tc > 1 || th >= ids || tot > 256 || q + 17 + tot > sl) return false;
        HuffSpec& h = huff[tc][th];
        h.have = true;
        h.total = tot;
        std::memcpy(h.counts, s + q + 1, 16);
        std::memset(h.vals, 0, 256);
        std::memcpy(h.vals, s + q + 17, (size_t)tot);
        q += 17 + (size_t)tot;
    }
    return true;
}

// the bytes [a, e) of a restart segment without their stuffing: every FF is kept, the 00 behind it dropped.  Returns the count.
inline size_t unstuff(const uint8_t* a, const uint8_t* e, uint8_t* dst) {
    size_t w = 0;
    while (a < e) {                                                   // copy up to and including the next FF, drop the 00 behind it
        const uint8_t* ff = (const uint8_t*)std::memchr(a, 0xFF, (size_t)(e - a));
        const size_t len = ff ? (size_t)(ff - a) + 1 : (size_t)(e - a);
        std::memcpy(dst + w, a, len);
        w += len;
        a += len;
        if (ff && a < e && *a == 0x00) ++a;
    }
    return w;
}

// The entropy-coded data that starts at `from`: its restart segments' byte ranges (want_segs) and their number, up to the marker that
// ends it, whose FF is *end.  Fill bytes in front of a marker (T.81 B.1.1.2) are no entropy-coded data: a segment ends at the first FF of
// the run its marker closes.  BBOCR_JPEG_OK, _RESTART (markers out of sequence) or _NO_EOI (the data runs to the end of the file).
inline int scan_segments(const uint8_t* f, size_t n, size_t from, bool want_segs, std::vector<std::pair<size_t, size_t>>& segs, int& nseg,
                         size_t& end) {
    size_t q = from, start = from;
    nseg = 0;
    auto first_ff = [&](size_t at) {
        while (at > start && f[at - 1] == 0xFF) --at;
        return at;
    };
    while (q < n) {
        const void* hit = std::memchr(f + q, 0xFF, n - q);
        if (!hit) break;
        q = (size_t)((const uint8_t*)hit - f);
        if (q + 1 >= n) break;
        const int b = f[q + 1];
        if (b == 0x00) {
            q += 2;
        } else if (b == 0xFF) {
            q += 1;
        } else if (b >= 0xD0 && b <= 0xD7) {
            if (b - 0xD0 != nseg % 8) return BBOCR_JPEG_RESTART;
            if (want_segs) segs.emplace_back(start, first_ff(q));
            ++nseg;
            q += 2;
            start = q;
        } else {
            if (want_segs) segs.emplace_back(start, first_ff(q));
            ++nseg;
            end = q;
            return BBOCR_JPEG_OK;
        }
    }
    return BBOCR_JPEG_NO_EOI;
}

// ---- the marker walk: what bbocr_host_jpeg_plan's (jpeg_walk) and bbocr_host_jpeg_progressive_plan's (prog_walk) share.  Both keep
// the frame in a bbocr_jpeg_plan -- for a progressive file a plan without a scan, which is how the stages behind the coefficients see it.
struct JpegHeader {                                   // what the marker segments have said so far
    unsigned short qt[4][64];                         // natural order
    bool have_qt[4] = {false, false, false, false};
    HuffSpec huff[2][4];                              // [class][id]
    bool have_sof = false, jfif = false;
    int adobe = -1, comp_id[4] = {0}, comp_tq[4] = {0}, dri = 0;
};
struct JpegParsed {                                   // a baseline file, or the frame of a progressive one
    bbocr_jpeg_plan plan;
    unsigned short quant[3][64] = {};                 // per component, natural order
    HuffSpec huff[2][2];                              // [class][id]
    int tab_dc[3] = {0, 0, 0}, tab_ac[3] = {0, 0, 0};
    std::vector<std::pair<size_t, size_t>> segs;      // byte ranges of the restart segments in the file (stuffing included)
};

// The marker segment at or behind p: fill bytes, SOI, RSTn and TEM are passed over.  SEG_OK: marker g.m, payload g.s[g.sl], the next
// marker at g.next; SEG_EOI; SEG_LOST: no marker where one must stand; SEG_CUT: the segment runs off the file.
struct Segment { int m; const uint8_t* s; size_t sl, next; };
enum { SEG_OK = 0, SEG_EOI, SEG_LOST, SEG_CUT };
inline int next_segment(const uint8_t* f, size_t n, size_t p, Segment& g) {
    for (;;) {
        if (p + 2 > n || f[p] != 0xFF) return SEG_LOST;
        if (f[p + 1] == 0xFF) { ++p; continue; }
        g.m = f[p + 1];
        p += 2;
        if (g.m == 0xD8 || (g.m >= 0xD0 && g.m <= 0xD7) || g.m == 0x01) continue;
        if (g.m == 0xD9) return SEG_EOI;
        if (p + 2 > n) return SEG_CUT;
        const size_t L = ((size_t)f[p] << 8) | f[p + 1];
        if (L < 2 || p + L > n) return SEG_CUT;
        g.s = f + p + 2;
        g.sl = L - 2;
        g.next = p + L;
        return SEG_OK;
    }
}

// A segment of the headers: the frame header `sof` into the frame (every other SOFn is BBOCR_JPEG_SOF: the other walk's, extended,
// lossless, arithmetic), DHT with ids below dht_ids, DQT, DRI, JFIF and Adobe into h.  Any other segment is passed over.
inline int take_header(const Segment& g, int sof, int dht_ids, JpegHeader& h, bbocr_jpeg_plan& fr) {
    const uint8_t* s = g.s;
    const size_t sl = g.sl;
    const int m = g.m;
    if (m == sof) {
        if (h.have_sof || sl < 6) return BBOCR_JPEG_SOF;
        if (s[0] != 8) return BBOCR_JPEG_PRECISION;
        fr.height = (s[1] << 8) | s[2];
        fr.width = (s[3] << 8) | s[4];
        fr.components = s[5];
        if (fr.height == 0 || fr.width == 0 || sl < 6 + 3 * (size_t)fr.components) return BBOCR_JPEG_SOF;
        for (int i = 0; i < fr.components && i < 4; ++i) {
            h.comp_id[i] = s[6 + 3 * i];
            if (i < 3) { fr.sampling[i][0] = s[7 + 3 * i] >> 4; fr.sampling[i][1] = s[7 + 3 * i] & 15; }
            h.comp_tq[i] = s[8 + 3 * i];
        }
        h.have_sof = true;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
        return BBOCR_JPEG_SOF;
    } else if (m == 0xC4) {
        if (!read_dht(s, sl, h.huff, dht_ids)) return BBOCR_JPEG_TABLES;
    } else if (m == 0xDB) {
        size_t q = 0;
        while (q < sl) {
            if (s[q] >> 4) return BBOCR_JPEG_PRECISION;
            const int id = s[q] & 15;
            if (id > 3 || q + 65 > sl) return BBOCR_JPEG_TABLES;
            for (int k = 0; k < 64; ++k) h.qt[id][JPEG_ZZ[k]] = s[q + 1 + k];
            h.have_qt[id] = true;
            q += 65;
        }
    } else if (m == 0xDD) {
        if (sl < 2) return BBOCR_JPEG_TRUNCATED;
        h.dri = (s[0] << 8) | s[1];
    } else if (m == 0xE0 && sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) {
        h.jfif = true;
    } else if (m == 0xEE && sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
        h.adobe = s[11];
    }
    return BBOCR_JPEG_OK;
}

// The frame rules at the first SOS: 1 or 3 components, YCbCr, 4:2:0 or a chroma class (cls; 0 for 4:2:0 and for one component)
inline int check_frame(const JpegHeader& h, const bbocr_jpeg_plan& fr, int& cls) {
    cls = 0;
    if (!h.have_sof) return BBOCR_JPEG_SOF;
    if (fr.components != 1 && fr.components != 3) return BBOCR_JPEG_COMPONENTS;
    if (fr.components == 1) return BBOCR_JPEG_OK;
    if (!h.jfif && h.adobe != 1) return BBOCR_JPEG_COLORSPACE;
    const int(&s)[3][2] = fr.sampling;
    if (s[0][0] == 2 && s[0][1] == 2 && s[1][0] == 1 && s[1][1] == 1 && s[2][0] == 1 && s[2][1] == 1) return BBOCR_JPEG_OK;
    cls = chroma_class_of(s);
    return cls ? BBOCR_JPEG_OK : BBOCR_JPEG_SAMPLING;
}
// component i's quantisation table into quant[i]; false: the frame names one no DQT brought
inline bool take_quant(const JpegHeader& h, int i, unsigned short (&quant)[3][64]) {
    if (h.comp_tq[i] > 3 || !h.have_qt[h.comp_tq[i]]) return false;
    std::memcpy(quant[i], h.qt[h.comp_tq[i]], sizeof h.qt[0]);
    return true;
}
inline void frame_mcus(bbocr_jpeg_plan& fr) {
    const int mcu_w = fr.components == 3 ? 8 * fr.sampling[0][0] : 8, mcu_h = fr.components == 3 ? 8 * fr.sampling[0][1] : 8;
    fr.mcu_cols = (fr.width + mcu_w - 1) / mcu_w;
    fr.mcu_rows = (fr.height + mcu_h - 1) / mcu_h;
}

// ---- baseline files.  jdmarker.c's walk over the headers up to SOS, then over the entropy-coded data up to the marker that ends it.
// Returns the reason; `cls` receives the chroma class of a file whose sampling alone is outside bbocr_jpeg_plan::supported, and the walk
// goes on as for a supported file.
inline int jpeg_walk(const uint8_t* f, size_t n, JpegParsed& out, bool want_segs, int& cls) {
    bbocr_jpeg_plan& pl = out.plan;
    std::memset(&pl, 0, sizeof pl);
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return BBOCR_JPEG_NOT_JPEG;
    pl.orientation = exif_orientation(f, n);                     // of its own walk: malformed EXIF never changes what follows
    JpegHeader h;
    Segment g;
    for (size_t p = 2;; p = g.next) {
        if (next_segment(f, n, p, g) != SEG_OK) return BBOCR_JPEG_TRUNCATED;     // EOI before SOS and lost marker sync too
        if (g.m == 0xDA) break;
        const int r = take_header(g, 0xC0, 2, h, pl);
        if (r != BBOCR_JPEG_OK) return r;
    }
    const int r = check_frame(h, pl, cls);
    if (r != BBOCR_JPEG_OK) return r;
    const int nc = pl.components;
    if (g.sl < 1 || g.s[0] != nc || g.sl < 1 + 2 * (size_t)nc + 3) return BBOCR_JPEG_MULTISCAN;
    for (int i = 0; i < nc; ++i) {
        if (g.s[1 + 2 * i] != h.comp_id[i]) return BBOCR_JPEG_MULTISCAN;
        const int td = g.s[2 + 2 * i] >> 4, ta = g.s[2 + 2 * i] & 15;
        if (td > 1 || ta > 1 || !h.huff[0][td].have || !h.huff[1][ta].have || !take_quant(h, i, out.quant)) return BBOCR_JPEG_TABLES;
        JpegHuff probe;                                              // what libjpeg refuses when it derives the scan's tables
        if (!derive_table(h.huff[0][td], probe, true) || !derive_table(h.huff[1][ta], probe)) return BBOCR_JPEG_TABLES;
        out.tab_dc[i] = td;
        out.tab_ac[i] = 2 + ta;
    }
    for (int c = 0; c < 2; ++c)
        for (int id = 0; id < 2; ++id) out.huff[c][id] = h.huff[c][id];
    frame_mcus(pl);
    pl.restart_interval = h.dri;
    pl.scan_offset = (long long)g.next;
    const long long nmcu = (long long)pl.mcu_cols * pl.mcu_rows, ri = h.dri ? h.dri : nmcu;
    size_t end = 0;
    int nseg = 0;
    const int walked = scan_segments(f, n, g.next, want_segs, out.segs, nseg, end);
    if (walked != BBOCR_JPEG_OK) return walked;
    if (f[end + 1] != 0xD9) return BBOCR_JPEG_MULTISCAN;
    if ((long long)nseg != (nmcu + ri - 1) / ri) return BBOCR_JPEG_RESTART;
    pl.segments = nseg;
    pl.scan_bytes = (long long)(end - g.next);
    return BBOCR_JPEG_OK;
}

// The plan of a file and its reason.  A file of a chroma class that passed every later check keeps reason BBOCR_JPEG_SAMPLING and
// supported 0, with `chroma` set and the whole plan filled; one that failed a later check is refused as before, nothing behind the
// sampling test filled.
inline int jpeg_parse(const uint8_t* f, size_t n, JpegParsed& out, bool want_segs) {
    int cls = 0;
    const int reason = jpeg_walk(f, n, out, want_segs, cls);
    bbocr_jpeg_plan& pl = out.plan;
    pl.supported = reason == BBOCR_JPEG_OK && !cls;
    if (!cls) return reason;
    if (reason == BBOCR_JPEG_OK) {
        pl.chroma = cls;
    } else {
        pl.restart_interval = pl.mcu_cols = pl.mcu_rows = pl.segments = 0;
        pl.scan_offset = pl.scan_bytes = 0;
    }
    return BBOCR_JPEG_SAMPLING;
}

// ---- progressive files
struct ProgScan {
    HuffSpec tab[3];                                  // per scan component: its DC (Ss = 0) or AC table as it stood at this SOS
    std::vector<std::pair<size_t, size_t>> segs;      // byte ranges of the restart segments in the file (stuffing included)
};
struct ProgParsed {
    bbocr_jpeg_progressive_plan plan;
    JpegParsed frame;                                 // the frame, its quantisation tables and `supported` as jpeg_parse would give them
    std::vector<ProgScan> scans;
};

// component c's own block raster (what a non-interleaved scan walks), and its blocks across / down an MCU
inline void prog_comp_raster(const bbocr_jpeg_plan& fr, int c, int& bw, int& bh, int& ch, int& cv) {
    const int hmax = fr.components == 3 ? fr.sampling[0][0] : 1, vmax = fr.components == 3 ? fr.sampling[0][1] : 1;
    ch = fr.components == 3 ? fr.sampling[c][0] : 1;
    cv = fr.components == 3 ? fr.sampling[c][1] : 1;
    bw = ((fr.width * ch + hmax - 1) / hmax + 7) / 8;
    bh = ((fr.height * cv + vmax - 1) / vmax + 7) / 8;
}
inline int prog_scan_units(const bbocr_jpeg_plan& fr, const bbocr_jpeg_scan& sc) {
    if (sc.components > 1) return fr.mcu_cols * fr.mcu_rows;
    int bw, bh, ch, cv;
    prog_comp_raster(fr, sc.component[0], bw, bh, ch, cv);
    return bw * bh;
}

// jdmarker.c's walk over a whole SOF2 file: headers, then scan after scan (jdphuff.c's checks of the script as T.81 G.1.1 states them),
// up to EOI.  Returns the reason; plan.n_scans scans are described when it returns, refused or not.
inline int prog_walk(const uint8_t* f, size_t n, ProgParsed& out, bool want_segs) {
    bbocr_jpeg_progressive_plan& pl = out.plan;
    bbocr_jpeg_plan& fr = out.frame.plan;
    std::memset(&pl, 0, sizeof pl);
    std::memset(&fr, 0, sizeof fr);
    out.scans.clear();
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return BBOCR_JPEG_NOT_JPEG;
    fr.orientation = exif_orientation(f, n);
    JpegHeader h;
    Segment g;
    signed char bits[3][64];                                          // the Al a coefficient has reached, -1: not sent yet
    std::memset(bits, -1, sizeof bits);
    for (size_t p = 2;; p = g.next) {
        const int seg = next_segment(f, n, p, g);
        if (seg == SEG_EOI) break;
        if (seg != SEG_OK) return seg == SEG_LOST && pl.n_scans ? BBOCR_JPEG_NO_EOI : BBOCR_JPEG_TRUNCATED;
        if (g.m != 0xDA) {
            if (g.m == 0xDB && pl.n_scans) return BBOCR_JPEG_MULTISCAN;     // the IDCT stage dequantises once, behind the last scan
            const int r = take_header(g, 0xC2, 4, h, fr);
            if (r != BBOCR_JPEG_OK) return r;
            continue;
        }
        const uint8_t* s = g.s;
        const size_t sl = g.sl;
        const int nc = fr.components;
        if (pl.n_scans == 0) {                               // the frame, by the rules of the baseline walk
            const int r = check_frame(h, fr, fr.chroma);
            if (r != BBOCR_JPEG_OK) return r;
            for (int i = 0; i < nc; ++i)
                if (!take_quant(h, i, out.frame.quant)) return BBOCR_JPEG_TABLES;
            frame_mcus(fr);
        }
        if (pl.n_scans == BBOCR_JPEG_MAX_SCANS) return BBOCR_JPEG_SCANS;
        bbocr_jpeg_scan sc{};
        ProgScan ps;
        const int ns = sl >= 1 ? s[0] : 0;
        if (ns < 1 || ns > 3 || ns > nc || sl < 1 + 2 * (size_t)ns + 3) return BBOCR_JPEG_MULTISCAN;
        sc.components = ns;
        for (int i = 0; i < ns; ++i) {
            int c = -1;
            for (int k = 0; k < nc; ++k)
                if (h.comp_id[k] == s[1 + 2 * i]) { c = k; break; }
            if (c < 0 || (i > 0 && c <= sc.component[i - 1])) return BBOCR_JPEG_MULTISCAN;
            sc.component[i] = c;
            sc.dc_table[i] = s[2 + 2 * i] >> 4;
            sc.ac_table[i] = s[2 + 2 * i] & 15;
        }
        sc.ss = s[1 + 2 * ns];
        sc.se = s[2 + 2 * ns];
        sc.ah = s[3 + 2 * ns] >> 4;
        sc.al = s[3 + 2 * ns] & 15;
        if (sc.ss == 0 ? sc.se != 0 : (ns != 1 || sc.se < sc.ss || sc.se > 63)) return BBOCR_JPEG_SCRIPT;
        if (sc.ah > 13 || sc.al > 13) return BBOCR_JPEG_SCRIPT;
        for (int i = 0; i < ns; ++i) {
            signed char* b = bits[sc.component[i]];
            if (sc.ss > 0 && b[0] < 0) return BBOCR_JPEG_SCRIPT;                      // AC before the component's first DC scan
            for (int k = sc.ss; k <= sc.se; ++k) {
                if (b[k] < 0 ? sc.ah != 0 : (sc.ah != b[k] || sc.al != sc.ah - 1)) return BBOCR_JPEG_SCRIPT;
                b[k] = (signed char)sc.al;
            }
            if (!(sc.ss == 0 && sc.ah > 0)) {                                          // a DC refinement reads raw bits
                const int id = sc.ss == 0 ? sc.dc_table[i] : sc.ac_table[i];
                JpegHuff probe;
                if (id > 3 || !h.huff[sc.ss == 0 ? 0 : 1][id].have || !derive_table(h.huff[sc.ss == 0 ? 0 : 1][id], probe, sc.ss == 0)) return BBOCR_JPEG_TABLES;
                ps.tab[i] = h.huff[sc.ss == 0 ? 0 : 1][id];
            }
        }
        sc.restart_interval = h.dri;
        sc.offset = (long long)g.next;
        const long long units = prog_scan_units(fr, sc), ri = h.dri ? h.dri : units;
        int nseg = 0;
        size_t end = 0;
        const int r = scan_segments(f, n, g.next, want_segs, ps.segs, nseg, end);
        if (r != BBOCR_JPEG_OK) return r;
        if ((long long)nseg != (units + ri - 1) / ri) return BBOCR_JPEG_RESTART;
        sc.segments = nseg;
        sc.bytes = (long long)end - sc.offset;
        pl.scans[pl.n_scans++] = sc;
        out.scans.push_back(std::move(ps));
        g.next = end;
    }
    if (!pl.n_scans) return BBOCR_JPEG_TRUNCATED;
    for (int c = 0; c < fr.components; ++c)
        for (int k = 0; k < 64; ++k)
            if (bits[c][k] != 0) return BBOCR_JPEG_SCRIPT;                                 // incomplete: libjpeg-turbo would smooth
    return BBOCR_JPEG_OK;
}
// the walk, then the frame as the public plan states it
inline int prog_parse(const uint8_t* f, size_t n, ProgParsed& out, bool want_segs) {
    const int reason = prog_walk(f, n, out, want_segs);
    bbocr_jpeg_progressive_plan& pl = out.plan;
    bbocr_jpeg_plan& fr = out.frame.plan;
    pl.width = fr.width;
    pl.height = fr.height;
    pl.components = fr.components;
    std::memcpy(pl.sampling, fr.sampling, sizeof pl.sampling);
    pl.mcu_cols = fr.mcu_cols;
    pl.mcu_rows = fr.mcu_rows;
    pl.chroma = fr.chroma;
    pl.orientation = fr.orientation;
    pl.reason = reason;
    pl.supported = reason == BBOCR_JPEG_OK;
    fr.supported = pl.supported && !fr.chroma;
    return reason;
}

// tables a scan reads: one per scan component, none in a DC refinement (raw bits)
inline int prog_scan_tables(const bbocr_jpeg_scan& s) { return s.ss == 0 && s.ah > 0 ? 0 : s.components; }
// subsequences of S bits a scan of `segments` restart segments and `bytes` bytes is cut into at most: every segment is cut on its own
inline size_t scan_subs_bound(int segments, long long bytes, int S) { return (size_t)segments + (size_t)bytes * 8 / (size_t)S + 1; }
// ... a progressive scan (0 for a refinement, which is not cut)
inline size_t prog_scan_subs(const bbocr_jpeg_scan& s, int S) { return s.ah > 0 ? 0 : scan_subs_bound(s.segments, s.bytes, S); }

// The restart segments `segs` of a scan of `file` as the device reads them: their bytes without the stuffing, one segment after the
// other, into data (at most the scan's bytes) and seg_byte[segments + 1]; S > 0: every segment cut on its own into subsequences of S
// bits, at least one, into seg_sub[segments + 1] and sub_seg[scan_subs_bound].  Returns the bytes; nsub receives the subsequences.
inline size_t cut_scan(const uint8_t* file, const std::vector<std::pair<size_t, size_t>>& segs, int S, uint8_t* data, int* seg_byte, int* seg_sub,
                       int* sub_seg, int& nsub) {
    const int nseg = (int)segs.size();
    size_t w = 0;
    nsub = 0;
    for (int g = 0; g < nseg; ++g) {
        seg_byte[g] = (int)w;
        w += unstuff(file + segs[g].first, file + segs[g].second, data + w);
        if (S > 0) {
            const int cnt = (int)std::max<size_t>(((w - (size_t)seg_byte[g]) * 8 + S - 1) / S, 1);
            seg_sub[g] = nsub;
            for (int i = 0; i < cnt; ++i) sub_seg[nsub + i] = g;
            nsub += cnt;
        }
    }
    seg_byte[nseg] = (int)w;
    if (S > 0) seg_sub[nseg] = nsub;
    return w;
}

// Scan k of a parsed file as jpegprog.h reads it: cut_scan's tables (a refinement is not cut), the derived tables into
// huff[prog_scan_tables], and every field of `sc` but its pointers, which the caller owns.
inline void prog_fill_scan(const ProgParsed& pp, int k, const uint8_t* file, int S, uint8_t* data, int* seg_byte, JpegHuff* huff, int* seg_sub,
                           int* sub_seg, JpScan& sc) {
    const bbocr_jpeg_plan& fr = pp.frame.plan;
    const bbocr_jpeg_scan& s = pp.plan.scans[k];
    cut_scan(file, pp.scans[k].segs, s.ah == 0 ? S : 0, data, seg_byte, seg_sub, sub_seg, sc.nsub);
    sc.S = S;
    for (int i = 0; i < prog_scan_tables(s); ++i) derive_table(pp.scans[k].tab[i], huff[i]);      // prefix codes: the plan checked
    sc.nseg = s.segments;
    sc.ncs = s.components;
    for (int i = 0; i < 3; ++i) sc.comp[i] = s.component[i];
    sc.Ss = s.ss;
    sc.Se = s.se;
    sc.Ah = s.ah;
    sc.Al = s.al;
    sc.nunits = prog_scan_units(fr, s);
    sc.ri = s.restart_interval ? s.restart_interval : std::max(sc.nunits, 1);
    int bh;
    prog_comp_raster(fr, s.component[0], sc.bw, bh, sc.ch, sc.cv);
    sc.hs = fr.components == 3 ? fr.sampling[0][0] : 1;
    sc.vs = fr.components == 3 ? fr.sampling[0][1] : 1;
    sc.coff = s.component[0] == 0 ? 0 : sc.hs * sc.vs + s.component[0] - 1;
    sc.bpm = fr.components == 3 ? sc.hs * sc.vs + 2 : 1;
    sc.mcux = fr.mcu_cols;
    sc.ncomp = fr.components;
    sc.nblocks = fr.mcu_cols * fr.mcu_rows * sc.bpm;
}

}  // namespace jpeg_host
