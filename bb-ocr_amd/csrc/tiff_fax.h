// The CCITT strip decoder of the device TIFF decoder next to tiff_codecs.h, compiled for host and device alike: TIFF compression 2 (modified
// Huffman), 3 (T.4, 1-D and 2-D) and 4 (T.6) as tiffdec.hip's td_strips runs it, one wavefront per strip, and a serial host driver over the
// same functions (tools/tiff_fax_hostcheck.cpp runs it under a sanitizer; tests/tiff_fax_ref.py states what it must produce).  The decoder
// takes a strip's stored bytes in[0 .. n), the width and the strip's rows and writes out[0 .. rows * ceil(W / 8)): a white run as 0 bits, a
// black run as 1 bits, MSB first, the bits behind the width 0.  It returns 0 or TIFFC_ERR_* bits.  Bytes behind the last row (RTC, EOFB,
// padding) are not interpreted.  The code tables are T.4's tables 2 and 3 and T.6's mode table, written out here from the Recommendations.
//
// The scheme.  A row is kept as its CHANGING ELEMENTS -- the positions at which the colour changes, the row starting white -- in a line
// buffer of W + 8 uint16; two of them, the row being coded and the reference line, change places per row: the 2-D modes need exactly that
// of the row before (b1 is the first element right of a0 whose index has the parity of the colour being coded; the elements are kept as
// decoded, a zero-length run leaves two equal ones).  The serial chain is one code after the other, so a code is resolved by the wave and
// not by a tree walk: lane l holds words l and 64 + l of each colour's 104 code words (64 terminating, 27 + 13 make-up), every lane compares
// the 16 bits at the head of the stream with its words, and because the words of a colour are prefix-free ONE ballot names the lane that
// matched; length and run come over with a readlane.  The mode codes of T.6 are seven bits at most and are told apart by their leading
// zeros.  A finished row is rendered by all lanes: each element toggles its bit in a bitmap of the row (an LDS atomic XOR), a prefix XOR
// -- shifts inside a word, one ballot across the 64 words of a step -- turns the toggles into pixels, and each lane stores its word's bytes.
// On the device every lane runs the same control flow on the same values: what is read from the strip or from a line buffer goes through
// X::uniform (a readfirstlane).  LDS per workgroup: fax_lds_bytes(W) = 2 * 2 (W + 8) + 4 ceil(W / 32) bytes, 42,272 at the width limit.
//
// Every loop consumes input or produces output per iteration, or ends on the error it raised; the one loop that does neither, the search
// for b1, steps forward through the reference line, which the row before produced, and a vertical mode to the left steps it back by one.
// Strict where libtiff patches a bad line and carries on: a stream is decoded exactly or refused (the cases: bbocr.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "tiff_codecs.h"

// the status word's bits behind tiff_codecs.h's (which end at 1 << 17)
enum {
    TIFFC_ERR_FAX_CODE = 1 << 18,    // a bit pattern that is no code word of the colour, or no mode
    TIFFC_ERR_FAX_EXT = 1 << 19,     // an extension code (uncompressed mode)
    TIFFC_ERR_FAX_WIDTH = 1 << 20,   // runs beyond the width, or more changing elements than a line of that width holds
    TIFFC_ERR_FAX_MODE = 1 << 21,    // a vertical mode that does not move a0 forwards or moves it past the width; a pass mode whose b2 is the line's end
    TIFFC_ERR_FAX_EOL = 1 << 22      // T.4: fewer than eleven 0 bits before the 1 that ends an EOL
};

struct FaxWord {                     // a code word, right-aligned
    uint16_t code, len;
};
constexpr int FAX_WORDS = 104;       // per colour: index i < 64 the terminating code of run i, index 63 + k the make-up code of 64 k
constexpr int FAX_LINE_SLACK = 8;    // a line buffer holds W + 8 elements: at most W + 4 as decoded, three times W behind them

TIFFC_HD inline FaxWord fax_word(int colour, int i) {
    static constexpr FaxWord words[2][FAX_WORDS] = {{
        {0x35,8}, {0x7,6}, {0x7,4}, {0x8,4}, {0xB,4}, {0xC,4}, {0xE,4}, {0xF,4}, {0x13,5}, {0x14,5}, {0x7,5}, {0x8,5}, {0x8,6},
        {0x3,6}, {0x34,6}, {0x35,6}, {0x2A,6}, {0x2B,6}, {0x27,7}, {0xC,7}, {0x8,7}, {0x17,7}, {0x3,7}, {0x4,7}, {0x28,7}, {0x2B,7},
        {0x13,7}, {0x24,7}, {0x18,7}, {0x2,8}, {0x3,8}, {0x1A,8}, {0x1B,8}, {0x12,8}, {0x13,8}, {0x14,8}, {0x15,8}, {0x16,8}, {0x17,8},
        {0x28,8}, {0x29,8}, {0x2A,8}, {0x2B,8}, {0x2C,8}, {0x2D,8}, {0x4,8}, {0x5,8}, {0xA,8}, {0xB,8}, {0x52,8}, {0x53,8}, {0x54,8},
        {0x55,8}, {0x24,8}, {0x25,8}, {0x58,8}, {0x59,8}, {0x5A,8}, {0x5B,8}, {0x4A,8}, {0x4B,8}, {0x32,8}, {0x33,8}, {0x34,8}, {0x1B,5},
        {0x12,5}, {0x17,6}, {0x37,7}, {0x36,8}, {0x37,8}, {0x64,8}, {0x65,8}, {0x68,8}, {0x67,8}, {0xCC,9}, {0xCD,9}, {0xD2,9}, {0xD3,9},
        {0xD4,9}, {0xD5,9}, {0xD6,9}, {0xD7,9}, {0xD8,9}, {0xD9,9}, {0xDA,9}, {0xDB,9}, {0x98,9}, {0x99,9}, {0x9A,9}, {0x18,6}, {0x9B,9},
        {0x8,11}, {0xC,11}, {0xD,11}, {0x12,12}, {0x13,12}, {0x14,12}, {0x15,12}, {0x16,12}, {0x17,12}, {0x1C,12}, {0x1D,12}, {0x1E,12}, {0x1F,12},
    }, {
        {0x37,10}, {0x2,3}, {0x3,2}, {0x2,2}, {0x3,3}, {0x3,4}, {0x2,4}, {0x3,5}, {0x5,6}, {0x4,6}, {0x4,7}, {0x5,7}, {0x7,7},
        {0x4,8}, {0x7,8}, {0x18,9}, {0x17,10}, {0x18,10}, {0x8,10}, {0x67,11}, {0x68,11}, {0x6C,11}, {0x37,11}, {0x28,11}, {0x17,11}, {0x18,11},
        {0xCA,12}, {0xCB,12}, {0xCC,12}, {0xCD,12}, {0x68,12}, {0x69,12}, {0x6A,12}, {0x6B,12}, {0xD2,12}, {0xD3,12}, {0xD4,12}, {0xD5,12}, {0xD6,12},
        {0xD7,12}, {0x6C,12}, {0x6D,12}, {0xDA,12}, {0xDB,12}, {0x54,12}, {0x55,12}, {0x56,12}, {0x57,12}, {0x64,12}, {0x65,12}, {0x52,12}, {0x53,12},
        {0x24,12}, {0x37,12}, {0x38,12}, {0x27,12}, {0x28,12}, {0x58,12}, {0x59,12}, {0x2B,12}, {0x2C,12}, {0x5A,12}, {0x66,12}, {0x67,12}, {0xF,10},
        {0xC8,12}, {0xC9,12}, {0x5B,12}, {0x33,12}, {0x34,12}, {0x35,12}, {0x6C,13}, {0x6D,13}, {0x4A,13}, {0x4B,13}, {0x4C,13}, {0x4D,13}, {0x72,13},
        {0x73,13}, {0x74,13}, {0x75,13}, {0x76,13}, {0x77,13}, {0x52,13}, {0x53,13}, {0x54,13}, {0x55,13}, {0x5A,13}, {0x5B,13}, {0x64,13}, {0x65,13},
        {0x8,11}, {0xC,11}, {0xD,11}, {0x12,12}, {0x13,12}, {0x14,12}, {0x15,12}, {0x16,12}, {0x17,12}, {0x1C,12}, {0x1D,12}, {0x1E,12}, {0x1F,12},
    }};
    return words[colour][i];
}

TIFFC_HD inline int fax_word_run(int i) { return i < 64 ? i : 64 * (i - 63); }

// the scratch of one strip in flight: two line buffers and the row's bitmap, in this order (on the device: the workgroup's LDS)
TIFFC_HD inline size_t fax_line_bytes(int W) { return (2 * ((size_t)W + FAX_LINE_SLACK) + 3) & ~(size_t)3; }
TIFFC_HD inline size_t fax_lds_bytes(int W) { return 2 * fax_line_bytes(W) + 4 * (((size_t)W + 31) / 32); }

TIFFC_HD inline uint32_t fax_rev8(uint32_t b) {            // the bits of every byte of b reversed, the bytes in place
    b = ((b & 0xF0F0F0F0u) >> 4) | ((b & 0x0F0F0F0Fu) << 4);
    b = ((b & 0xCCCCCCCCu) >> 2) | ((b & 0x33333333u) << 2);
    return ((b & 0xAAAAAAAAu) >> 1) | ((b & 0x55555555u) << 1);
}

// the strip as a stream of bits, MSB first; with fill order 2 the bits of every stored byte are reversed on read
struct FaxBits {
    const uint8_t* in;
    size_t n, pos;
    uint64_t buf, used;              // bits leave the buffer from its most significant end; used: the bits taken so far
    int cnt;
    bool rev;
    template <typename X> TIFFC_HD void fill() {
        if (cnt <= 32 && n - pos >= 4) {                         // four bytes at once: their loads are in flight together
            uint32_t w = X::uniform((uint32_t)in[pos] << 24 | (uint32_t)in[pos + 1] << 16 | (uint32_t)in[pos + 2] << 8 | (uint32_t)in[pos + 3]);
            if (rev) w = fax_rev8(w);
            buf |= (uint64_t)w << (32 - cnt);
            cnt += 32;
            pos += 4;
            return;
        }
        while (cnt <= 56 && pos < n) {
            uint32_t b = X::uniform(in[pos++]);
            if (rev) b = fax_rev8(b);
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    TIFFC_HD uint32_t head16() const { return (uint32_t)(buf >> 48); }
    TIFFC_HD void take(int k) {      // k <= cnt
        buf = k < 64 ? buf << k : 0;
        cnt -= k;
        used += (uint64_t)k;
    }
};

// one run of the colour: any number of make-up codes and one terminating code
template <typename X> TIFFC_HD inline int fax_run(FaxBits& b, const typename X::Words& words, int colour, int W, int& run) {
    run = 0;
    for (;;) {
        b.template fill<X>();
        int len = 0, r = 0;
        if (!X::resolve(words, colour, b.head16(), len, r)) return b.cnt < 13 ? (int)TIFFC_ERR_INPUT : (int)((b.head16() >> 7) == 1 ? TIFFC_ERR_FAX_EXT : TIFFC_ERR_FAX_CODE);
        if (len > b.cnt) return TIFFC_ERR_INPUT;
        b.take(len);
        run += r;
        if (run > W) return TIFFC_ERR_FAX_WIDTH;
        if (r < 64) return 0;
    }
}

// a 1-D row: runs, white first, until they reach the width -> its n changing elements in cur
template <typename X> TIFFC_HD inline int fax_row_1d(FaxBits& b, const typename X::Words& words, uint16_t* cur, int W, int& n) {
    int x = 0, colour = 0;
    n = 0;
    while (x < W) {
        int run;
        const int err = fax_run<X>(b, words, colour, W, run);
        if (err) return err;
        x += run;
        if (x > W || n >= W + 4) return TIFFC_ERR_FAX_WIDTH;
        X::put(cur, n++, x);
        colour ^= 1;
    }
    return 0;
}

// a 2-D row against the reference line ref (its elements, then W three times) -> its n changing elements in cur
template <typename X> TIFFC_HD inline int fax_row_2d(FaxBits& b, const typename X::Words& words, const uint16_t* ref, uint16_t* cur, int W, int& n) {
    int a0 = -1, colour = 0, pb = 0;
    n = 0;
    while (a0 < W) {
        int b1 = X::get(ref, pb);
        while (b1 <= a0 && b1 < W) {                         // (forwards through the reference line)
            pb += 2;
            b1 = X::get(ref, pb);
        }
        b.template fill<X>();
        const uint32_t h = b.head16() >> 9;                  // seven bits: the longest mode code
        int len, d = 0;
        enum { PASS, HORIZONTAL, VERTICAL } mode = VERTICAL;
        if (h & 0x40) len = 1;
        else if (h & 0x20) len = 3, d = (h & 0x10) ? 1 : -1;
        else if (h & 0x10) len = 3, mode = HORIZONTAL;
        else if (h & 0x08) len = 4, mode = PASS;
        else if (h & 0x04) len = 6, d = (h & 0x02) ? 2 : -2;
        else if (h & 0x02) len = 7, d = (h & 0x01) ? 3 : -3;
        else return b.cnt < 7 ? (int)TIFFC_ERR_INPUT : (int)(h ? TIFFC_ERR_FAX_EXT : TIFFC_ERR_FAX_CODE);
        if (len > b.cnt) return TIFFC_ERR_INPUT;
        b.take(len);
        if (n + 2 > W + 4) return TIFFC_ERR_FAX_WIDTH;
        if (mode == PASS) {
            const int b2 = X::get(ref, pb + 1);
            if (b2 >= W) return TIFFC_ERR_FAX_MODE;
            a0 = b2;
            pb += 2;
        } else if (mode == HORIZONTAL) {
            int r1, r2, err;
            if ((err = fax_run<X>(b, words, colour, W, r1)) || (err = fax_run<X>(b, words, colour ^ 1, W, r2))) return err;
            const int a1 = (a0 < 0 ? 0 : a0) + r1, a2 = a1 + r2;
            if (a2 > W) return TIFFC_ERR_FAX_WIDTH;
            X::put(cur, n++, a1);
            X::put(cur, n++, a2);
            a0 = a2;
        } else {
            const int a1 = b1 + d;
            if (a1 <= a0 || a1 > W) return TIFFC_ERR_FAX_MODE;
            X::put(cur, n++, a1);
            a0 = a1;
            colour ^= 1;
            pb = d < 0 && pb > 0 ? pb - 1 : pb + 1;
        }
    }
    return 0;
}

// T.4: any number of 0 bits, at least eleven, and a 1
template <typename X> TIFFC_HD inline int fax_eol(FaxBits& b) {
    int zeros = 0;
    for (;;) {
        b.template fill<X>();
        if (b.cnt == 0) return TIFFC_ERR_INPUT;
        const uint32_t w = (uint32_t)(b.buf >> 32);
        int z = w ? __builtin_clz(w) : 32;
        const bool one = z < 32 && z < b.cnt;
        if (!one && z > b.cnt) z = b.cnt;
        b.take(one ? z + 1 : z);
        zeros = zeros + z > 4096 ? 4096 : zeros + z;
        if (one) return zeros < 11 ? TIFFC_ERR_FAX_EOL : 0;
    }
}

// scheme: 2, 3 or 4 (the TIFF compression); t4_options: bit 0 the 2-D coding of scheme 3 (bit 2, aligned EOLs, changes nothing here: the
// fill is zeros before an EOL); line0 / line1 / bitmap: the scratch (fax_line_bytes / fax_lds_bytes); W <= BBOCR_FAX_MAX_WIDTH
template <typename X> TIFFC_HD inline int fax_decode_strip(const uint8_t* in, size_t n, uint8_t* out, int W, int rows, int scheme, int t4_options, int fill_order,
                                                            uint16_t* line0, uint16_t* line1, uint32_t* bitmap) {
    typename X::Words words;
    X::load(words);
    FaxBits b{in, n, 0, 0, 0, 0, fill_order == 2};
    const size_t row_bytes = ((size_t)W + 7) / 8;
    uint16_t *cur = line0, *ref = line1;
    for (int k = 0; k < 3; ++k) X::put(ref, k, W);           // the reference line of a strip's first row is white
    for (int y = 0; y < rows; ++y) {
        bool one_d = scheme != 4;
        int err = 0, count = 0;
        if (scheme == 2) {
            const int skip = (int)((0 - b.used) & 7);            // rows start on a byte boundary
            b.template fill<X>();
            b.take(skip < b.cnt ? skip : b.cnt);
        } else if (scheme == 3) {
            if ((err = fax_eol<X>(b))) return err;
            if (t4_options & 1) {
                b.template fill<X>();
                if (b.cnt < 1) return TIFFC_ERR_INPUT;
                one_d = (b.head16() >> 15) != 0;
                b.take(1);
            }
        }
        X::sync();                                           // (the reference line's elements are in place)
        err = one_d ? fax_row_1d<X>(b, words, cur, W, count) : fax_row_2d<X>(b, words, ref, cur, W, count);
        if (err) return err;
        for (int k = 0; k < 3; ++k) X::put(cur, count + k, W);
        X::sync();
        X::render(cur, count, W, bitmap, out + (size_t)y * row_bytes, row_bytes);
        uint16_t* t = cur;
        cur = ref;
        ref = t;
    }
    return 0;
}

// ---- the serial host driver
struct FaxSerial {
    struct Words {};
    static void load(Words&) {}
    static uint32_t uniform(uint32_t v) { return v; }
    static void sync() {}
    static bool resolve(const Words&, int colour, uint32_t head16, int& len, int& run) {
        for (int i = 0; i < FAX_WORDS; ++i) {
            const FaxWord w = fax_word(colour, i);
            if ((head16 >> (16 - w.len)) == w.code) {
                len = w.len;
                run = fax_word_run(i);
                return true;
            }
        }
        return false;
    }
    static void put(uint16_t* line, int i, int v) { line[i] = (uint16_t)v; }
    static int get(const uint16_t* line, int i) { return line[i]; }
    static void render(const uint16_t* cur, int n, int W, uint32_t*, uint8_t* out, size_t row_bytes) {
        for (size_t i = 0; i < row_bytes; ++i) out[i] = 0;
        for (int k = 0; k < n; k += 2) {                     // black from an element of even index to the next one
            const int to = k + 1 < n ? cur[k + 1] : W;
            for (int x = cur[k]; x < to; ++x) out[x >> 3] |= (uint8_t)(0x80u >> (x & 7));
        }
    }
};

inline int fax_decode_strip_host(const uint8_t* in, size_t n, uint8_t* out, int W, int rows, int scheme, int t4_options, int fill_order) {
    std::vector<uint16_t> line0((size_t)W + FAX_LINE_SLACK), line1((size_t)W + FAX_LINE_SLACK);      // exact sizes: a sanitizer sees one element too far
    return fax_decode_strip<FaxSerial>(in, n, out, W, rows, scheme, t4_options, fill_order, line0.data(), line1.data(), nullptr);
}
