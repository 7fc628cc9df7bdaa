// The strip decoders of the device TIFF decoder next to png_inflate.h's Deflate, compiled for host and device alike: PackBits and LZW as
// tiffdec.hip's td_strips runs them, and serial host drivers over the same functions (tools/tiffdec_hostcheck.cpp runs them under a
// sanitizer; tests/tiff_decode_ref.py states what they must produce).  A decoder takes a strip's stored bytes in[0 .. n) and the count the
// strip must produce, need = rows_in_strip * row_bytes, writes out[0 .. need) and returns 0 or TIFFC_ERR_* bits.  Bytes behind the point
// where the count is reached are not read (libtiff does not read them either).  Written once over an execution policy X, as
// png_inflate.h is:
//   X::copy_in(out, o, in, n)             n stored bytes into the output
//   X::fill(out, o, v, n)                 n times the byte v
//   X::copy_back(out, o, src, len, kwkwk, synced)   out[o .. o + len) = out[src .. src + len); src + len <= o, or, with kwkwk, src + len
//                                         == o + 1: the last byte is then the string's first (out[src])
// On the device every lane of the wave runs the same control flow on the same values (the strip is read at uniform addresses) and only
// the copies are shared out among the lanes.  Every loop consumes input or produces output per iteration, or ends on the error it raised.
//
// LZW (TIFF 6.0 section 13 as libtiff and Pillow write it): codes MSB first, 9 bits at the start and after a Clear (256); EOI is 257; the
// first free entry is 258; the width grows one entry EARLY -- a code is read with 9 bits while the next free entry is below 511, 10 below
// 1023, 11 below 2047, else 12 -- so the width is a function of the entry count.  The table is no table of strings: the entry defined
// after code c follows code p is p's string plus c's first byte, and those bytes already stand back to back in the strip's output.  An
// entry is (offset in the strip's output, length) and decoding a code copies `length` earlier bytes forward.  A code equal to the next
// free entry (KwKwK) is the entry being defined: the copy overlaps its destination by one byte, which equals the string's first.
// Stricter than libtiff, so that a stream is either decoded exactly as libtiff decodes it or refused: a strip starts with a Clear.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TIFFC_HD __host__ __device__
#else
#define TIFFC_HD
#endif

// the status word's bits behind png_inflate.h's PNGI_ERR_* (which end at 1024) and pngdec.h's
enum {
    TIFFC_ERR_INPUT = 1 << 13,     // the strip runs out of input before it has produced its count
    TIFFC_ERR_OVERRUN = 1 << 14,   // a run or a string would write beyond the count
    TIFFC_ERR_CODE = 1 << 15,      // an LZW code above the next free entry
    TIFFC_ERR_CLEAR = 1 << 16,     // the first LZW code of a strip is no Clear, or the first code after a Clear is no literal
    TIFFC_ERR_EOI = 1 << 17        // EOI before the count is reached
};

struct TiffcEntry {                // an LZW string: out[off .. off + len)
    uint32_t off, len;
};
constexpr int TIFFC_LZW_ENTRIES = 4096;      // 32 KB: the table of one strip in flight

TIFFC_HD inline int tiffc_lzw_width(uint32_t next_free) { return next_free < 511 ? 9 : (next_free < 1023 ? 10 : (next_free < 2047 ? 11 : 12)); }

template <typename X> TIFFC_HD inline int tiffc_packbits(const uint8_t* in, size_t n, uint8_t* out, size_t need) {
    size_t at = 0, o = 0;
    while (o < need) {
        if (at >= n) return TIFFC_ERR_INPUT;
        const int hdr = (int8_t)in[at++];
        if (hdr == -128) continue;                               // the no-op header
        if (hdr < 0) {
            const size_t run = (size_t)(1 - hdr);
            if (at >= n) return TIFFC_ERR_INPUT;
            if (run > need - o) return TIFFC_ERR_OVERRUN;
            X::fill(out, o, in[at++], run);
            o += run;
        } else {
            const size_t run = (size_t)hdr + 1;
            if (run > n - at) return TIFFC_ERR_INPUT;
            if (run > need - o) return TIFFC_ERR_OVERRUN;
            X::copy_in(out, o, in + at, run);
            at += run;
            o += run;
        }
    }
    return 0;
}

// table[TIFFC_LZW_ENTRIES]: entries 258 and up are used; need < 2^32
template <typename X> TIFFC_HD inline int tiffc_lzw(const uint8_t* in, size_t n, uint8_t* out, size_t need, TiffcEntry* table) {
    uint64_t buf = 0;                                            // codes leave the buffer from its most significant end
    int cnt = 0;
    size_t pos = 0, o = 0, synced = 0;
    uint32_t next_free = 258;
    uint32_t prev_off = 0, prev_len = 0;                         // the string of the code before; prev_len 0: none (behind a Clear)
    bool first = true;
    while (o < need) {
        const int w = tiffc_lzw_width(next_free);
        while (cnt <= 56 && pos < n) {
            buf |= (uint64_t)in[pos++] << (56 - cnt);
            cnt += 8;
        }
        if (cnt < w) return TIFFC_ERR_INPUT;
        const uint32_t code = (uint32_t)(buf >> (64 - w));
        buf <<= w;
        cnt -= w;
        if (first && code != 256) return TIFFC_ERR_CLEAR;
        first = false;
        if (code == 256) {
            next_free = 258;
            prev_len = 0;
            continue;
        }
        if (code == 257) return TIFFC_ERR_EOI;
        if (prev_len == 0) {                                     // behind a Clear: a literal, and no entry yet
            if (code > 255) return TIFFC_ERR_CLEAR;
            X::fill(out, o, (uint8_t)code, 1);
            prev_off = (uint32_t)o;
            prev_len = 1;
            ++o;
            continue;
        }
        if (code > next_free || (code == next_free && next_free >= (uint32_t)TIFFC_LZW_ENTRIES)) return TIFFC_ERR_CODE;
        uint32_t src, len;
        const bool kwkwk = code == next_free;
        if (code < 256) {
            src = 0;
            len = 1;
        } else if (kwkwk) {
            src = prev_off;
            len = prev_len + 1;
        } else {
            const TiffcEntry e = table[code];
            src = e.off;
            len = e.len;
        }
        if (len > need - o) return TIFFC_ERR_OVERRUN;
        if (next_free < (uint32_t)TIFFC_LZW_ENTRIES) {           // the string before plus this one's first byte: they stand back to back
            table[next_free].off = prev_off;
            table[next_free].len = prev_len + 1;
            ++next_free;
        }
        if (code < 256) X::fill(out, o, (uint8_t)code, 1);
        else X::copy_back(out, o, src, len, kwkwk, synced);
        prev_off = (uint32_t)o;
        prev_len = len;
        o += len;
    }
    return 0;
}

// the zlib header of a Deflate strip: png_parse.h's test
TIFFC_HD inline bool tiffc_zlib_header_ok(const uint8_t* z, size_t n) {
    return n >= 2 && (z[0] & 15) == 8 && (z[0] >> 4) <= 7 && !(z[1] & 0x20) && (((uint32_t)z[0] << 8) | z[1]) % 31 == 0;
}

// ---- the serial host drivers
struct TiffcSerial {
    static void copy_in(uint8_t* out, size_t o, const uint8_t* in, size_t n) {
        for (size_t i = 0; i < n; ++i) out[o + i] = in[i];
    }
    static void fill(uint8_t* out, size_t o, uint8_t v, size_t n) {
        for (size_t i = 0; i < n; ++i) out[o + i] = v;
    }
    static void copy_back(uint8_t* out, size_t o, uint32_t src, uint32_t len, bool, size_t&) {
        for (uint32_t i = 0; i < len; ++i) out[o + i] = out[src + i];       // (in order: the KwKwK byte is there when it is read)
    }
};

inline int tiffc_packbits_host(const uint8_t* in, size_t n, uint8_t* out, size_t need) { return tiffc_packbits<TiffcSerial>(in, n, out, need); }

inline int tiffc_lzw_host(const uint8_t* in, size_t n, uint8_t* out, size_t need) {
    static TiffcEntry table[TIFFC_LZW_ENTRIES];                  // (one driver at a time)
    return tiffc_lzw<TiffcSerial>(in, n, out, need, table);
}
