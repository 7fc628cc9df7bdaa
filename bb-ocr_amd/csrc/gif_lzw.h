// GIF's LZW split at its clear codes, compiled for host and device alike as tiff_codecs.h is: the closed form of a code's position, the
// scan that cuts a payload into pieces and the walk of one piece, as gifdec.hip's kernels run them, and serial host drivers over the same
// functions (tools/gifdec_hostcheck.cpp runs them under a sanitizer; tests/gif_decode_ref.py states what they must produce).
//
// The rule (GIF89a appendix F as Pillow's decoder reads it): codes LSB first; clear = 1 << m, the end code clear + 1.  Behind a clear --
// and at the start of the payload, which counts as one -- the width is m + 1 and the next free entry clear + 2.  The first data code
// behind a clear must be below clear and adds no entry; every later one adds an entry while fewer than 4096 exist; the width grows when
// the next free entry reaches 1 << width, up to 12, and with the table full 12-bit codes go on.  So code k (0-based) behind a clear is
// read while the next free entry is clear + 2 + max(0, k - 1): its width is min(12, bit length of clear + 1 + k), a function of k alone,
// and its bit offset the sum of the widths before it -- per width the count of codes read with it (gifl_pos).  A clear or end code sits at
// position k like a data code.  Nothing behind a clear depends on what stands before it but the output position.
//
// A code above the next free entry is damage; one equal to it is the entry being defined (the string before plus its own first byte).  An
// entry is (offset, length) into the PIECE's own output, as in the TIFF LZW: decoding a code copies earlier bytes forward.
//
// Execution policy X, as in tiff_codecs.h:
//   X::first_stop(f, lane, end)        f(l), l = 0 .. 63, is lane l's class of its code (-1 data, else GIFL_END_*): -> the first lane whose
//                                      class is not -1 and that class, or lane = -1
//   X::leader()                        the one that stores what every lane computed alike
//   X::fill(out, o, v, n) / X::copy_back(out, o, src, len, kwkwk, synced)       tiff_codecs.h's
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GIFL_HD __host__ __device__
#else
#define GIFL_HD
#endif

enum {                             // a piece's and a file's status bits
    GIFL_ERR_FIRST = 1,            // the first code behind a clear is no literal
    GIFL_ERR_CODE = 2,             // a code above the next free entry
    GIFL_ERR_SHORT = 4,            // the end code or the end of the payload before the frame is full
    GIFL_ERR_PIECES = 8            // more pieces than the table holds
};
enum { GIFL_END_CLEAR = 0, GIFL_END_EOI = 1, GIFL_END_INPUT = 2 };      // how a piece ends

constexpr int GIFL_STEP = 64;                  // codes per scan step: one per lane
constexpr int GIFL_ENTRIES = 4096;

struct GiflPiece {                 // the codes between two clears
    uint32_t bit_lo, bit_hi;       // the position of its first code
    uint32_t codes;                // data codes: the stop code sits at position `codes`
    uint32_t end;                  // GIFL_END_*
};
struct GiflEntry {                 // a string: out[off .. off + len) of the piece's output
    uint32_t off, len;
};

// the piece table's room for a payload: a piece costs at least one clear code of m + 1 bits; at most max(4096, bytes / 16) all the same
GIFL_HD inline size_t gifl_piece_room(uint64_t payload_bytes, int m) {
    const uint64_t bound = 8 * payload_bytes / (uint64_t)(m + 1) + 1, most = payload_bytes / 16 > 4096 ? payload_bytes / 16 : 4096;
    return (size_t)(bound < most ? bound : most);
}

GIFL_HD inline int gifl_width(int m, uint64_t k) {
    const int w = 64 - __builtin_clzll((1ull << m) + 1 + k);
    return w > 12 ? 12 : w;
}

GIFL_HD inline uint64_t gifl_pos(int m, uint64_t k) {
    const uint64_t c1 = (1ull << m) + 1, top = c1 + k;
    uint64_t bits = 0;
    for (int w = m + 1; w <= 12; ++w) {
        const uint64_t half = 1ull << (w - 1), lo = c1 > half ? c1 : half, hi = (w == 12 || top < 2 * half) ? top : 2 * half;
        if (hi > lo) bits += (hi - lo) * (uint64_t)w;
    }
    return bits;
}

// the code at a bit position of in[0 .. nbits / 8), or -1 when it reaches past the end (nbits is a multiple of 8)
GIFL_HD inline int gifl_read(const uint8_t* in, uint64_t nbits, uint64_t bit, int width) {
    if (bit + (uint64_t)width > nbits) return -1;
    const uint64_t b = bit >> 3, nbytes = nbits >> 3;
    uint32_t v = in[b];
    if (b + 1 < nbytes) v |= (uint32_t)in[b + 1] << 8;
    if (b + 2 < nbytes) v |= (uint32_t)in[b + 2] << 16;
    return (int)((v >> (bit & 7)) & ((1u << width) - 1));
}

// The scan: pieces[0 .. *count) of a payload, 64 codes per step from the last clear.  -> 0 or GIFL_ERR_PIECES (*count = cap then).
// Every step either ends a piece or moves 64 codes on, and a position past the payload ends the last piece.
template <typename X> GIFL_HD inline int gifl_scan(const uint8_t* in, uint64_t nbits, int m, GiflPiece* pieces, uint32_t cap, uint32_t* count) {
    const int clear = 1 << m;
    uint64_t bit = 0, k0 = 0;
    uint32_t n = 0;
    for (;;) {
        int lane = -1, end = 0;
        X::first_stop(
            [&](int l) {
                const uint64_t k = k0 + (uint64_t)l;
                const int c = gifl_read(in, nbits, bit + gifl_pos(m, k), gifl_width(m, k));
                return c < 0 ? (int)GIFL_END_INPUT : (c == clear ? (int)GIFL_END_CLEAR : (c == clear + 1 ? (int)GIFL_END_EOI : -1));
            },
            lane, end);
        if (lane < 0) {
            k0 += GIFL_STEP;
            continue;
        }
        if (n >= cap) {
            *count = n;
            return GIFL_ERR_PIECES;
        }
        const uint64_t k = k0 + (uint64_t)lane;
        if (X::leader()) pieces[n] = GiflPiece{(uint32_t)bit, (uint32_t)(bit >> 32), (uint32_t)k, (uint32_t)end};
        ++n;
        if (end != GIFL_END_CLEAR) {
            *count = n;
            return 0;
        }
        bit += gifl_pos(m, k) + (uint64_t)gifl_width(m, k);
        k0 = 0;
    }
}

// the two tables a piece is walked with: lengths alone (the lengths pass), or (offset, length) (the decode)
struct GiflLengths {
    uint16_t* len;                 // [GIFL_ENTRIES]: a string is at most 4096 bytes long
    GIFL_HD void set(uint32_t i, uint32_t, uint32_t l) const { len[i] = (uint16_t)l; }
    GIFL_HD uint32_t off(uint32_t) const { return 0; }
    GIFL_HD uint32_t length(uint32_t i) const { return len[i]; }
};
struct GiflStrings {
    GiflEntry* e;                  // [GIFL_ENTRIES]
    GIFL_HD void set(uint32_t i, uint32_t o, uint32_t l) const { e[i] = GiflEntry{o, l}; }
    GIFL_HD uint32_t off(uint32_t i) const { return e[i].off; }
    GIFL_HD uint32_t length(uint32_t i) const { return e[i].len; }
};

// One piece: `codes` data codes from first_bit on (the scan has read each: none is a clear or end code, none reaches past the payload),
// at most `room` bytes -- the frame is full there, and the walk ends.  kDecode: the bytes go to out[0 .. room); else only the count is
// kept.  -> 0 or the error met, *produced = the bytes before it.  Entries clear + 2 and up of the table are used.
template <typename X, bool kDecode, typename T>
GIFL_HD inline int gifl_piece(const uint8_t* in, uint64_t nbits, int m, uint64_t first_bit, uint32_t codes, uint8_t* out, uint32_t room, const T& table,
                              uint32_t* produced) {
    const uint32_t clear = 1u << m;
    uint32_t next = clear + 2, o = 0, prev_off = 0, prev_len = 0;       // prev_len 0: no code yet
    uint64_t bit = first_bit;
    size_t synced = 0;
    int err = 0;
    for (uint32_t k = 0; k < codes && o < room; ++k) {
        const int w = gifl_width(m, k);
        const int c = gifl_read(in, nbits, bit, w);
        bit += (uint64_t)w;
        if (c < 0) {                                                    // (not met behind the scan)
            err = GIFL_ERR_SHORT;
            break;
        }
        const uint32_t code = (uint32_t)c;
        uint32_t src = 0, len = 1;
        bool kwkwk = false;
        if (prev_len == 0) {
            if (code >= clear) {
                err = GIFL_ERR_FIRST;
                break;
            }
        } else {
            // (a clear or end code is not met behind the scan; refused all the same: it has no entry)
            if (code > next || (code == next && next >= (uint32_t)GIFL_ENTRIES) || code == clear || code == clear + 1) {
                err = GIFL_ERR_CODE;
                break;
            }
            if (code == next) {
                kwkwk = true;
                src = prev_off;
                len = prev_len + 1;
            } else if (code >= clear) {
                src = table.off(code);
                len = table.length(code);
            }
            if (next < (uint32_t)GIFL_ENTRIES) {                        // the string before plus this one's first byte: they stand back to back
                table.set(next, prev_off, prev_len + 1);
                ++next;
            }
        }
        const uint32_t n = len < room - o ? len : room - o;             // the frame may be full inside this string
        if (kDecode) {
            if (code < clear) X::fill(out, o, (uint8_t)code, 1);
            else X::copy_back(out, o, src, n, kwkwk && n == len, synced);
        }
        prev_off = o;
        prev_len = len;
        o += n;
    }
    *produced = o;
    return err;
}

// ---- the serial host drivers
struct GiflSerial {
    template <typename F> static void first_stop(F&& f, int& lane, int& end) {
        lane = -1;
        for (int l = 0; l < GIFL_STEP; ++l) {
            const int c = f(l);
            if (c >= 0) {
                lane = l;
                end = c;
                return;
            }
        }
    }
    static bool leader() { return true; }
    static void fill(uint8_t* out, size_t o, uint8_t v, size_t n) {
        for (size_t i = 0; i < n; ++i) out[o + i] = v;
    }
    static void copy_back(uint8_t* out, size_t o, uint32_t src, uint32_t len, bool, size_t&) {
        for (uint32_t i = 0; i < len; ++i) out[o + i] = out[src + i];       // (in order: the byte of the entry being defined is there when it is read)
    }
};

inline int gifl_scan_host(const uint8_t* in, size_t bytes, int m, GiflPiece* pieces, uint32_t cap, uint32_t* count) {
    return gifl_scan<GiflSerial>(in, 8 * (uint64_t)bytes, m, pieces, cap, count);
}

inline int gifl_lengths_host(const uint8_t* in, size_t bytes, int m, const GiflPiece& p, uint32_t room, uint32_t* produced) {
    static uint16_t len[GIFL_ENTRIES];                                   // (one driver at a time)
    return gifl_piece<GiflSerial, false>(in, 8 * (uint64_t)bytes, m, ((uint64_t)p.bit_hi << 32) | p.bit_lo, p.codes, nullptr, room, GiflLengths{len}, produced);
}

inline int gifl_decode_host(const uint8_t* in, size_t bytes, int m, const GiflPiece& p, uint8_t* out, uint32_t room, uint32_t* produced) {
    static GiflEntry e[GIFL_ENTRIES];
    return gifl_piece<GiflSerial, true>(in, 8 * (uint64_t)bytes, m, ((uint64_t)p.bit_hi << 32) | p.bit_lo, p.codes, out, room, GiflStrings{e}, produced);
}

// The file's status and its pieces' offsets from the lengths pass: offsets[0 .. count] (the last: the total), saturated at need.  In piece
// order: the frame is full inside or behind a piece -- then what follows does not count --, or the piece ended in an error, the end code
// or the payload's end before that.  (gifdec.hip's gd_offsets computes the same with a wave scan.)
inline int gifl_offsets_host(const GiflPiece* pieces, const uint32_t* lengths, const int* errors, uint32_t count, int scan_error, uint32_t need,
                             uint32_t* offsets) {
    uint64_t cum = 0;
    int status = scan_error;
    bool done = false;
    for (uint32_t i = 0; i < count; ++i) {
        offsets[i] = (uint32_t)(cum < need ? cum : need);
        if (!done && !status) {
            if (cum + lengths[i] >= need) done = true;
            else if (errors[i]) status |= errors[i];
            else if (pieces[i].end != GIFL_END_CLEAR) status |= GIFL_ERR_SHORT;
        }
        cum += lengths[i];
    }
    offsets[count] = (uint32_t)(cum < need ? cum : need);
    if (!done && !status) status |= GIFL_ERR_SHORT;
    return status;
}
