// Inflate (RFC 1951) as the device PNG decoder runs it, compiled for host and device alike: the bit reader, the canonical table builder
// and the symbol step of pngdec.hip's pd_inflate, and a serial host driver over the same functions (tools/pngdec_hostcheck.cpp runs it
// under a sanitizer; tests/png_decode_ref.py states what it must produce).  The functions are written once over an execution policy X:
//   X::leader()            this caller writes the shared tables and the single output bytes (host: always; device: lane 0 of the wave)
//   X::barrier()           what the leader wrote is visible to every caller (host: nothing; device: the workgroup barrier)
//   X::put / copy_in / copy_match   one byte, a stored block's bytes, a match's bytes into the output
// On the device every lane of the wave runs the same control flow on the same values (the stream is read at uniform addresses), so the
// state lives in registers and only the copies are shared out among the lanes.  Every loop consumes at least one input bit or produces at
// least one output byte per iteration, or ends on the error it raised: a damaged stream terminates.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGI_HD __host__ __device__
#else
#define PNGI_HD
#endif

// what a damaged stream raises (pd_inflate ORs the bits into the file's status word; pngdec.hip adds its own behind them)
enum {
    PNGI_ERR_INPUT = 1,          // the input runs out
    PNGI_ERR_BTYPE = 2,          // block type 3
    PNGI_ERR_STORED = 4,         // stored LEN != ~NLEN
    PNGI_ERR_OVERSUBSCRIBED = 8, // a code with more patterns than its lengths allow
    PNGI_ERR_INCOMPLETE = 16,    // an incomplete code (zlib's one exception: a literal/length or distance code of a single 1-bit pattern)
    PNGI_ERR_DISTANCE = 32,      // a distance beyond the bytes produced
    PNGI_ERR_OVERRUN = 64,       // output beyond the bound
    PNGI_ERR_SHORT = 128,        // the end of the stream before the bound
    PNGI_ERR_ADLER = 256,        // an Adler-32 that differs from the trailer
    PNGI_ERR_SYMBOL = 512,       // a bit pattern without a code; literal/length symbol 286 / 287, distance symbol 30 / 31; a header that names
                                 // more than 286 / 30 codes, repeats nothing, repeats past the last length or has no end-of-block code
    PNGI_ERR_ZLIB = 1024         // the host driver only: the zlib header (the device decoder's plan refuses such a file)
};

constexpr int PNGI_LFAST = 10, PNGI_DFAST = 8;      // bits the fast tables resolve in one lookup; longer codes walk the canonical counts
constexpr int PNGI_MAXL = 288, PNGI_MAXD = 32;

struct PngiCode {                 // a canonical code: symbols per length, the symbols ordered by (length, symbol)
    uint16_t* count;              // [16]
    uint16_t* sym;
    uint16_t* fast;               // [1 << fast_bits]: (symbol << 4) | length for every pattern of a code of at most fast_bits bits, else 0
    int fast_bits;
};

struct PngiTables {               // the decoder's tables: the device keeps them in LDS
    uint16_t lcount[16], dcount[16];
    uint16_t lsym[PNGI_MAXL], dsym[PNGI_MAXD];
    uint16_t lfast[1 << PNGI_LFAST], dfast[1 << PNGI_DFAST];
    uint16_t csym[19], cfast[1 << 7], ccount[16];
    uint16_t offs[16];
    uint8_t lens[PNGI_MAXL + PNGI_MAXD + 8];
};

struct PngiBits {                 // the bit reader: bits leave the buffer from its least significant end
    const uint8_t* in;
    size_t n, pos;                // pos: the next byte to load
    uint64_t buf;
    int cnt;
    int err;
};

template <typename X> PNGI_HD inline void pngi_refill(PngiBits& b) {
    while (b.cnt <= 56 && b.pos < b.n) {
        b.buf |= (uint64_t)b.in[b.pos++] << b.cnt;
        b.cnt += 8;
    }
}
// k <= 16 bits; past the end of the input: the error, and zeros
template <typename X> PNGI_HD inline uint32_t pngi_take(PngiBits& b, int k) {
    if (b.cnt < k) pngi_refill<X>(b);
    if (b.cnt < k) {
        b.err |= PNGI_ERR_INPUT;
        b.buf = 0;
        b.cnt = 0;
        return 0;
    }
    const uint32_t v = (uint32_t)(b.buf & ((1u << k) - 1));
    b.buf >>= k;
    b.cnt -= k;
    return v;
}
// the reader at the next whole byte of the input, nothing buffered: -> that byte's position
PNGI_HD inline size_t pngi_byte_align(PngiBits& b) {
    b.pos -= (size_t)(b.cnt >> 3);
    b.buf = 0;
    b.cnt = 0;
    return b.pos;
}

PNGI_HD inline uint32_t pngi_rev(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// The canonical code of lens[0 .. n): c.count, c.sym and c.fast written by the leader.  -> 0, or the error.  `strict`: the code-length
// code, for which zlib allows no incomplete set; the others may be incomplete when their longest code has one bit.
template <typename X> PNGI_HD inline int pngi_build(const uint8_t* lens, int n, PngiCode& c, uint16_t* offs, bool strict) {
    int count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s]];
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return PNGI_ERR_OVERSUBSCRIBED;
        if (count[l]) max = l;
    }
    if (left > 0 && max != 0 && (strict || max != 1)) return PNGI_ERR_INCOMPLETE;
    if (X::leader()) {
        for (int l = 0; l < 16; ++l) c.count[l] = (uint16_t)(l ? count[l] : 0);
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        for (int i = 0; i < (1 << c.fast_bits); ++i) c.fast[i] = 0;
        int next[16];
        int code = 0;
        next[0] = 0;
        for (int l = 1; l < 16; ++l) {
            code = (code + (l > 1 ? count[l - 1] : 0)) << 1;
            next[l] = code;
        }
        for (int s = 0; s < n; ++s) {
            const int l = lens[s];
            if (!l) continue;
            c.sym[offs[l]++] = (uint16_t)s;
            const int cd = next[l]++;
            if (l <= c.fast_bits)
                for (uint32_t p = pngi_rev((uint32_t)cd, l); p < (1u << c.fast_bits); p += 1u << l) c.fast[p] = (uint16_t)((s << 4) | l);
        }
    }
    X::barrier();
    return 0;
}

// one symbol of the code; -1 with the error raised for a pattern without a code or an input that ran out
template <typename X> PNGI_HD inline int pngi_symbol(PngiBits& b, const PngiCode& c) {
    if (b.cnt < 15) pngi_refill<X>(b);
    const uint32_t e = c.fast[b.buf & ((1u << c.fast_bits) - 1)];
    if (e) {
        const int l = (int)(e & 15);
        if (l > b.cnt) {
            b.err |= PNGI_ERR_INPUT;
            return -1;
        }
        b.buf >>= l;
        b.cnt -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    uint64_t bits = b.buf;
    for (int l = 1; l < 16; ++l) {
        if (l > b.cnt) {
            b.err |= PNGI_ERR_INPUT;
            return -1;
        }
        code |= (int)(bits & 1);
        bits >>= 1;
        const int cn = c.count[l];
        if (code - cn < first) {
            b.buf >>= l;
            b.cnt -= l;
            return c.sym[index + (code - first)];
        }
        index += cn;
        first = (first + cn) << 1;
        code <<= 1;
    }
    b.err |= PNGI_ERR_SYMBOL;
    return -1;
}

PNGI_HD inline int pngi_len_base(int s) {      // s = symbol - 257
    return s < 8 ? 3 + s : (s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1)));
}
PNGI_HD inline int pngi_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
PNGI_HD inline int pngi_dist_base(int s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1)); }
PNGI_HD inline int pngi_dist_extra(int s) { return s < 4 ? 0 : (s >> 1) - 1; }

// A dynamic block's header -> the two codes.  The HLIT + HDIST lengths are ONE sequence: a repeat may run from the literal/length
// lengths into the distance lengths.
template <typename X> PNGI_HD inline void pngi_dynamic_header(PngiBits& b, PngiTables& T, PngiCode& lc, PngiCode& dc) {
    const int nlen = (int)pngi_take<X>(b, 5) + 257, ndist = (int)pngi_take<X>(b, 5) + 1, ncode = (int)pngi_take<X>(b, 4) + 4;
    if (b.err) return;
    if (nlen > 286 || ndist > 30) {
        b.err |= PNGI_ERR_SYMBOL;
        return;
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) cl[order[i]] = (uint8_t)pngi_take<X>(b, 3);
    if (b.err) return;
    PngiCode cc{T.ccount, T.csym, T.cfast, 7};
    X::barrier();                                   // nobody still reads the tables of the block before
    int e = pngi_build<X>(cl, 19, cc, T.offs, true);
    if (e) {
        b.err |= e;
        return;
    }
    int at = 0, prev = 0;
    while (at < nlen + ndist) {                     // every iteration takes a symbol of at least one bit
        const int s = pngi_symbol<X>(b, cc);
        if (s < 0) return;
        int rep = 1, v = s;
        if (s == 16) {
            if (at == 0) {
                b.err |= PNGI_ERR_SYMBOL;
                return;
            }
            v = prev;
            rep = 3 + (int)pngi_take<X>(b, 2);
        } else if (s == 17) {
            v = 0;
            rep = 3 + (int)pngi_take<X>(b, 3);
        } else if (s == 18) {
            v = 0;
            rep = 11 + (int)pngi_take<X>(b, 7);
        }
        if (b.err) return;
        if (at + rep > nlen + ndist) {
            b.err |= PNGI_ERR_SYMBOL;
            return;
        }
        if (X::leader())
            for (int i = 0; i < rep; ++i) T.lens[at + i] = (uint8_t)v;
        at += rep;
        prev = v;
    }
    X::barrier();
    if (T.lens[256] == 0) {
        b.err |= PNGI_ERR_SYMBOL;                   // no end-of-block code
        return;
    }
    e = pngi_build<X>(T.lens, nlen, lc, T.offs, false);
    if (!e) e = pngi_build<X>(T.lens + nlen, ndist, dc, T.offs, false);
    b.err |= e;
}

template <typename X> PNGI_HD inline void pngi_fixed_tables(PngiBits& b, PngiTables& T, PngiCode& lc, PngiCode& dc) {
    X::barrier();
    if (X::leader()) {
        for (int s = 0; s < 288; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));
        for (int s = 0; s < 32; ++s) T.lens[288 + s] = 5;
    }
    X::barrier();
    int e = pngi_build<X>(T.lens, 288, lc, T.offs, false);
    if (!e) e = pngi_build<X>(T.lens + 288, 32, dc, T.offs, false);
    b.err |= e;
}

// A raw deflate stream in[0 .. n) -> out[0 .. cap): -> the error bits (0: every block decoded and the last one was final), *produced = the
// bytes written (never more than cap), *end = the input position behind the last block, at a whole byte.  The caller compares *produced
// with the size it expects and reads the trailer at *end.
template <typename X> PNGI_HD inline int pngi_inflate(const uint8_t* in, size_t n, uint8_t* out, size_t cap, PngiTables& T, size_t* produced,
                                                       size_t* end) {
    PngiBits b{in, n, 0, 0, 0, 0};
    size_t synced = 0;                            // out[0 .. synced) is known to be readable by every caller (the device's copy_match)
    PngiCode lc{T.lcount, T.lsym, T.lfast, PNGI_LFAST}, dc{T.dcount, T.dsym, T.dfast, PNGI_DFAST};
    size_t o = 0;
    int last = 0;
    while (!last && !b.err) {
        last = (int)pngi_take<X>(b, 1);
        const int type = (int)pngi_take<X>(b, 2);
        if (b.err) break;
        if (type == 3) {
            b.err |= PNGI_ERR_BTYPE;
            break;
        }
        if (type == 0) {
            b.buf >>= b.cnt & 7;
            b.cnt -= b.cnt & 7;
            const uint32_t len = pngi_take<X>(b, 16), nlen = pngi_take<X>(b, 16);
            if (b.err) break;
            if (len != (nlen ^ 0xFFFFu)) {
                b.err |= PNGI_ERR_STORED;
                break;
            }
            const size_t at = pngi_byte_align(b);
            if (len > n - at) {
                b.err |= PNGI_ERR_INPUT;
                break;
            }
            if (len > cap - o) {
                b.err |= PNGI_ERR_OVERRUN;
                break;
            }
            X::copy_in(out, o, in + at, len);
            o += len;
            b.pos = at + len;
            continue;
        }
        if (type == 1) pngi_fixed_tables<X>(b, T, lc, dc);
        else pngi_dynamic_header<X>(b, T, lc, dc);
        while (!b.err) {                          // a symbol of at least one bit per iteration
            const int s = pngi_symbol<X>(b, lc);
            if (s < 0) break;
            if (s < 256) {
                if (o >= cap) {
                    b.err |= PNGI_ERR_OVERRUN;
                    break;
                }
                X::put(out, o, (uint8_t)s);
                ++o;
                continue;
            }
            if (s == 256) break;
            if (s > 285) {
                b.err |= PNGI_ERR_SYMBOL;
                break;
            }
            const int ls = s - 257;
            const int len = pngi_len_base(ls) + (int)pngi_take<X>(b, pngi_len_extra(ls));
            const int ds = pngi_symbol<X>(b, dc);
            if (ds < 0) break;
            if (ds > 29) {
                b.err |= PNGI_ERR_SYMBOL;
                break;
            }
            const int de = pngi_dist_extra(ds);
            uint32_t dist = (uint32_t)pngi_dist_base(ds);
            if (de > 0) {                         // up to 13 bits
                dist += pngi_take<X>(b, de);
            }
            if (b.err) break;
            if (dist > o) {
                b.err |= PNGI_ERR_DISTANCE;
                break;
            }
            if ((size_t)len > cap - o) {
                b.err |= PNGI_ERR_OVERRUN;
                break;
            }
            X::copy_match(out, o, dist, len, synced);
            o += (size_t)len;
        }
    }
    *produced = o;
    *end = pngi_byte_align(b);
    return b.err;
}

PNGI_HD inline uint32_t pngi_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// ---- the serial host driver
struct PngiSerial {
    static bool leader() { return true; }
    static void barrier() {}
    static void put(uint8_t* out, size_t o, uint8_t v) { out[o] = v; }
    static void copy_in(uint8_t* out, size_t o, const uint8_t* in, size_t n) {
        for (size_t i = 0; i < n; ++i) out[o + i] = in[i];
    }
    static void copy_match(uint8_t* out, size_t o, uint32_t dist, int len, size_t&) {
        for (int i = 0; i < len; ++i) out[o + i] = out[o + i - dist];
    }
};

inline uint32_t pngi_adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) {
        a = (a + p[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return (b << 16) | a;
}

// A zlib stream z[0 .. n) that must inflate to exactly `expect` bytes -> out[0 .. expect): the error bits, *produced = the bytes written.
// Bytes behind the trailer are ignored, as libpng and Pillow ignore them.
inline int pngi_inflate_zlib(const uint8_t* z, size_t n, uint8_t* out, size_t expect, size_t* produced) {
    *produced = 0;
    if (n < 2) return PNGI_ERR_ZLIB;
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || (z[1] & 0x20) || ((z[0] << 8) | z[1]) % 31) return PNGI_ERR_ZLIB;
    static PngiTables T;                          // (one driver at a time)
    size_t end = 0;
    int err = pngi_inflate<PngiSerial>(z + 2, n - 2, out, expect, T, produced, &end);
    if (err) return err;
    if (*produced != expect) return PNGI_ERR_SHORT;
    if (n - 2 - end < 4) return PNGI_ERR_INPUT;
    if (pngi_be32(z + 2 + end) != pngi_adler32(out, expect)) return PNGI_ERR_ADLER;
    return 0;
}
