// Progressive JPEG (SOF2), the entropy side of one scan into the coefficient buffer of jpegdec.hip (int16 [blocks][64], natural order,
// blocks in MCU order): T.81 G.1.2 as libjpeg-turbo's jdphuff.c carries it out (decode_mcu_DC_first, _AC_first, _DC_refine, _AC_refine),
// stated by tests/jpeg_progressive_ref.py.  What decodes is here and compiles for the device and for the host: jp_run_first (a first scan
// from any state, the unit of the speculative passes -- jpeg_spec.h's, with its state, subsequence lookup and zig-zag table), jp_dc_refine_unit, jp_refine_walk (an AC refinement's symbol by mask
// arithmetic).  jp_decode_segment strings them together in the host's order, one restart segment after the other
// (tools/jpegprog_hostcheck.cpp: the same routines under the sanitisers); jpegprog.hip runs them in the device's.
// The bytes are untrusted: every stream read is clamped to the segment (past its end: 1-bits), every coefficient access is
// index-checked, every loop's trip count is fixed by the plan (units of the segment, the band Ss .. Se, S + 32 symbols a subsequence).
#pragma once
#include "jpeg_spec.h"

// The descriptor's pointers are global memory.  Read out of a structure they are generic to the compiler, and a generic access waits for
// every store before it; the device build says what they are.
#if defined(__HIP_DEVICE_COMPILE__)
#define JP_GLOBAL __attribute__((address_space(1)))
#else
#define JP_GLOBAL
#endif

// One scan of one file; the pointers are device memory (host memory in the host build).  Every scan has data, seg_byte and nseg (0: the
// file has no scan of this index); a first scan (Ah = 0) is cut into subsequences of S bits and decoded speculatively, as jpegdec.hip
// decodes a baseline scan, and has the rest of JpegSubs too.  An end-of-band run counts its blocks at its symbol.
struct JpScan : JpegSubs {
    const JpegHuff* huff;              // [ncs] per scan component: its DC table (Ss = 0) or AC table as it stood at this SOS
    short* coef;                       // the file's coefficient buffer
    int* status;                       // JD_ERR_* bits
    int nblocks;                       // blocks of the buffer
    int ncs, comp[3];                  // scan components: their indices in the frame
    int Ss, Se, Ah, Al;
    int ri, nunits;                    // units a segment / in the scan: MCUs (ncs > 1) or the component's blocks
    int bw;                            // ncs == 1: blocks a row of the component's raster
    int ch, cv, coff;                  // ncs == 1: the component's blocks across / down an MCU, its first block in the MCU
    int hs, vs, bpm, mcux, ncomp;      // the frame: JpegDesc's
};

// The bit reader of one segment, bytes [b0, b1) of `d`: a 64-bit window over bytes wb .. wb + 7 (wb a multiple of 4) and the 32 bits
// behind it, fetched one step ahead of their use so that the walk does not wait for them.
struct JpBits {
    const JP_GLOBAL uint8_t* d;
    unsigned b0, b1, p;                // p: next bit, counted from the start of `d`
    unsigned long long win;
    unsigned wb, ahead;
};
// the four bytes at a (a multiple of 4), first byte in the high bits; outside the segment: ones
JP_HD unsigned jp_load32(const JpBits& s, unsigned a) {
    if (a >= s.b0 && a + 4 <= s.b1) {
        const unsigned v = *(const JP_GLOBAL unsigned*)(s.d + a);                     // `d` is 4-byte aligned (jpegdec.cpp's blob, the host's vector)
        return (v << 24) | ((v & 0xFF00u) << 8) | ((v >> 8) & 0xFF00u) | (v >> 24);
    }
    unsigned w = 0;
    for (unsigned i = 0; i < 4; ++i) w = (w << 8) | ((a + i >= s.b0 && a + i < s.b1) ? (unsigned)s.d[a + i] : 0xFFu);
    return w;
}
// the reader of segment [b0, b1) at bit p
JP_HD JpBits jp_open_at(const uint8_t* d, unsigned b0, unsigned b1, unsigned p) {
    JpBits s{(const JP_GLOBAL uint8_t*)d, b0, b1, p, 0, (p >> 3) & ~3u, 0};
    s.win = ((unsigned long long)jp_load32(s, s.wb) << 32) | jp_load32(s, s.wb + 4);
    s.ahead = jp_load32(s, s.wb + 8);
    return s;
}
JP_HD JpBits jp_open(const uint8_t* d, unsigned b0, unsigned b1) { return jp_open_at(d, b0, b1, b0 * 8u); }
// n bits (1 .. 16) at the reader's position, which they do not move.  A read advances the position by at most 16 bits, so two steps of
// the window always reach it.
JP_HD unsigned jp_peek(JpBits& s, int n) {
    for (int i = 0; i < 2 && s.p - s.wb * 8u >= 32u; ++i) {
        s.win = (s.win << 32) | s.ahead;
        s.wb += 4;
        s.ahead = jp_load32(s, s.wb + 8);
    }
    const unsigned o = (s.p - s.wb * 8u) & 31u;
    return (unsigned)((s.win << o) >> (64 - n));
}
JP_HD unsigned jp_get(JpBits& s, int n) {
    const unsigned v = jp_peek(s, n);
    s.p += (unsigned)n;
    return v;
}
// one Huffman symbol; -1: a look-ahead without a code
JP_HD int jp_symbol(const JpegHuff& H, JpBits& s) {
    const unsigned v = jp_peek(s, 16);
    const unsigned e = H.look[v >> 7];
    if (e) {
        s.p += e >> 8;
        return (int)(e & 255);
    }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= H.maxcode[l]) {
            s.p += (unsigned)l;
            return H.val[(code + H.valoff[l]) & 255];
        }
    }
    return -1;
}
// jdhuff.h's HUFF_EXTEND of n received bits
JP_HD int jp_extend(unsigned bits, int n) { return bits >= (1u << (n - 1)) ? (int)bits : (int)bits - (1 << n) + 1; }

// frame component of scan component ci, without indexing the descriptor (which then stays in registers)
JP_HD int jp_scan_comp(const JpScan& sc, int ci) { return ci == 0 ? sc.comp[0] : (ci == 1 ? sc.comp[1] : sc.comp[2]); }

// the buffer's block of unit u of the scan (block j of scan component ci of MCU u when the scan interleaves); may lie outside the buffer
JP_HD long long jp_block(const JpScan& sc, int u, int ci, int j) {
    if (sc.ncs > 1) {
        const int c = jp_scan_comp(sc, ci);
        return (long long)u * sc.bpm + (sc.ncomp == 1 ? 0 : (c == 0 ? j : sc.hs * sc.vs + c - 1));
    }
    const int by = u / sc.bw, bx = u % sc.bw;
    return ((long long)(by / sc.cv) * sc.mcux + bx / sc.ch) * sc.bpm + sc.coff + (by % sc.cv) * sc.ch + bx % sc.ch;
}

// blocks of scan component ci in one unit of the scan
JP_HD int jp_unit_blocks(const JpScan& sc, int ci) { return sc.ncs > 1 && jp_scan_comp(sc, ci) == 0 && sc.ncomp == 3 ? sc.hs * sc.vs : 1; }

// DC refinement of unit u of the scan: one raw bit per block, no code, at the block's ordinal in its restart segment -- a plain parallel
// pass over the units.  The unit that opens a segment also checks that the segment holds the bits of its blocks and no byte more.
JP_HD int jp_dc_refine_unit(const JpScan& sc, int u) {
    if (u < 0 || u >= sc.nunits || sc.ri < 1) return JD_ERR_COUNT;
    const int seg = u / sc.ri, i = u - seg * sc.ri;
    if (seg >= sc.nseg) return JD_ERR_COUNT;
    int bpu = 0;
    for (int ci = 0; ci < sc.ncs; ++ci) bpu += jp_unit_blocks(sc, ci);
    const JP_GLOBAL int* seg_byte = (const JP_GLOBAL int*)sc.seg_byte;
    const JP_GLOBAL uint8_t* data = (const JP_GLOBAL uint8_t*)sc.data;
    JP_GLOBAL short* coef = (JP_GLOBAL short*)sc.coef;
    const unsigned b0 = (unsigned)seg_byte[seg], b1 = (unsigned)seg_byte[seg + 1];
    int err = 0;
    if (i == 0) {
        const long long nu = sc.nunits - (long long)seg * sc.ri < sc.ri ? sc.nunits - (long long)seg * sc.ri : sc.ri;
        const long long need = nu * bpu, have = ((long long)b1 - b0) * 8;
        if (need > have || have - need >= 8) err = JD_ERR_COUNT;
    }
    unsigned bit = b0 * 8u + (unsigned)i * (unsigned)bpu;
    for (int ci = 0; ci < sc.ncs; ++ci)
        for (int j = 0; j < jp_unit_blocks(sc, ci); ++j, ++bit) {
            const unsigned a = bit >> 3;
            const unsigned byte = a >= b0 && a < b1 ? data[a] : 0xFFu;
            const long long blk = jp_block(sc, u, ci, j);
            if (((byte >> (7 - (bit & 7))) & 1) && blk >= 0 && blk < sc.nblocks) coef[blk * 64] = (short)(coef[blk * 64] | (1 << sc.Al));
        }
    return err;
}

// A symbol of an AC refinement resolved with mask arithmetic instead of a walk over the coefficients.  nz: which coefficients have a
// history (bit = zig-zag position); k: where the walk stands; r: coefficients without a history to skip (64 and more: to the band's end,
// an end-of-band run).  -> target: the (r + 1)-th such coefficient from k (Se + 1: the band ended first), where a new coefficient goes or
// a run of 16 zeros ends; passed: the coefficients with a history before it, each of which takes one correction bit, in order.
struct JpWalk { int target; unsigned long long passed; };
JP_HD JpWalk jp_refine_walk(unsigned long long nz, int k, int Se, int r) {
    const unsigned long long upto = Se >= 63 ? ~0ull : (1ull << (Se + 1)) - 1, band = upto & ~((1ull << k) - 1);
    unsigned long long z = r >= 64 ? 0ull : ~nz & band;
    for (int i = 0; i < r && i < 16; ++i) z &= z - 1;
    JpWalk w;
    w.target = z ? __builtin_ctzll(z) : Se + 1;
    w.passed = nz & band & (w.target >= 64 ? ~0ull : (1ull << w.target) - 1);
    return w;
}

// One block of an AC refinement (decode_mcu_AC_refine) in the host's order: jpegprog.hip's wavefront resolves the same symbols with the
// same jp_refine_walk and applies the corrections of `passed` side by side.  Returns JD_ERR_* bits.
JP_HD int jp_ac_refine_block(int Ss, int Se, int Al, const JpegHuff& H, const unsigned char* ZZ, JpBits& s, JP_GLOBAL short* c, int& eobrun) {
    const int p1 = 1 << Al;
    unsigned long long nz = 0;
    for (int k = Ss; k <= Se; ++k)
        if (c[ZZ[k]] != 0) nz |= 1ull << k;
    int k = Ss;
    if (eobrun == 0) {
        for (; k <= Se; ++k) {
            const int sym = jp_symbol(H, s);
            if (sym < 0) return JD_ERR_CODE;
            const int r = sym >> 4, sz = sym & 15;
            bool place = false, negative = false;
            if (sz) {
                if (sz != 1) return JD_ERR_CODE;
                place = true;
                negative = !jp_get(s, 1);
            } else if (r != 15) {
                eobrun = 1 << r;
                if (r) eobrun += (int)jp_get(s, r);
                break;
            }
            const JpWalk w = jp_refine_walk(nz, k, Se, r);
            for (unsigned long long m = w.passed; m; m &= m - 1) {
                JP_GLOBAL short* q = c + ZZ[__builtin_ctzll(m)];
                if (jp_get(s, 1) && !(*q & p1)) *q = (short)(*q < 0 ? *q - p1 : *q + p1);
            }
            k = w.target;
            if (place) {
                if (k > Se) return JD_ERR_CODE;
                c[ZZ[k]] = (short)(negative ? -p1 : p1);
            }
        }
    }
    if (eobrun > 0) {
        for (unsigned long long m = k <= Se ? jp_refine_walk(nz, k, Se, 64).passed : 0ull; m; m &= m - 1) {
            JP_GLOBAL short* q = c + ZZ[__builtin_ctzll(m)];
            if (jp_get(s, 1) && !(*q & p1)) *q = (short)(*q < 0 ? *q - p1 : *q + p1);
        }
        --eobrun;
    }
    return 0;
}

// ---- the first scans (Ah = 0): DC first and AC first, decodable from any bit once the state there is known -- jpeg_spec.h's JpegState:
// the bit in `data`, the block in the unit (DC), the zig-zag position in the band (AC)
JP_HD int jp_unit_total(const JpScan& sc) {
    int n = 0;
    for (int ci = 0; ci < sc.ncs && ci < 3; ++ci) n += jp_unit_blocks(sc, ci);
    return n;
}
// scan component of block w of a unit; *j receives the block's index within that component
JP_HD int jp_unit_comp(const JpScan& sc, int w, int* j) {
    int ci = 0;
    for (int c = 0; c + 1 < sc.ncs && c < 2; ++c) {
        const int nb = jp_unit_blocks(sc, c);
        if (ci == c && w >= nb) { w -= nb; ci = c + 1; }
    }
    *j = w;
    return ci;
}
// the buffer's block of block o of the scan, counted in scan order from its start
JP_HD long long jp_ordinal_block(const JpScan& sc, int bpu, long long o) {
    int j;
    const int ci = jp_unit_comp(sc, (int)(o % bpu), &j);
    return jp_block(sc, (int)(o / bpu), ci, j);
}
// The start state of a segment: block 0 of the unit, the band's first coefficient.
JP_HD JpegState jp_start(const JpScan& sc, unsigned p) { return JpegState{p, 0, sc.Ss}; }
// ... and where its last subsequence, bits [.., b1 * 8), must end: there again, less than a byte of padding left
JP_HD bool jp_at_end(const JpScan& sc, const JpegState& st, unsigned b1) { return st.b == 0 && st.z == sc.Ss && st.p <= b1 * 8u && b1 * 8u - st.p < 8u; }

// Decode from st while its bit is before `end` and fewer than max_blocks blocks are complete.  Returns the blocks completed; an
// end-of-band run counts its blocks at its symbol, since they take no bits -- the state stays (bit, place in the band).  *invalid: a
// pattern without a code, a DC category above 15 or a coefficient behind the block; *over: a run that leaves the max_blocks.  store:
// coefficients of block first + n (in scan order) are stored, DC terms as differences.  At most S + 32 symbols: each takes a bit.
JP_HD int jp_run_first(const JpScan& sc, const JpegHuff* T, const unsigned char* ZZ, int bpu, unsigned b0, unsigned b1, JpegState& st, unsigned end,
                       int max_blocks, bool store, long long first, bool* invalid, bool* over) {
    JpBits s = jp_open_at(sc.data, b0, b1, st.p);
    JP_GLOBAL short* coef = (JP_GLOBAL short*)sc.coef;
    const int Ss = sc.Ss, Se = sc.Se, Al = sc.Al, S = sc.S;
    int b = st.b, z = st.z, n = 0;
    *invalid = *over = false;
    for (int it = 0; it < S + 32 && s.p < end && n < max_blocks; ++it) {
        if (Ss == 0) {
            int j;
            const int ci = jp_unit_comp(sc, b, &j);
            const int sz = jp_symbol(T[ci], s);
            if (sz < 0 || sz > 15) { *invalid = true; s.p = end; break; }
            const int diff = sz ? jp_extend(jp_get(s, sz), sz) : 0;
            if (store) {
                const long long blk = jp_ordinal_block(sc, bpu, first + n);
                if (blk >= 0 && blk < sc.nblocks) coef[blk * 64] = (short)diff;
            }
            b = b + 1 >= bpu ? 0 : b + 1;
            n += 1;
            continue;
        }
        const int sym = jp_symbol(T[0], s);
        if (sym < 0) { *invalid = true; s.p = end; break; }
        const int r = sym >> 4, sz = sym & 15;
        if (sz) {
            z += r;
            const int v = jp_extend(jp_get(s, sz), sz);
            if (z > 63) { *invalid = true; s.p = end; break; }
            if (store) {
                const long long blk = jp_block(sc, (int)(first + n), 0, 0);
                if (blk >= 0 && blk < sc.nblocks) coef[blk * 64 + ZZ[z]] = (short)((unsigned)v << Al);
            }
            z += 1;
        } else if (r == 15) {
            z += 16;
        } else {
            int run = 1 << r;
            if (r) run += (int)jp_get(s, r);
            if (run > max_blocks - n) { *over = true; n = max_blocks; z = Ss; break; }
            n += run - 1;
            z = Se + 1;
        }
        if (z > Se) {
            z = Ss;
            n += 1;
        }
    }
    st.p = s.p;
    st.b = b;
    st.z = z;
    return n;
}

// The running sums of a DC first scan for items [i0, i0 + cnt) of scan component ci in segment seg, `carry` the sum before them:
// the differences the run stored become the terms, shifted by Al.  Returns the sum behind them.  (The device runs it 64 items at a time.)
JP_HD long long jp_dc_item_block(const JpScan& sc, int seg, int ci, int i) {
    const int nb = jp_unit_blocks(sc, ci);
    return jp_block(sc, seg * sc.ri + i / nb, ci, i % nb);
}

// One restart segment in the host's order.  ZZ: JPEG_ZZ.  A first scan goes subsequence by subsequence through jpeg_spec.h's lookup and
// packed state, as the device's lanes do one beside the other.
JP_HD int jp_decode_segment(const JpScan& sc, const JpegHuff* T, const unsigned char* ZZ, int seg) {
    if (seg < 0 || seg >= sc.nseg || sc.ri < 1 || sc.bw < 1 || sc.ch < 1 || sc.cv < 1) return JD_ERR_COUNT;
    const JP_GLOBAL int* seg_byte = (const JP_GLOBAL int*)sc.seg_byte;
    JP_GLOBAL short* coef = (JP_GLOBAL short*)sc.coef;
    const long long u0 = (long long)seg * sc.ri;
    const int nu = (int)(sc.nunits - u0 < sc.ri ? sc.nunits - u0 : sc.ri);
    const int Ss = sc.Ss, Se = sc.Se, Ah = sc.Ah, Al = sc.Al;         // read once: a store to the coefficients may not alias them
    const bool dc = Ss == 0;
    int eobrun = 0, err = 0;
    if (dc && Ah > 0) {                                              // the host's order of the device's parallel pass
        for (int i = 0; i < nu; ++i) err |= jp_dc_refine_unit(sc, (int)u0 + i);
        return err;
    }
    if (Ah == 0) {                                                    // the host's order of the device's subsequences: one after the other
        const int bpu = jp_unit_total(sc);
        const unsigned b1 = (unsigned)seg_byte[seg + 1];
        unsigned long long state = jpeg_pack(jp_start(sc, (unsigned)seg_byte[seg] * 8u));   // packed, as a lane hands it to its neighbour
        long long done = 0;
        const long long want = (long long)nu * bpu;
        for (int i = sc.seg_sub[seg]; i < sc.seg_sub[seg + 1] && !err; ++i) {
            bool invalid, over;
            const JpegSub s = jpeg_sub(sc, i);
            JpegState st = jpeg_unpack(state);
            done += jp_run_first(sc, T, ZZ, bpu, s.b0, s.b1, st, s.end, (int)(want - done), true, u0 * bpu + done, &invalid, &over);
            state = jpeg_pack(st);
            if (invalid) err = JD_ERR_CODE;
            else if (over) err = JD_ERR_COUNT;
        }
        if (!err && (done != want || !jp_at_end(sc, jpeg_unpack(state), b1))) err = JD_ERR_COUNT;
        if (dc && !err)
            for (int ci = 0; ci < sc.ncs && ci < 3; ++ci) {
                unsigned sum = 0;
                const int items = nu * jp_unit_blocks(sc, ci);
                for (int i = 0; i < items; ++i) {
                    const long long blk = jp_dc_item_block(sc, seg, ci, i);
                    if (!(blk >= 0 && blk < sc.nblocks)) continue;
                    sum += (unsigned)(int)coef[blk * 64];
                    coef[blk * 64] = (short)(sum << Al);
                }
            }
        return err;
    }
    JpBits s = jp_open(sc.data, (unsigned)seg_byte[seg], (unsigned)seg_byte[seg + 1]);
    for (int i = 0; i < nu && !err; ++i) {
        const long long blk = jp_block(sc, (int)u0 + i, 0, 0);
        if (!(blk >= 0 && blk < sc.nblocks) || Ss < 1 || Se > 63) { err = JD_ERR_COUNT; break; }   // never, for a plan of jpeg_parse.h
        err = jp_ac_refine_block(Ss, Se, Al, T[0], ZZ, s, coef + blk * 64, eobrun);
    }
    if (!err && (eobrun != 0 || s.p > s.b1 * 8u || s.b1 * 8u - s.p >= 8u)) err = JD_ERR_COUNT;
    return err;
}

// The refinements among scans[0 .. n): a DC refinement one lane per unit, an AC refinement one wavefront per restart segment.  max_groups:
// the most workgroups of 64 lanes one of them needs (jp_scan_groups).
inline int jp_scan_groups(int ss, int ah, int nseg, int nunits) { return ah == 0 ? 0 : (ss == 0 ? (nunits + 63) / 64 : nseg); }
hipError_t launch_jp_scan(const JpScan* scans, int n, int max_groups, hipStream_t s);
// The first scans among scans[0 .. n): `passes` synchronisation launches (one more than the workgroups of 64 subsequences a scan spans at
// most, max_groups), the prefix of the counts, the write pass and the DC sums (max_seg: the most restart segments of a scan).
hipError_t launch_jp_first(const JpScan* scans, int n, int max_groups, int passes, int max_seg, hipStream_t s);
