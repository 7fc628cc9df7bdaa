// Speculative Huffman decoding with self-synchronisation (Weissenberger & Schmidt), written once for jpegdec.hip's baseline scan and
// jpegprog.hip's first scans: the zig-zag order, the state a lane carries between subsequences, the lookup of a subsequence in a
// JpegSubs (kernels.h), and the three passes over it as templates over a codec policy C --
//   jpeg_sync_pass    one lane per S-bit subsequence: decode from the assumed state, then take the left neighbour's exit state and decode
//                     again until no state of the workgroup changes; launched once more per workgroup a segment spans, a launch returning
//                     at once when the launch before it changed nothing (flags[pass - 1] == 0; pass 0 always sets its flag)
//   jpeg_prefix_pass  exclusive scan of the block counts: first output block of every subsequence
//   jpeg_write_pass   decode from the exact entry states into the coefficient buffer; checks what the file promised (JD_ERR_*)
// C supplies what differs: Desc (JpegDesc, JpScan) and Lds (where its tables stand in LDS), cut(d) (the descriptor holds a cut scan),
// load (tables into LDS, then a barrier), unit_blocks / units (blocks of a unit, units of the scan: d.ri units a segment), start (a
// segment's first state), run (decode one subsequence), at_end (the state a segment's last subsequence must end in) and note_first.
// The kernels of the two files hold the descriptor -- by value or in place -- and the LDS, and call a pass.  The first part compiles
// for the host as well (jpegprog.h's jp_decode_segment, jpeg_parse.h).
#pragma once
#include <stdint.h>
#include "kernels.h"

#if defined(__HIPCC__)
#define JP_HD __host__ __device__ __forceinline__
#else
#define JP_HD inline
#endif

// zig-zag position -> place in the block in natural order: the one table of the decoder, device and host
constexpr unsigned char JPEG_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegState { unsigned p; int b, z; };                       // bit in `data`, block in the unit (MCU), zig-zag position
JP_HD unsigned long long jpeg_pack(const JpegState& s) {
    return (unsigned long long)s.p | ((unsigned long long)(unsigned)s.b << 32) | ((unsigned long long)(unsigned)s.z << 40);
}
JP_HD JpegState jpeg_unpack(unsigned long long v) { return JpegState{(unsigned)v, (int)((v >> 32) & 7), (int)((v >> 40) & 63)}; }

// subsequence i: the j-th of segment seg, whose bytes are [b0, b1); its bits are [start, end)
struct JpegSub { int seg, j; unsigned b0, b1, start, end; };
JP_HD JpegSub jpeg_sub(const JpegSubs& d, int i) {
    JpegSub s;
    const int g = d.sub_seg[i];
    s.seg = g < 0 ? 0 : (g > d.nseg - 1 ? d.nseg - 1 : g);
    s.j = i - d.seg_sub[s.seg];
    s.b0 = (unsigned)d.seg_byte[s.seg];
    s.b1 = (unsigned)d.seg_byte[s.seg + 1];
    s.start = s.b0 * 8u + (unsigned)s.j * (unsigned)d.S;
    s.end = s.start + (unsigned)d.S < s.b1 * 8u ? s.start + (unsigned)d.S : s.b1 * 8u;
    return s;
}

#if defined(__HIPCC__)
// ex: JD_LANES words of LDS, the exit states of the workgroup's lanes
template <class C> __device__ __forceinline__ void jpeg_sync_pass(const typename C::Desc& d, const typename C::Lds& lds, unsigned long long* ex, int pass) {
    const int t = threadIdx.x, i = blockIdx.x * JD_LANES + t;
    if (!C::cut(d) || (int)blockIdx.x * JD_LANES >= d.nsub || pass >= d.passes) return;
    if (pass > 0 && d.flags[pass - 1] == 0) return;           // the pass before changed nothing: every state is final
    C::load(d, lds, t, JD_LANES);
    const int bpu = C::unit_blocks(d);
    const bool valid = i < d.nsub;
    JpegSub s{};
    unsigned long long entry = 0, exit_ = 0;
    int count = 0;
    bool inv, over;
    if (valid) {
        s = jpeg_sub(d, i);
        if (pass == 0) {
            JpegState st = C::start(d, s.start);
            entry = jpeg_pack(st);
            count = C::run(d, lds, bpu, s, st, 0x7fffffff, false, 0, &inv, &over);
            exit_ = jpeg_pack(st);
        } else {
            entry = d.entry[i];
            exit_ = d.exits[i];
            count = d.count[i];
        }
    }
    bool any = false;
    for (int iter = 0; iter <= JD_LANES; ++iter) {
        ex[t] = exit_;
        __syncthreads();
        bool ch = false;
        if (valid && s.j > 0) {                               // subsequence 0 of a segment is exact by construction
            unsigned long long prev = entry;
            if (t > 0) prev = ex[t - 1];
            else if (pass > 0) prev = __hip_atomic_load(&d.exits[i - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev != entry) {
                entry = prev;
                JpegState st = jpeg_unpack(entry);
                count = C::run(d, lds, bpu, s, st, 0x7fffffff, false, 0, &inv, &over);
                exit_ = jpeg_pack(st);
                ch = true;
            }
        }
        if (!__syncthreads_or(ch)) break;
        any = true;
    }
    if (valid) {
        d.entry[i] = entry;
        __hip_atomic_store(&d.exits[i], exit_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d.count[i] = count;
    }
    if (t == 0 && (pass == 0 ? blockIdx.x == 0 : any)) d.flags[pass] = 1;
}

// one workgroup of 256 lanes per scan; sh: 256 words of LDS.  The runs of a damaged stream may sum past the scan: the sum saturates.
template <class C> __device__ __forceinline__ void jpeg_prefix_pass(const typename C::Desc& d, long long* sh) {
    if (!C::cut(d)) return;
    const int t = threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < d.nsub; base += 256) {
        const int i = base + t;
        const long long v = i < d.nsub ? d.count[i] : 0;
        sh[t] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const long long a = t >= o ? sh[t - o] : 0;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (i < d.nsub) d.scan[i] = (int)min(carry + sh[t] - v, 0x7fffffffLL);
        carry += sh[255];
        __syncthreads();
    }
}

template <class C> __device__ __forceinline__ void jpeg_write_pass(const typename C::Desc& d, const typename C::Lds& lds) {
    const int t = threadIdx.x, i = blockIdx.x * JD_LANES + t;
    if (!C::cut(d) || (int)blockIdx.x * JD_LANES >= d.nsub) return;
    C::load(d, lds, t, JD_LANES);
    if (i >= d.nsub) return;
    const int bpu = C::unit_blocks(d);
    const JpegSub s = jpeg_sub(d, i);
    const unsigned long long entry = d.entry[i];
    int err = 0;
    if (s.j > 0 && d.exits[i - 1] != entry) err |= JD_ERR_SYNC;
    const long long seg_first = (long long)s.seg * d.ri * bpu;
    const long long seg_end = seg_first + (long long)min(d.ri, C::units(d) - s.seg * d.ri) * bpu;
    const long long first = seg_first + ((long long)d.scan[i] - d.scan[d.seg_sub[s.seg]]);
    C::note_first(d, i, first);
    const int room = (int)max(min(seg_end - first, 0x7fffffffLL), 0LL);
    JpegState st = jpeg_unpack(entry);
    bool inv, over;
    const int n = C::run(d, lds, bpu, s, st, room, true, first, &inv, &over);
    if (inv) err |= JD_ERR_CODE;
    if (over || n != d.count[i]) err |= JD_ERR_COUNT;
    if (i + 1 == d.seg_sub[s.seg + 1] && (first + n != seg_end || !C::at_end(d, st, s))) err |= JD_ERR_COUNT;
    if (err) atomicOr(d.status, err);
}
#endif
