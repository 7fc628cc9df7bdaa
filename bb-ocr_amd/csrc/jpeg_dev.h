// Device functions of libjpeg-turbo that more than one translation unit runs: the decoder half (jidctint.c, jdsample.c) of the thumbnail's
// JPEG round trip (thumb.hip) and the baseline decoder (jpegdec.hip), the encoder half (jccolor.c, jfdctint.c) of the round trip and the
// baseline encoder (jpegenc.hip), and the encoder's entropy coding of one block (jchuff.c), which also compiles for the host.  Each is
// stated by tests/jpeg_ref.py / tests/jpeg_encode_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- libjpeg's ISLOW transforms (jfdctint.c / jidctint.c), CONST_BITS 13, PASS1_BITS 2, in 64-bit like JLONG
constexpr int CB = 13, P1 = 2;
constexpr long long F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                    F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
__device__ __forceinline__ long long dsc(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }

// one 1-D inverse pass; the second (row) pass returns the samples through the post-IDCT range-limit table
__device__ __forceinline__ void idct8(int* v, int s, bool first) {
    long long z2 = v[2 * s], z3 = v[6 * s];
    long long z1 = (z2 + z3) * F0541;
    const long long t2e = z1 - z3 * F1847, t3e = z1 + z2 * F0765;
    z2 = v[0] + (first ? 0 : (1 << (P1 + 2)));
    z3 = v[4 * s];
    const long long t0e = (z2 + z3) << CB, t1e = (z2 - z3) << CB;
    const long long t10 = t0e + t3e, t13 = t0e - t3e, t11 = t1e + t2e, t12 = t1e - t2e;
    long long t0 = v[7 * s], t1 = v[5 * s], t2 = v[3 * s], t3 = v[s];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    long long z4 = t1 + t3;
    const long long z5 = (z3 + z4) * F1175;
    t0 *= F0298; t1 *= F2053; t2 *= F3072; t3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    const long long o[8] = {t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3};
    for (int i = 0; i < 8; ++i) {
        if (first) {
            v[i * s] = (int)dsc(o[i], CB - P1);
        } else {
            const int r = (int)(o[i] >> (CB + P1 + 3)) & 1023;          // RANGE_MASK
            v[i * s] = r < 128 ? r + 128 : (r < 512 ? 255 : (r < 896 ? 0 : r - 896));
        }
    }
}

// ---- libjpeg's reduced-size inverse transforms (jidctred.c), which a decode at scale 1/2, 1/4 or 1/8 runs: one 1-D pass over the eight
// inputs v[0], v[s], ..., v[7 s] that leaves its N outputs in v[0], ..., v[(N - 1) s].  The first (column) pass descales to PASS1_BITS
// fraction bits; the second (row) pass returns the samples through the post-IDCT range-limit table.
__device__ __forceinline__ int jd_range_limit(long long x) {
    const int r = (int)x & 1023;                                        // RANGE_MASK
    return r < 128 ? r + 128 : (r < 512 ? 255 : (r < 896 ? 0 : r - 896));
}

// jpeg_idct_4x4: input 4 is never read
__device__ __forceinline__ void idct4(int* v, int s, bool first) {
    const long long i0 = v[0], i1 = v[s], i2 = v[2 * s], i3 = v[3 * s], i5 = v[5 * s], i6 = v[6 * s], i7 = v[7 * s];
    const long long t0 = i0 << (CB + 1), t2 = i2 * F1847 - i6 * F0765;
    const long long t10 = t0 + t2, t12 = t0 - t2;
    const long long oa = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697;      // FIX 0.211164243, 1.451774981, 2.172734803, 1.061594337
    const long long ob = -i7 * 4176 - i5 * 4926 + i3 * F0899 + i1 * F2562;      // FIX 0.509795579, 0.601344887, 0.899976223, 2.562915447
    const int sh = first ? CB - P1 + 1 : CB + P1 + 3 + 1;
    const long long o[4] = {dsc(t10 + ob, sh), dsc(t12 + oa, sh), dsc(t12 - oa, sh), dsc(t10 - ob, sh)};
    for (int i = 0; i < 4; ++i) v[i * s] = first ? (int)o[i] : jd_range_limit(o[i]);
}

// jpeg_idct_2x2: inputs 2, 4 and 6 are never read
__device__ __forceinline__ void idct2(int* v, int s, bool first) {
    const long long t10 = (long long)v[0] << (CB + 2);
    const long long t0 = -(long long)v[7 * s] * 5906 + (long long)v[5 * s] * 6967 - (long long)v[3 * s] * 10426 +
                         (long long)v[s] * 29692;                                // FIX 0.720959822, 0.850430095, 1.272758580, 3.624509785
    const int sh = first ? CB - P1 + 2 : CB + P1 + 3 + 2;
    const long long a = dsc(t10 + t0, sh), b = dsc(t10 - t0, sh);
    v[0] = first ? (int)a : jd_range_limit(a);
    v[s] = first ? (int)b : jd_range_limit(b);
}

// jpeg_idct_1x1 of the dequantised DC term
__device__ __forceinline__ int idct1(int dc) { return jd_range_limit(dsc((long long)dc, 3)); }

// ---- jfdctint.c
// one 1-D forward pass over v[0], v[s], ..., v[7 s]
__device__ __forceinline__ void fdct8(int* v, int s, bool first) {
    const long long t0 = v[0] + v[7 * s], t7 = v[0] - v[7 * s], t1 = v[s] + v[6 * s], t6 = v[s] - v[6 * s];
    const long long t2 = v[2 * s] + v[5 * s], t5 = v[2 * s] - v[5 * s], t3 = v[3 * s] + v[4 * s], t4 = v[3 * s] - v[4 * s];
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = first ? CB - P1 : CB + P1;
    v[0] = (int)(first ? (t10 + t11) << P1 : dsc(t10 + t11, P1));
    v[4 * s] = (int)(first ? (t10 - t11) << P1 : dsc(t10 - t11, P1));
    long long z1 = (t12 + t13) * F0541;
    v[2 * s] = (int)dsc(z1 + t13 * F0765, sh);
    v[6 * s] = (int)dsc(z1 - t12 * F1847, sh);
    z1 = t4 + t7;
    long long z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const long long z5 = (z3 + z4) * F1175;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    v[7 * s] = (int)dsc(t4 * F0298 + z1 + z3, sh);
    v[5 * s] = (int)dsc(t5 * F2053 + z2 + z4, sh);
    v[3 * s] = (int)dsc(t6 * F3072 + z2 + z3, sh);
    v[s] = (int)dsc(t7 * F1501 + z1 + z4, sh);
}

// jccolor.c::rgb_ycc_convert
__device__ __forceinline__ int th_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int th_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int th_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// one chroma sample of h2v2_fancy_upsample at output (y, x); the plane is ch x cw valid samples (rows `cpitch` apart)
__device__ __forceinline__ int th_fancy(const uint8_t* __restrict__ c, int cpitch, int ch, int cw, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return c[(size_t)cy * cpitch + cx];           // h2v2_upsample
    const int ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t* r0 = c + (size_t)cy * cpitch;
    const uint8_t* r1 = c + (size_t)ny * cpitch;
    const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    const int s = 3 * r0[cx] + r1[cx], sn = 3 * r0[nx] + r1[nx];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// one chroma sample of h2v1_fancy_upsample (4:2:2) at output (y, x): the row has cw valid samples; h2v1_upsample when cw <= 2.  The end
// samples come out copied: their neighbour is clamped to themselves.
__device__ __forceinline__ int th_fancy_h2v1(const uint8_t* __restrict__ c, int cpitch, int cw, int y, int x) {
    const uint8_t* r = c + (size_t)y * cpitch;
    const int cx = x >> 1;
    if (cw <= 2) return r[cx];
    const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    return (3 * r[cx] + r[nx] + ((x & 1) ? 2 : 1)) >> 2;
}

// one chroma sample of h1v2_fancy_upsample (4:4:0) at output (y, x): the plane has ch valid rows; the rows above the first and below the
// last are those rows again
__device__ __forceinline__ int th_fancy_h1v2(const uint8_t* __restrict__ c, int cpitch, int ch, int y, int x) {
    const int cy = y >> 1;
    const int ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    return (3 * c[(size_t)cy * cpitch + x] + c[(size_t)ny * cpitch + x] + ((y & 1) ? 2 : 1)) >> 2;
}

// ---- jchuff.c::encode_one_block of one block of quantised coefficients in zig-zag order, as a bit count and as bits.  JeHuff (kernels.h)
// holds (code << 5) | length per symbol.  Also compiled for the host, where a stand-alone program runs both against Pillow's scan.
#ifdef __HIP_DEVICE_COMPILE__
#define JE_CLZ(x) __clz((int)(x))
#else
#define JE_CLZ(x) ((x) ? __builtin_clz((unsigned)(x)) : 32)
#endif
__host__ __device__ __forceinline__ int je_nbits(int v) { return 32 - JE_CLZ(v < 0 ? -v : v); }

// bits of the block whose DC term follows `prev_dc` of its component; dc / ac: the component's tables
__host__ __device__ inline int je_block_bits(const short* zz, int prev_dc, const uint32_t* dc, const uint32_t* ac) {
    const int n = je_nbits(zz[0] - prev_dc);
    int bits = (int)(dc[n] & 31) + n, r = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++r;
            continue;
        }
        const int s = je_nbits(v);
        bits += (r >> 4) * (int)(ac[0xF0] & 31) + (int)(ac[((r & 15) << 4) + s] & 31) + s;
        r = 0;
    }
    return r ? bits + (int)(ac[0] & 31) : bits;
}

// Writer of bits at a bit offset of a zeroed buffer of 32-bit words that hold the stream MSB first, byte after byte (so a word is stored
// byte-swapped).  The words a run of bits shares with its neighbours -- the first it touches and the one finish() writes -- are OR-ed
// in (atomically on the device: the result is the same in whatever order the runs are written); the words between are its own.
struct JeBits {
    uint32_t* w;                 // next word
    unsigned long long acc;      // low `n` bits: not yet written (bits in front of a run's first word are zero)
    int n;
    bool first;
    __host__ __device__ JeBits(uint32_t* words, long long bit) : w(words + (bit >> 5)), acc(0), n((int)(bit & 31)), first(true) {}
    __host__ __device__ __forceinline__ void merge(uint32_t v) {
        v = __builtin_bswap32(v);
#ifdef __HIP_DEVICE_COMPILE__
        atomicOr(w, v);
#else
        *w |= v;
#endif
    }
    __host__ __device__ __forceinline__ void put(uint32_t code, int len) {       // len <= 16
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const uint32_t v = (uint32_t)(acc >> (n - 32));
            if (first) merge(v);
            else *w = __builtin_bswap32(v);
            first = false;
            ++w;
            n -= 32;
        }
    }
    __host__ __device__ __forceinline__ void finish() {
        if (n) merge((uint32_t)(acc << (32 - n)));
    }
};

__host__ __device__ __forceinline__ void je_put_value(JeBits& o, int v, int s) { o.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s); }

__host__ __device__ inline void je_block_pack(JeBits& o, const short* zz, int prev_dc, const uint32_t* dc, const uint32_t* ac) {
    const int diff = zz[0] - prev_dc, n = je_nbits(diff);
    o.put(dc[n] >> 5, (int)(dc[n] & 31));
    if (n) je_put_value(o, diff, n);
    int r = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++r;
            continue;
        }
        for (; r > 15; r -= 16) o.put(ac[0xF0] >> 5, (int)(ac[0xF0] & 31));
        const int s = je_nbits(v);
        const uint32_t e = ac[(r << 4) + s];
        o.put(e >> 5, (int)(e & 31));
        je_put_value(o, v, s);
        r = 0;
    }
    if (r) o.put(ac[0] >> 5, (int)(ac[0] & 31));
}
