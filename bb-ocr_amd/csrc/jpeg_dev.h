// Device functions of libjpeg-turbo's decoder half that two translation units run: the thumbnail's JPEG round trip (thumb.hip) and the
// baseline decoder (jpegdec.hip).  Each is stated against jidctint.c / jdsample.c by tests/jpeg_ref.py.
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
