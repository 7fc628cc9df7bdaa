// The trace previews' PNG files written on the device: a lossless 8-bit gray or RGB PNG whose IDAT is one zlib stream of independent
// deflate blocks, one per chunk of PNG_CHUNK bytes of the filtered stream.  tests/png_ref.py states every rule below; the device is held to
// it byte for byte.
//   png_filter   one row per workgroup: the five PNG filters over the raw neighbours, the sum of |(int8) x| of each, the smallest sum wins
//                (ties: the lowest filter number); [filter byte][row] at y * (1 + W * c)
//   png_codes    one chunk per workgroup: the tokens (png_token: run heads and leftovers are literals, the rest of a run of equal bytes is
//                matches of distance 1), their histogram, the code lengths of the dynamic block (png_code_lengths), its header
//                (png_header_tokens), the block's exact size, the choice stored / dynamic, the Adler-32 sums
//   (scan)       launch_je_scan over the chunk sizes
//   png_pack     one chunk per workgroup: canonical codes, header + tokens + end of block + the empty stored block packed in LDS (per-token
//                bit offsets by a block scan), written at the chunk's offset in the compacted buffer
// Everything is integer work; the only atomics are integer sums and ORs into LDS, whose results do not depend on their order.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PNG_SEG = 64;                                    // chunk bytes per thread (256 threads)
constexpr int PNG_SEG_PITCH = 68;                              // LDS bytes between two threads' segments: 17 dwords, so the lanes' reads fall on different banks
constexpr int PNG_OUT_WORDS = (PNG_CHUNK + 5) / 4 + 8;         // a dynamic block is shorter than the stored one (5 + PNG_CHUNK bytes)
constexpr int PNG_MAX_TOK = PNG_LITLEN + 2;                    // header tokens: at most one per code length

struct PngLenTab {
    uint8_t sym[259];                                          // match length -> length symbol - 257
    uint8_t extra[29];                                         // extra bits of the symbol
    uint16_t base[29];                                         // its first length
};
constexpr PngLenTab png_len_tab() {                            // RFC 1951 3.2.5
    PngLenTab t{};
    int len = 3;
    for (int s = 0; s < 28; ++s) {
        const int e = s < 8 ? 0 : (s - 4) / 4;
        t.extra[s] = (uint8_t)e;
        t.base[s] = (uint16_t)len;
        for (int k = 0; k < (1 << e); ++k) t.sym[len++] = (uint8_t)s;
    }
    t.sym[258] = 28;                                           // 258 has its own symbol (285, no extra bits)
    t.extra[28] = 0;
    t.base[28] = 258;
    return t;
}
__device__ const PngLenTab PNG_LEN = png_len_tab();
__device__ const uint8_t PNG_CL_ORDER[PNG_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ------------------------------------------------------------------------------------------------ stage A
__device__ __forceinline__ int png_abs8(int v) { return v < 128 ? v : 256 - v; }
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// the five filtered values of stream byte j of a row (a: left, b: up, c: up-left; 0 outside the page)
__device__ __forceinline__ void png_filters(int x, int a, int b, int c, int* f) {
    f[0] = x;
    f[1] = (x - a) & 255;
    f[2] = (x - b) & 255;
    f[3] = (x - ((a + b) >> 1)) & 255;
    f[4] = (x - png_paeth(a, b, c)) & 255;
}

__global__ void __launch_bounds__(256) png_filter_kernel(const uint8_t* __restrict__ src, size_t pitch, int layout, int H, int W, uint8_t* __restrict__ stream) {
    __shared__ unsigned long long sums[5][256];
    const int t = threadIdx.x, y = blockIdx.x, bpp = layout == PAGE_GRAY ? 1 : 3;
    const long long nb = (long long)W * bpp;
    const bool swap = layout == PAGE_BGR;
    const uint8_t* cur = src + (size_t)y * pitch;
    const uint8_t* up = y > 0 ? cur - pitch : nullptr;
    auto at = [&](const uint8_t* row, long long j) -> int {      // stream byte j of a row: channel order R, G, B
        if (!row || j < 0) return 0;
        return row[swap ? j + 2 - 2 * (j % 3) : j];
    };
    unsigned long long s[5] = {0, 0, 0, 0, 0};
    for (long long j = t; j < nb; j += 256) {
        int f[5];
        png_filters(at(cur, j), at(cur, j - bpp), at(up, j), at(up, j - bpp), f);
        for (int k = 0; k < 5; ++k) s[k] += (unsigned long long)png_abs8(f[k]);
    }
    for (int k = 0; k < 5; ++k) sums[k][t] = s[k];
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d)
            for (int k = 0; k < 5; ++k) sums[k][t] += sums[k][t + d];
        __syncthreads();
    }
    int best = 0;
    for (int k = 1; k < 5; ++k)
        if (sums[k][0] < sums[best][0]) best = k;
    uint8_t* out = stream + (size_t)y * (size_t)(nb + 1);
    if (t == 0) out[0] = (uint8_t)best;
    for (long long j = t; j < nb; j += 256) {
        int f[5];
        png_filters(at(cur, j), at(cur, j - bpp), at(up, j), at(up, j - bpp), f);
        out[1 + j] = (uint8_t)f[best];
    }
}

// ------------------------------------------------------------------------------------------------ stage B: tokens
__device__ __forceinline__ int png_at(const uint8_t* b, int p) { return b[(p >> 6) * PNG_SEG_PITCH + (p & 63)]; }

__device__ __forceinline__ void png_load_chunk(const uint8_t* __restrict__ src, int n, uint8_t* b) {
    const int t = threadIdx.x;
    if (((uintptr_t)src & 3) == 0) {
        const uint32_t* g = (const uint32_t*)src;
        for (int e = t; e < (n >> 2); e += 256) *(uint32_t*)(b + ((e * 4) >> 6) * PNG_SEG_PITCH + ((e * 4) & 63)) = g[e];
        for (int e = (n & ~3) + t; e < n; e += 256) b[(e >> 6) * PNG_SEG_PITCH + (e & 63)] = src[e];
    } else {
        for (int e = t; e < n; e += 256) b[(e >> 6) * PNG_SEG_PITCH + (e & 63)] = src[e];
    }
}

// Byte k of a maximal run of L equal bytes: 1 = a literal, 3 .. 258 = a match of that length (distance 1) starts here, 0 = inside a match.
// The run's first byte is a literal; of the R = L - 1 others, while R >= 3 a match takes min(R, 258); the last 0 .. 2 are literals.
__device__ __forceinline__ int png_token(int k, int L) {
    if (k == 0) return 1;
    const int j = k - 1, q = j / 258, rem = L - 1 - q * 258;
    if (rem < 3) return 1;
    return j == q * 258 ? min(rem, 258) : 0;
}

// The runs a thread's segment [t * 64, t * 64 + 64) lies in.  A break is a position whose byte differs from the one before it (position 0
// is one).  start_in: the last break before the segment; end_out: the first break behind it, or n.  Contains a barrier.
struct PngRuns { int p0, p1, start_in, end_out; };
__device__ __forceinline__ PngRuns png_runs(const uint8_t* b, int n, int* lastbrk, int* firstbrk) {
    const int t = threadIdx.x;
    PngRuns r{min(t * PNG_SEG, n), min(t * PNG_SEG + PNG_SEG, n), 0, n};
    int lb = -1, fb = n, prev = r.p0 > 0 ? png_at(b, r.p0 - 1) : -1;
    for (int i = r.p0; i < r.p1; ++i) {
        const int v = png_at(b, i);
        if (v != prev) {
            if (fb == n) fb = i;
            lb = i;
        }
        prev = v;
    }
    lastbrk[t] = lb;
    firstbrk[t] = fb;
    __syncthreads();
    for (int u = t - 1; u >= 0; --u)
        if (lastbrk[u] >= 0) { r.start_in = lastbrk[u]; break; }
    for (int u = t + 1; u < 256; ++u)
        if (firstbrk[u] < n) { r.end_out = firstbrk[u]; break; }
    return r;
}

// f(position, byte, token) for every position of the thread's segment, in order
template <typename F> __device__ __forceinline__ void png_walk(const uint8_t* b, const PngRuns& r, F&& f) {
    int i = r.p0;
    while (i < r.p1) {
        const int v = png_at(b, i);
        const bool brk = i == 0 || png_at(b, i - 1) != v;
        const int s = brk ? i : r.start_in;
        int e = i + 1;
        while (e < r.p1 && png_at(b, e) == v) ++e;
        const int mine = e;
        if (e == r.p1) e = r.end_out;
        for (int p = i; p < mine; ++p) f(p, v, png_token(p - s, e - s));
        i = mine;
    }
}

// exclusive scan of one value per thread over the workgroup (256 threads); *total: the sum
__device__ __forceinline__ unsigned int png_block_scan(unsigned int v, unsigned int* sh, unsigned int* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned int a = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const unsigned int incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

// ------------------------------------------------------------------------------------------------ stage C: codes
struct PngTree {
    uint32_t w[2 * PNG_LITLEN];                                // weights while merging, depths afterwards
    uint16_t parent[2 * PNG_LITLEN];
    uint16_t sorted[PNG_LITLEN];                               // used symbols by (count, symbol) ascending
};

// Length-limited code lengths of the symbols with freq > 0, a pure integer function of freq:
//   1. the used symbols sorted by (count, symbol) ascending;
//   2. Huffman's tree by the two-queue merge: leaves in that order, internal nodes in the order made; of two equal heads the leaf is taken;
//   3. depths above maxbits are cut to maxbits (*limited |= flag); while the Kraft sum exceeds 1, one leaf of the longest length below
//      maxbits moves one level down and takes a leaf of length maxbits with it as its sibling (each step lowers the sum by 2^-maxbits);
//   4. the lengths, longest first, go to the symbols in the order of 1.
// A single used symbol gets length 1.  Called by the whole workgroup; len[] is complete after the call.
__device__ void png_code_lengths(const uint32_t* freq, int nsym, int maxbits, uint8_t* len, PngTree& tr, int flag, int* limited) {
    const int t = threadIdx.x;
    for (int s = t; s < nsym; s += 256) {
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        int r = 0;
        for (int u = 0; u < nsym; ++u) {
            const uint32_t fu = freq[u];
            r += (fu && (fu < f || (fu == f && u < s))) ? 1 : 0;
        }
        tr.sorted[r] = (uint16_t)s;
    }
    __syncthreads();
    if (t == 0) {
        int m = 0;
        for (int s = 0; s < nsym; ++s) m += freq[s] ? 1 : 0;
        if (m == 1) len[tr.sorted[0]] = 1;
        if (m >= 2) {
            for (int i = 0; i < m; ++i) tr.w[i] = freq[tr.sorted[i]];
            int li = 0, ii = m, nn = m;
            for (int k = 0; k < m - 1; ++k) {
                int pick[2];
                for (int h = 0; h < 2; ++h) pick[h] = (li < m && (ii >= nn || tr.w[li] <= tr.w[ii])) ? li++ : ii++;
                tr.w[nn] = tr.w[pick[0]] + tr.w[pick[1]];
                tr.parent[pick[0]] = tr.parent[pick[1]] = (uint16_t)nn;
                ++nn;
            }
            tr.w[2 * m - 2] = 0;                                   // the root's depth
            for (int i = 2 * m - 3; i >= m; --i) tr.w[i] = tr.w[tr.parent[i]] + 1;
            int bl[16] = {0};
            for (int i = 0; i < m; ++i) {
                int d = (int)tr.w[tr.parent[i]] + 1;
                if (d > maxbits) {
                    d = maxbits;
                    *limited |= flag;
                }
                ++bl[d];
            }
            int excess = -(1 << maxbits);
            for (int d = 1; d <= maxbits; ++d) excess += bl[d] << (maxbits - d);
            for (; excess > 0; --excess) {
                int d = maxbits - 1;
                while (bl[d] == 0) --d;
                --bl[d];
                bl[d + 1] += 2;
                --bl[maxbits];
            }
            int i = 0;
            for (int d = maxbits; d >= 1; --d)
                for (int k = 0; k < bl[d]; ++k) len[tr.sorted[i++]] = (uint8_t)d;
        }
    }
    __syncthreads();
}

// The code lengths of the header as code-length symbols: the HLIT + 257 literal/length lengths and the one distance length as ONE
// sequence, cut into maximal runs of equal values.  A run of n zeros: while n >= 11 symbol 18 takes min(n, 138); then 3 .. 10 left: symbol
// 17; 1 .. 2 left: that many symbols 0.  A run of n lengths v > 0: v itself, then while n >= 3 symbol 16 takes min(n, 6), then the last
// 0 .. 2 as v.  One thread; returns the token count; *nlit: HLIT + 257; clfreq (when given) += the symbols' counts.
__device__ int png_header_tokens(const uint8_t* litlen, int dist, uint8_t* tsym, uint8_t* textra, uint32_t* clfreq, int* nlit_out) {
    int nlit = PNG_LITLEN;
    while (nlit > 257 && litlen[nlit - 1] == 0) --nlit;
    *nlit_out = nlit;
    const int total = nlit + 1;
    int nt = 0;
    auto get = [&](int i) -> int { return i < nlit ? litlen[i] : dist; };
    auto emit = [&](int sym, int extra) {
        tsym[nt] = (uint8_t)sym;
        textra[nt] = (uint8_t)extra;
        ++nt;
        if (clfreq) ++clfreq[sym];
    };
    for (int i = 0; i < total;) {
        const int v = get(i);
        int j = i + 1;
        while (j < total && get(j) == v) ++j;
        int n = j - i;
        if (v == 0) {
            while (n >= 11) {
                const int c = min(n, 138);
                emit(18, c - 11);
                n -= c;
            }
            if (n >= 3) {
                emit(17, n - 3);
                n = 0;
            }
            for (; n > 0; --n) emit(0, 0);
        } else {
            emit(v, 0);
            --n;
            while (n >= 3) {
                const int c = min(n, 6);
                emit(16, c - 3);
                n -= c;
            }
            for (; n > 0; --n) emit(v, 0);
        }
        i = j;
    }
    return nt;
}
__device__ __forceinline__ int png_cl_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }
__device__ __forceinline__ int png_hclen(const uint8_t* cl) {
    int h = PNG_CL;
    while (h > 4 && cl[PNG_CL_ORDER[h - 1]] == 0) --h;
    return h;
}

__global__ void __launch_bounds__(256) png_codes_kernel(const uint8_t* __restrict__ stream, size_t total, uint32_t* __restrict__ hist_out,
                                                        PngRec* __restrict__ rec, unsigned long long* __restrict__ size, uint32_t* __restrict__ adler) {
    __shared__ __attribute__((aligned(16))) uint8_t b[256 * PNG_SEG_PITCH];
    __shared__ uint32_t hist[PNG_HIST_ROW], clfreq[PNG_CL], adl[2];
    __shared__ int lastbrk[256], firstbrk[256];
    __shared__ PngTree tr;
    __shared__ uint8_t litlen[PNG_LITLEN], cl[PNG_CL], tsym[PNG_MAX_TOK], textra[PNG_MAX_TOK];
    __shared__ int flags, kind;
    const int t = threadIdx.x, c = blockIdx.x;
    const size_t at = (size_t)c * PNG_CHUNK;
    const int n = (int)min((size_t)PNG_CHUNK, total - at);
    for (int e = t; e < PNG_HIST_ROW; e += 256) hist[e] = e == 256 ? 1u : 0u;      // the end-of-block symbol is always in the code
    if (t < PNG_CL) clfreq[t] = 0;
    if (t < 2) adl[t] = 0;
    if (t == 0) flags = 0;
    png_load_chunk(stream + at, n, b);
    __syncthreads();
    const PngRuns r = png_runs(b, n, lastbrk, firstbrk);
    uint32_t a = 0, bs = 0, ntok = 0, nmatch = 0;
    png_walk(b, r, [&](int p, int v, int tok) {
        a += (uint32_t)v;
        bs += (uint32_t)(n - p) * (uint32_t)v;
        if (tok == 1) {
            atomicAdd(&hist[v], 1u);
            ++ntok;
        } else if (tok) {
            atomicAdd(&hist[257 + PNG_LEN.sym[tok]], 1u);
            ++ntok;
            ++nmatch;
        }
    });
    atomicAdd(&adl[0], a);
    atomicAdd(&adl[1], bs % 65521u);
    if (nmatch) atomicAdd(&hist[286], nmatch);
    if (ntok) atomicAdd(&hist[287], ntok);
    __syncthreads();
    for (int e = t; e < PNG_HIST_ROW; e += 256) hist_out[(size_t)c * PNG_HIST_ROW + e] = hist[e];
    png_code_lengths(hist, PNG_LITLEN, 15, litlen, tr, PNG_LIMIT15, &flags);
    const int dist = hist[286] ? 1 : 0;
    if (t == 0) {
        int nlit;
        png_header_tokens(litlen, dist, tsym, textra, clfreq, &nlit);
    }
    __syncthreads();
    png_code_lengths(clfreq, PNG_CL, 7, cl, tr, PNG_LIMIT7, &flags);
    if (t == 0) {
        unsigned long long bits = 3 + 5 + 5 + 4 + 3 * (unsigned long long)png_hclen(cl);
        for (int s = 0; s < PNG_CL; ++s) bits += (unsigned long long)clfreq[s] * (unsigned)(cl[s] + png_cl_extra_bits(s));
        for (int s = 0; s < PNG_LITLEN; ++s) bits += (unsigned long long)hist[s] * (unsigned)(litlen[s] + (s >= 257 ? PNG_LEN.extra[s - 257] : 0));
        bits += hist[286];                                     // the one-bit distance code of every match
        const unsigned long long dyn = (bits + 3 + 7) / 8 + 4, stored = 5 + (unsigned long long)n;
        kind = dyn >= stored ? PNG_STORED : PNG_DYNAMIC;
        size[c] = dyn >= stored ? stored : dyn;
        adler[2 * c] = adl[0] % 65521u;
        adler[2 * c + 1] = adl[1] % 65521u;
    }
    __syncthreads();
    uint8_t* o = (uint8_t*)&rec[c];
    for (int e = t; e < PNG_REC; e += 256) {
        uint8_t v = 0;
        if (e == 0) v = (uint8_t)kind;
        else if (e == 1) v = (uint8_t)flags;
        else if (e < 2 + PNG_LITLEN) v = litlen[e - 2];
        else if (e == 2 + PNG_LITLEN) v = (uint8_t)dist;
        else if (e < 3 + PNG_LITLEN + PNG_CL) v = cl[e - 3 - PNG_LITLEN];
        o[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------ stage D: packing
// deflate's bit order: values from the least significant bit on; Huffman codes are stored bit-reversed so that they go through put() too
struct PngBits {
    uint32_t* w;
    unsigned long long acc = 0;
    int nacc, word;
    __device__ PngBits(uint32_t* words, unsigned int bit) : w(words), nacc((int)(bit & 31)), word((int)(bit >> 5)) {}
    __device__ __forceinline__ void put(uint32_t v, int nb) {
        acc |= (unsigned long long)v << nacc;
        nacc += nb;
        if (nacc >= 32) {
            atomicOr(&w[word++], (uint32_t)acc);
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0) atomicOr(&w[word], (uint32_t)acc);
    }
};
__device__ __forceinline__ uint32_t png_rev(uint32_t code, int len) { return len ? __brev(code) >> (32 - len) : 0u; }

// canonical codes (RFC 1951 3.2.2) of nsym lengths, bit-reversed; next[]: 16 ints of scratch.  Whole workgroup; contains barriers.
__device__ void png_codes_of(const uint8_t* len, int nsym, uint16_t* code, int* next) {
    const int t = threadIdx.x;
    if (t == 0) {
        int count[16] = {0};
        for (int s = 0; s < nsym; ++s) ++count[len[s]];
        count[0] = 0;
        int c = 0;
        next[0] = 0;
        for (int l = 1; l < 16; ++l) {
            c = (c + count[l - 1]) << 1;
            next[l] = c;
        }
    }
    __syncthreads();
    for (int s = t; s < nsym; s += 256) {
        const int l = len[s];
        int k = 0;
        for (int u = 0; u < s; ++u) k += len[u] == l ? 1 : 0;
        code[s] = (uint16_t)png_rev((uint32_t)(next[l] + k), l);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) png_pack_kernel(const uint8_t* __restrict__ stream, size_t total, const PngRec* __restrict__ rec,
                                                       const unsigned long long* __restrict__ off, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t b[256 * PNG_SEG_PITCH];
    __shared__ uint32_t words[PNG_OUT_WORDS];
    __shared__ unsigned int sh[256];
    __shared__ int lastbrk[256], firstbrk[256], next[16];
    __shared__ uint8_t litlen[PNG_LITLEN], cl[PNG_CL], tsym[PNG_MAX_TOK], textra[PNG_MAX_TOK];
    __shared__ uint16_t lcode[PNG_LITLEN], ccode[PNG_CL];
    __shared__ unsigned int hdr_bits;
    const int t = threadIdx.x, c = blockIdx.x;
    const size_t at = (size_t)c * PNG_CHUNK;
    const int n = (int)min((size_t)PNG_CHUNK, total - at);
    const uint8_t* src = stream + at;
    uint8_t* dst = out + off[c];
    const int bytes = (int)(off[c + 1] - off[c]);
    const uint8_t* r8 = (const uint8_t*)&rec[c];
    if (r8[0] == PNG_STORED) {                                 // BFINAL 0, BTYPE 00, LEN, ~LEN, the bytes
        if (t == 0) {
            dst[0] = 0;
            dst[1] = (uint8_t)(n & 255);
            dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)(~n & 255);
            dst[4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int e = t; e < n; e += 256) dst[5 + e] = src[e];
        return;
    }
    for (int e = t; e < PNG_OUT_WORDS; e += 256) words[e] = 0;
    for (int e = t; e < PNG_LITLEN; e += 256) litlen[e] = r8[2 + e];
    if (t < PNG_CL) cl[t] = r8[3 + PNG_LITLEN + t];
    const int dist = r8[2 + PNG_LITLEN];
    png_load_chunk(src, n, b);
    __syncthreads();
    png_codes_of(cl, PNG_CL, ccode, next);
    png_codes_of(litlen, PNG_LITLEN, lcode, next);
    if (t == 0) {                                              // the block header
        int nlit;
        const int nt = png_header_tokens(litlen, dist, tsym, textra, nullptr, &nlit), hclen = png_hclen(cl);
        PngBits o(words, 0);
        o.put(0, 1);                                           // BFINAL
        o.put(2, 2);                                           // BTYPE: dynamic
        o.put((uint32_t)(nlit - 257), 5);
        o.put(0, 5);                                           // HDIST: one distance code
        o.put((uint32_t)(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) o.put(cl[PNG_CL_ORDER[k]], 3);
        for (int k = 0; k < nt; ++k) {
            const int s = tsym[k];
            o.put(ccode[s], cl[s]);
            if (s >= 16) o.put(textra[k], png_cl_extra_bits(s));
        }
        hdr_bits = (unsigned int)o.word * 32u + (unsigned int)o.nacc;
        o.finish();
    }
    const PngRuns r = png_runs(b, n, lastbrk, firstbrk);      // (its barrier publishes hdr_bits)
    unsigned int mine = 0;
    png_walk(b, r, [&](int p, int v, int tok) {
        if (tok == 1) mine += litlen[v];
        else if (tok) mine += litlen[257 + PNG_LEN.sym[tok]] + PNG_LEN.extra[PNG_LEN.sym[tok]] + 1u;
    });
    unsigned int body;
    const unsigned int before = png_block_scan(mine, sh, &body);
    PngBits o(words, hdr_bits + before);
    png_walk(b, r, [&](int p, int v, int tok) {
        if (tok == 1) {
            o.put(lcode[v], litlen[v]);
        } else if (tok) {
            const int s = PNG_LEN.sym[tok];
            o.put(lcode[257 + s], litlen[257 + s]);
            if (PNG_LEN.extra[s]) o.put((uint32_t)(tok - PNG_LEN.base[s]), PNG_LEN.extra[s]);
            o.put(0, 1);                                       // distance symbol 0: distance 1
        }
    });
    o.finish();
    if (t == 0) {                                              // end of block, then the empty stored block that aligns the stream: 000, pad, 00 00 FF FF
        const unsigned int endbit = hdr_bits + body;
        PngBits e(words, endbit);
        e.put(lcode[256], litlen[256]);
        e.finish();
        const unsigned int q = (endbit + litlen[256] + 3 + 7) / 8;
        atomicOr(&words[(q + 2) >> 2], 0xFFu << (8 * ((q + 2) & 3)));
        atomicOr(&words[(q + 3) >> 2], 0xFFu << (8 * ((q + 3) & 3)));
    }
    __syncthreads();
    for (int e = t; e < bytes; e += 256) dst[e] = (uint8_t)(words[e >> 2] >> (8 * (e & 3)));
}

}  // namespace

hipError_t launch_png_filter(const uint8_t* src, size_t pitch, int layout, int H, int W, uint8_t* stream, hipStream_t s) {
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)H), dim3(256), 0, s, src, pitch, layout, H, W, stream);
    return hipGetLastError();
}
hipError_t launch_png_codes(const uint8_t* stream, size_t n, int chunks, uint32_t* hist, PngRec* rec, unsigned long long* size, uint32_t* adler,
                            hipStream_t s) {
    if (chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(png_codes_kernel, dim3((unsigned)chunks), dim3(256), 0, s, stream, n, hist, rec, size, adler);
    return hipGetLastError();
}
hipError_t launch_png_pack(const uint8_t* stream, size_t n, int chunks, const PngRec* rec, const unsigned long long* off, uint8_t* out, hipStream_t s) {
    if (chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)chunks), dim3(256), 0, s, stream, n, rec, off, out);
    return hipGetLastError();
}
