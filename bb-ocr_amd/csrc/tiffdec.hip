// The device TIFF decoder (bbocr_tiff_decode): three launches over a batch, whatever mix of codecs and shapes it holds (tiffdec.h).
//   td_strips     one wavefront per strip, over all files: the strip's stored bytes -> its rows of the file's stream.  Raw strips are
//                 COPIED (the stream is then one piece whatever order and gaps the file keeps its strips in, and the stage entry point can
//                 hand it out), in pieces of 64 KB that tiffdec.cpp makes strips of their own; PackBits: every lane reads the same header
//                 byte and the lanes share out the run; LZW: tiff_codecs.h's match copy, the table of (offset, length) pairs in LDS --
//                 every lane runs the code loop on the same values and the lanes share out the copy; Deflate: png_inflate.h under
//                 pngdec.hip's wave policy, the zlib header and the Adler-32 checked per strip.  LDS per wavefront: 32 KB when the batch
//                 holds an LZW strip (five wavefronts on a CU's 160 KB), sizeof(PngiTables) when it holds Deflate strips only, none
//                 otherwise.  CCITT (TD_FAX, batches of bbocr_tiff_decode_fax only): tiff_fax.h under the wave policy below -- a code
//                 is resolved by one ballot over the lanes' code words, a row is kept as its changing elements in LDS and rendered by
//                 all lanes; fax_lds_bytes(the batch's widest CCITT file) of LDS, whichever of the sizes above is larger.
//   td_predictor  predictor 2, in place: one wavefront per row, a prefix sum modulo 256 per sample position -- 64 pixels per step, a wave
//                 scan, the carry handed from segment to segment.
//   td_output     fully parallel: both planes by reader.decode_file's rule.
// A strip writes its own status word and ORs it into its file's; a file whose word is not 0 is skipped by the later launches.  No launch
// writes outside the file's stream or its destinations' rows.
#include "tiffdec.h"
#include "wave_copy.h"

namespace {

constexpr int kWave = 64;

using TiffcWave = WaveCopy;                               // a workgroup of ONE wavefront: wave_copy.h's output policy

struct PngiWaveT {                                        // pngdec.hip's policy for pngi_inflate
    __device__ static bool leader() { return threadIdx.x == 0; }
    __device__ static void barrier() { __syncthreads(); }
    __device__ static void put(uint8_t* out, size_t o, uint8_t v) {
        if (threadIdx.x == 0) out[o] = v;
    }
    __device__ static void copy_in(uint8_t* out, size_t o, const uint8_t* in, size_t n) {
        for (size_t i = threadIdx.x; i < n; i += kWave) out[o + i] = in[i];
    }
    __device__ static void copy_match(uint8_t* out, size_t o, uint32_t dist, int len, size_t& synced) {
        if (o - dist + (dist < (uint32_t)len ? dist : (uint32_t)len) > synced) {
            drain_and_sync();
            synced = o;
        }
        const uint8_t* from = out + o - dist;
        for (int i = (int)threadIdx.x; i < len; i += kWave) out[o + i] = from[dist >= (uint32_t)len ? (uint32_t)i : (uint32_t)i % dist];
    }
};

struct FaxWave {                                          // tiff_fax.h's policy for a workgroup of ONE wavefront
    struct Words {                                        // lane l: words l and 64 + l of both colours
        uint32_t key[2][2];                               // the word left-aligned in 16 bits | the mask of its length << 16
        uint32_t meta[2][2];                              // length | run << 8; 0: no word (lanes 40 .. 63 of the second set)
    };
    __device__ static void load(Words& w) {
        for (int c = 0; c < 2; ++c)
            for (int s = 0; s < 2; ++s) {
                const int i = 64 * s + (int)threadIdx.x;
                w.key[c][s] = w.meta[c][s] = 0;
                if (i < FAX_WORDS) {
                    const FaxWord f = fax_word(c, i);
                    w.key[c][s] = ((uint32_t)f.code << (16 - f.len)) | ((0xFFFFu << (16 - f.len)) & 0xFFFFu) << 16;
                    w.meta[c][s] = (uint32_t)f.len | (uint32_t)fax_word_run(i) << 8;
                }
            }
    }
    __device__ static uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ static void sync() { __syncthreads(); }
    __device__ static bool resolve(const Words& w, int colour, uint32_t head16, int& len, int& run) {
        const uint32_t k0 = colour ? w.key[1][0] : w.key[0][0], k1 = colour ? w.key[1][1] : w.key[0][1];
        const uint32_t m0 = colour ? w.meta[1][0] : w.meta[0][0], m1 = colour ? w.meta[1][1] : w.meta[0][1];
        const unsigned long long hit0 = __ballot(m0 && !((head16 ^ k0) & (k0 >> 16)));
        const unsigned long long hit1 = __ballot(m1 && !((head16 ^ k1) & (k1 >> 16)));
        if (!(hit0 | hit1)) return false;                 // (the words are prefix-free: at most one lane of one set matches)
        const int lane = hit0 ? __ffsll(hit0) - 1 : __ffsll(hit1) - 1;
        const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)(hit0 ? m0 : m1), lane);
        len = (int)(m & 255u);
        run = (int)(m >> 8);
        return true;
    }
    __device__ static void put(uint16_t* line, int i, int v) {
        if (threadIdx.x == 0) line[i] = (uint16_t)v;
    }
    __device__ static int get(const uint16_t* line, int i) { return __builtin_amdgcn_readfirstlane((int)line[i]); }
    // the n changing elements -> the row's bytes: toggles in the bitmap, a prefix XOR over it, the words stored byte by byte
    __device__ static void render(const uint16_t* cur, int n, int W, uint32_t* bitmap, uint8_t* out, size_t row_bytes) {
        const int lane = (int)threadIdx.x, words = (W + 31) / 32;
        for (int i = lane; i < words; i += kWave) bitmap[i] = 0;
        __syncthreads();
        for (int i = lane; i < n; i += kWave) {
            const int c = cur[i];
            if (c < W) atomicXor(&bitmap[c >> 5], 0x80000000u >> (c & 31));
        }
        __syncthreads();
        uint32_t carry = 0;                               // the colour at the start of this step's words
        for (int base = 0; base < words; base += kWave) {
            const int i = base + lane;
            const uint32_t t = i < words ? bitmap[i] : 0;
            uint32_t v = t;
            v ^= v >> 1;
            v ^= v >> 2;
            v ^= v >> 4;
            v ^= v >> 8;
            v ^= v >> 16;                                 // bit j from the top = the XOR of the toggles 0 .. j
            const unsigned long long odd = __ballot(__popc(t) & 1);
            if ((__popcll(odd & ((1ull << lane) - 1)) & 1) ^ carry) v = ~v;
            carry ^= (uint32_t)__popcll(odd) & 1u;
            if (i == words - 1 && (W & 31)) v &= ~0u << (32 - (W & 31));      // the bits behind the width are 0
            if (i < words)
                for (int k = 0; k < 4; ++k)
                    if ((size_t)(4 * i + k) < row_bytes) out[4 * i + k] = (uint8_t)(v >> (24 - 8 * k));
        }
        __syncthreads();                                  // (the bitmap is free for the next row)
    }
};

__device__ inline int strip_fax(const TdStrip& s, unsigned char* lds) {
    const int W = s.fax_width;
    const size_t row_bytes = ((size_t)W + 7) / 8;
    uint16_t* line0 = (uint16_t*)lds;
    uint16_t* line1 = (uint16_t*)(lds + fax_line_bytes(W));
    uint32_t* bitmap = (uint32_t*)(lds + 2 * fax_line_bytes(W));
    return fax_decode_strip<FaxWave>(s.src, s.src_bytes, s.dst, W, (int)(s.need / row_bytes), s.fax_mode & 255, (s.fax_mode >> 8) & 255, s.fax_mode >> 16,
                                     line0, line1, bitmap);
}

__device__ inline int strip_deflate(const TdStrip& s, PngiTables& T) {
    if (!tiffc_zlib_header_ok(s.src, s.src_bytes)) return PNGI_ERR_ZLIB;
    size_t produced = 0, end = 0;
    const size_t zn = (size_t)s.src_bytes - 2;
    int err = pngi_inflate<PngiWaveT>(s.src + 2, zn, s.dst, (size_t)s.need, T, &produced, &end);
    if (!err && produced != (size_t)s.need) err = PNGI_ERR_SHORT;
    if (!err && zn - end < 4) err = PNGI_ERR_INPUT;
    if (err) return err;
    drain_and_sync();
    // Adler-32 in pieces of 2048 bytes, as pd_inflate sums it
    uint32_t a = 1, b = 0;
    const size_t n = s.need;
    for (size_t base = 0; base < n; base += 2048) {
        const uint32_t m = (uint32_t)(n - base < 2048 ? n - base : 2048);
        uint32_t A = 0, B = 0;
        for (uint32_t i = threadIdx.x; i < m; i += kWave) {
            const uint32_t c = s.dst[base + i];
            A += c;
            B += (m - i) * c;
        }
        for (int k = 32; k > 0; k >>= 1) {
            A += __shfl_xor(A, k);
            B += __shfl_xor(B, k);
        }
        b = (uint32_t)(((unsigned long long)b + (unsigned long long)m * a + B) % 65521u);
        a = (a + A) % 65521u;
    }
    return ((b << 16) | a) != pngi_be32(s.src + 2 + end) ? PNGI_ERR_ADLER : 0;
}

__global__ __launch_bounds__(kWave) void td_strips(const TdStrip* strips) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const TdStrip& s = strips[blockIdx.x];
    int err = 0;
    if (s.codec == TD_RAW) {
        if (s.src_bytes < s.need) err = TIFFC_ERR_INPUT;
        else TiffcWave::copy_in(s.dst, 0, s.src, s.need);
    } else if (s.codec == TD_PACKBITS) {
        err = tiffc_packbits<TiffcWave>(s.src, s.src_bytes, s.dst, s.need);
    } else if (s.codec == TD_LZW) {
        err = tiffc_lzw<TiffcWave>(s.src, s.src_bytes, s.dst, s.need, (TiffcEntry*)lds);
    } else if (s.codec == TD_FAX) {
        err = strip_fax(s, lds);
    } else {
        err = strip_deflate(s, *(PngiTables*)lds);
    }
    if (threadIdx.x == 0) {
        *s.status = err;
        if (err) atomicOr(s.file_status, err);
    }
}

__global__ __launch_bounds__(kWave) void td_predictor(const TdDesc* descs) {
    const TdDesc& d = descs[blockIdx.y];
    if (d.predictor != 2 || *d.status) return;
    const int lane = (int)threadIdx.x, S = d.samples;
    for (int y = (int)blockIdx.x; y < d.H; y += (int)gridDim.x) {
        uint8_t* row = d.stream + (size_t)y * (size_t)d.row_bytes;
        uint32_t carry[4] = {0, 0, 0, 0};
        for (int base = 0; base < d.W; base += kWave) {
            const int x = base + lane;
            uint8_t* px = row + (size_t)x * S;
            for (int k = 0; k < S; ++k) {
                uint32_t v = x < d.W ? px[k] : 0;
                for (int step = 1; step < kWave; step <<= 1) {                  // the wave's inclusive scan
                    const uint32_t up = __shfl_up(v, step);
                    if (lane >= step) v += up;
                }
                v += carry[k];
                if (x < d.W) px[k] = (uint8_t)v;
                carry[k] = __shfl(v, kWave - 1) & 255u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void td_output(const TdDesc* descs) {
    const TdDesc& d = descs[blockIdx.y];
    if (*d.status) return;
    const size_t total = (size_t)d.W * (size_t)d.H;
    const int phot = d.photometric, S = d.samples;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t y = i / (size_t)d.W, x = i - y * (size_t)d.W;
        const uint8_t* row = d.stream + y * (size_t)d.row_bytes;
        int r, g, b, gray;
        if (phot == 2) {
            const uint8_t* p = row + x * (size_t)S;                         // a fourth sample is dropped
            r = p[0], g = p[1], b = p[2];
            gray = (9797 * r + 19234 * g + 3737 * b) >> 15;
        } else {
            int v = d.bits == 8 ? row[x] : ((row[x >> 3] >> (7 - (int)(x & 7))) & 1) * 255;
            if (phot == 3) {
                r = d.palette[3 * v], g = d.palette[3 * v + 1], b = d.palette[3 * v + 2];
                gray = (9797 * r + 19234 * g + 3737 * b) >> 15;
            } else {
                if (phot == 0) v = 255 - v;
                r = g = b = gray = v;
            }
        }
        uint8_t* o = d.rgb + y * (size_t)d.pitch_rgb + 3 * x;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
        d.gray[y * (size_t)d.pitch_gray + x] = (uint8_t)gray;
    }
}

}  // namespace

size_t td_strips_lds(bool any_lzw, bool any_deflate, int fax_width) {
    const size_t plain = any_lzw ? sizeof(TiffcEntry) * (size_t)TIFFC_LZW_ENTRIES : (any_deflate ? sizeof(PngiTables) : 0);
    const size_t fax = fax_width > 0 ? fax_lds_bytes(fax_width) : 0;
    return plain > fax ? plain : fax;
}

hipError_t launch_td_strips(const TdStrip* s, int n, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL(td_strips, dim3((unsigned)n), dim3(kWave), lds_bytes, st, s);
    return hipGetLastError();
}

hipError_t launch_td_predictor(const TdDesc* d, int n, int max_rows, hipStream_t st) {
    for (int at = 0; at < n; at += 32768) {
        const int m = n - at < 32768 ? n - at : 32768;
        hipLaunchKernelGGL(td_predictor, dim3((unsigned)(max_rows < 1 ? 1 : (max_rows > 16384 ? 16384 : max_rows)), (unsigned)m), dim3(kWave), 0, st, d + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_td_output(const TdDesc* d, int n, unsigned long long max_pixels, hipStream_t st) {
    const unsigned long long blocks = (max_pixels + 1023) / 1024;        // four pixels per thread, more in the largest files
    for (int at = 0; at < n; at += 32768) {                              // the grid's second dimension holds at most 65535 files
        const int m = n - at < 32768 ? n - at : 32768;
        hipLaunchKernelGGL(td_output, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)), (unsigned)m), dim3(256), 0, st, d + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
