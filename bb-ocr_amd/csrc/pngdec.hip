// The device PNG decoder (bbocr_png_decode): three launches over the files of a batch, each file described by a PdDesc (pngdec.h).
//   pd_inflate   one wavefront per file: png_inflate.h's decoder under the wave policy below -- every lane runs the symbol loop on the
//                same values (uniform loads of the stream, the tables in LDS written by lane 0), the lanes share out the copies of a
//                match and of a stored block; then the Adler-32 of the output, summed by the wave, against the trailer.
//   pd_unfilter  one workgroup per file, in place: lanes = rows of a band of PD_UNFILTER_THREADS rows, each lane one pixel behind the lane
//                above, so Raw(x - bpp) stays in registers and Prior(x) / Prior(x - bpp) come from the lane above through LDS.
//   pd_output    fully parallel: both planes by reader.decode_file's rule.
// A file whose status word is not 0 is skipped by the later stages; no stage writes outside the file's scratch or its destinations' rows.
#include "pngdec.h"
#include "wave_copy.h"

namespace {

constexpr int kWave = 64;

struct PngiWave {                                         // a workgroup of ONE wavefront
    __device__ static bool leader() { return threadIdx.x == 0; }
    __device__ static void barrier() { __syncthreads(); }
    __device__ static void put(uint8_t* out, size_t o, uint8_t v) {
        if (threadIdx.x == 0) out[o] = v;
    }
    __device__ static void copy_in(uint8_t* out, size_t o, const uint8_t* in, size_t n) {
        for (size_t i = threadIdx.x; i < n; i += kWave) out[o + i] = in[i];
    }
    // out[o + i] = out[o + i - dist]: with dist < len the bytes repeat with period dist, so every lane reads behind o, from bytes the
    // barrier has made visible, and no lane waits for another's store
    // `synced`: the output up to there was stored before the last drain; only a match that reads behind it waits for the stores again
    __device__ static void copy_match(uint8_t* out, size_t o, uint32_t dist, int len, size_t& synced) {
        if (o - dist + (dist < (uint32_t)len ? dist : (uint32_t)len) > synced) {
            drain_and_sync();
            synced = o;
        }
        const uint8_t* from = out + o - dist;
        for (int i = (int)threadIdx.x; i < len; i += kWave) out[o + i] = from[dist >= (uint32_t)len ? (uint32_t)i : (uint32_t)i % dist];
    }
};

__global__ __launch_bounds__(kWave) void pd_inflate(const PdDesc* descs) {
    __shared__ PngiTables T;
    const PdDesc& d = descs[blockIdx.x];
    size_t produced = 0, end = 0;
    int err = pngi_inflate<PngiWave>(d.z + 2, (size_t)d.z_bytes - 2, d.raw, (size_t)d.raw_bytes, T, &produced, &end);   // (the plan has read the header)
    if (!err && produced != (size_t)d.raw_bytes) err = PNGI_ERR_SHORT;
    if (!err && (size_t)d.z_bytes - 2 - end < 4) err = PNGI_ERR_INPUT;
    if (!err) {
        drain_and_sync();
        // Adler-32 in pieces of 2048 bytes: a piece of m bytes with A = sum c_i, B = sum (m - i) c_i takes (a, b) to (a + A, b + m a + B)
        uint32_t a = 1, b = 0;
        const size_t n = d.raw_bytes;
        for (size_t base = 0; base < n; base += 2048) {
            const uint32_t m = (uint32_t)(n - base < 2048 ? n - base : 2048);
            uint32_t A = 0, B = 0;                        // per lane at most 32 * 255 and 32 * 2048 * 255; the wave's sums stay below 2^31
            for (uint32_t i = threadIdx.x; i < m; i += kWave) {
                const uint32_t c = d.raw[base + i];
                A += c;
                B += (m - i) * c;
            }
            for (int s = 32; s > 0; s >>= 1) {
                A += __shfl_xor(A, s);
                B += __shfl_xor(B, s);
            }
            b = (uint32_t)(((unsigned long long)b + (unsigned long long)m * a + B) % 65521u);
            a = (a + A) % 65521u;
        }
        if (((b << 16) | a) != pngi_be32(d.z + 2 + end)) err = PNGI_ERR_ADLER;
    }
    if (err && threadIdx.x == 0) atomicOr(d.status, err);
}

__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ __launch_bounds__(PD_UNFILTER_THREADS) void pd_unfilter(const PdDesc* descs) {
    __shared__ uint32_t line[2][PD_UNFILTER_THREADS];     // per step parity: the pixel each lane has just finished (bpp <= 4 bytes)
    const PdDesc& d = descs[blockIdx.x];
    if (*d.status) return;                                // (written by the launch before: uniform over the workgroup)
    const int t = (int)threadIdx.x, bpp = d.bpp;
    const size_t stride = (size_t)d.row_bytes + 1;
    const int npx = (d.row_bytes + bpp - 1) / bpp;        // whole pixels: row_bytes is a multiple of bpp
    bool bad = false;
    for (int band = 0; band < d.H; band += PD_UNFILTER_THREADS) {
        const int y = band + t;
        const bool live = y < d.H;
        uint8_t* row = d.raw + (size_t)(live ? y : 0) * stride;
        int f = live ? row[0] : 0;
        if (f > 4) {
            bad = true;
            f = 0;
        }
        const uint8_t* above = (t == 0 && y > 0 && live) ? row - stride + 1 : nullptr;   // the band's first row: the row above is final, in memory
        uint32_t left = 0, upleft = 0;
        const int rows = d.H - band < PD_UNFILTER_THREADS ? d.H - band : PD_UNFILTER_THREADS;
        const int steps = npx + rows - 1;                 // the band's last row starts rows - 1 steps behind its first
        for (int s = 0; s < steps; ++s) {
            const int x = s - t;
            uint32_t cur = 0;
            if (live && x >= 0 && x < npx) {
                uint32_t up = 0;
                if (t > 0) up = line[(s + 1) & 1][t - 1];                  // what the lane above finished in step s - 1: its pixel x
                else if (above)
                    for (int k = 0; k < bpp; ++k) up |= (uint32_t)above[(size_t)x * bpp + k] << (8 * k);
                uint8_t* px = row + 1 + (size_t)x * bpp;
                for (int k = 0; k < bpp; ++k) {
                    const int a = (left >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (upleft >> (8 * k)) & 255;
                    const int pred = f == 0 ? 0 : (f == 1 ? a : (f == 2 ? b : (f == 3 ? (a + b) >> 1 : paeth(a, b, c))));
                    const uint32_t v = (uint32_t)(px[k] + pred) & 255u;
                    if (f) px[k] = (uint8_t)v;
                    cur |= v << (8 * k);
                }
                left = cur;
                upleft = up;
                line[s & 1][t] = cur;
            }
            __syncthreads();
        }
        drain_and_sync();                                 // the band's last row is in memory before the next band's first lane reads it
    }
    if (bad) atomicOr(d.status, PD_ERR_FILTER);
}

__global__ __launch_bounds__(256) void pd_output(const PdDesc* descs) {
    const PdDesc& d = descs[blockIdx.y];
    if (*d.status) return;
    const size_t stride = (size_t)d.row_bytes + 1, total = (size_t)d.W * (size_t)d.H;
    const int depth = d.depth, ct = d.color_type;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t y = i / (size_t)d.W, x = i - y * (size_t)d.W;
        const uint8_t* row = d.raw + y * stride + 1;
        int r, g, b, gray = -1;
        if (ct == 2 || ct == 6) {
            const uint8_t* p = row + x * (size_t)d.channels;
            r = p[0], g = p[1], b = p[2];
        } else {
            int v;
            if (depth == 8) v = row[x * (size_t)d.channels];
            else {
                const size_t bit = x * (size_t)depth;
                v = (row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1 << depth) - 1);
            }
            if (ct == 3) {
                if (v >= d.palette_entries) {
                    bad = true;
                    v = 0;
                }
                r = d.palette[3 * v], g = d.palette[3 * v + 1], b = d.palette[3 * v + 2];
            } else {
                r = g = b = gray = v * (depth == 1 ? 255 : (depth == 2 ? 85 : (depth == 4 ? 17 : 1)));
            }
        }
        if (gray < 0) gray = (9797 * r + 19234 * g + 3737 * b) >> 15;
        uint8_t* o = d.rgb + y * (size_t)d.pitch_rgb + 3 * x;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
        d.gray[y * (size_t)d.pitch_gray + x] = (uint8_t)gray;
    }
    if (bad) atomicOr(d.status, PD_ERR_PALETTE);
}

}  // namespace

hipError_t launch_pd_inflate(const PdDesc* d, int n, hipStream_t s) {
    hipLaunchKernelGGL(pd_inflate, dim3((unsigned)n), dim3(kWave), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_pd_unfilter(const PdDesc* d, int n, hipStream_t s) {
    hipLaunchKernelGGL(pd_unfilter, dim3((unsigned)n), dim3(PD_UNFILTER_THREADS), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_pd_output(const PdDesc* d, int n, unsigned long long max_pixels, hipStream_t s) {
    const unsigned long long blocks = (max_pixels + 1023) / 1024;        // four pixels per thread, more in the largest files
    for (int at = 0; at < n; at += 32768) {                              // the grid's second dimension holds at most 65535 files
        const int m = n - at < 32768 ? n - at : 32768;
        hipLaunchKernelGGL(pd_output, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)), (unsigned)m), dim3(256), 0, s, d + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
