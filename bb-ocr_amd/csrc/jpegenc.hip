// The extractor's model-input JPEG (enhanced_extractor.py:399-411: Image.save(format="JPEG", quality=q)) written on the device: a
// baseline JFIF scan -- SOF0, one interleaved scan, no restart interval, the Annex K Huffman tables, YCbCr 4:2:0 or one component --
// byte for byte the one Pillow 12 / libjpeg-turbo produces (tests/jpeg_encode_ref.py states each step).
//   je_coef      one 16x16 pixel square per 64-lane workgroup: th_jpeg_mcu's colour conversion, edge replication, h2v2 downsampling,
//                jfdctint.c and quantisation; the coefficients stay, int16 in zig-zag order, blocks in MCU order.  Y blocks wholly beyond
//                ceil(W/8) x ceil(H/8) are jccoefct.c's dummy blocks: no AC terms, the DC term of the block before them in the MCU
//   je_sizes     one block per lane: jchuff.c's bit count (je_block_bits), scanned inside the tile of JE_TILE blocks
//   je_scan      exclusive scan of the tile sums by one workgroup (also of the stuffing counts)
//   je_pack      one block per lane: its bits at its offset (je_block_pack); words shared with a neighbour are OR-ed in atomically
//   je_ff_count  0xFF bytes per tile of JE_STUFF_TILE scan bytes
//   je_stuff     every byte to its place behind the zero bytes stuffed in front of it
#include "common.h"
#include "kernels.h"
#include "jpeg_dev.h"

namespace {

__device__ const JeHuff JE_HUFF = je_std_huff();
__device__ const unsigned char JE_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// (R, G, B) of pixel (y, x) as Pillow's convert("RGB") of the page holds it; YCbCr pages through jdcolor.c
__device__ __forceinline__ void je_rgb(const uint8_t* __restrict__ src, size_t pitch, int layout, int y, int x, int* c) {
    const uint8_t* p = src + (size_t)y * pitch + (size_t)x * page_px_bytes(layout);
    switch (layout) {
        case PAGE_GRAY: c[0] = c[1] = c[2] = p[0]; break;
        case PAGE_BGR: c[0] = p[2]; c[1] = p[1]; c[2] = p[0]; break;
        case PAGE_RGB: c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; break;
        default: {
            uint8_t o[3];
            jpeg_ycc_to_rgb(p[0], p[1], p[2], o);
            c[0] = o[0]; c[1] = o[1]; c[2] = o[2];
        }
    }
}

// Blocks 0-3 hold Y (2x2), 4 Cb, 5 Cr.  A gray page has Cb = Cr = 128 exactly: its chroma blocks (components == 3) are all zero and
// are written as such.  components == 1: the four Y blocks go to their raster places among ceil(H/8) x ceil(W/8), those beyond are dropped.
__global__ void __launch_bounds__(64) je_coef_kernel(const uint8_t* __restrict__ src, size_t pitch, int layout, int components, int H, int W, ThQuant q,
                                                     short* __restrict__ coef) {
    __shared__ int blk[6][64];
    const int t = threadIdx.x, mx = blockIdx.x, my = blockIdx.y;
    const bool colour = layout != PAGE_GRAY;
    const int nblk = colour ? 6 : 4;
    for (int p = 0; p < 4; ++p) {                              // 256 pixels, edge-replicated beyond the page (expand_right / bottom_edge)
        const int id = t + 64 * p, py = id >> 4, px = id & 15;
        int c[3];
        je_rgb(src, pitch, layout, min(my * 16 + py, H - 1), min(mx * 16 + px, W - 1), c);
        blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = (colour ? th_y(c[0], c[1], c[2]) : c[0]) - 128;
    }
    if (colour) {                                              // h2v2_downsample, as th_jpeg_mcu_kernel
        const int cy = t >> 3, cx = t & 7, kc = mx * 8 + cx;
        const int kr = min(my * 8 + cy, (H + 1) / 2 - 1);
        const int ys[2] = {2 * kr, min(2 * kr + 1, H - 1)}, xs[2] = {min(2 * kc, W - 1), min(2 * kc + 1, W - 1)};
        int scb = 0, scr = 0;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                int c[3];
                je_rgb(src, pitch, layout, ys[a], xs[b], c);
                scb += th_cb(c[0], c[1], c[2]);
                scr += th_cr(c[0], c[1], c[2]);
            }
        const int bias = (kc & 1) ? 2 : 1;
        blk[4][t] = ((scb + bias) >> 2) - 128;
        blk[5][t] = ((scr + bias) >> 2) - 128;
    }
    __syncthreads();
    const int b = t >> 3, l = t & 7;                          // lane -> (block, row / column)
    if (b < nblk) fdct8(&blk[b][l * 8], 1, true);
    __syncthreads();
    if (b < nblk) {
        int* col = &blk[b][l];
        fdct8(col, 8, false);
        const unsigned short* qt = q.q[b < 4 ? 0 : 1];
        for (int i = 0; i < 8; ++i) {                          // round half away from zero of coef / 8q
            const int d = 8 * qt[i * 8 + l], c = col[i * 8];
            const int m = (abs(c) + (d >> 1)) / d;
            col[i * 8] = c < 0 ? -m : m;
        }
    }
    __syncthreads();
    const int bw = (W + 7) / 8, bh = (H + 7) / 8;
    const int z = JE_ZIGZAG[t];
    if (components == 1) {
        for (int k = 0; k < 4; ++k) {
            const int bx = 2 * mx + (k & 1), by = 2 * my + (k >> 1);
            if (bx < bw && by < bh) coef[((size_t)by * bw + bx) * 64 + t] = (short)blk[k][z];
        }
        return;
    }
    short* out = coef + ((size_t)my * gridDim.x + mx) * 6 * 64;
    int dc = 0;
    for (int k = 0; k < 4; ++k) {
        const bool real = 2 * mx + (k & 1) < bw && 2 * my + (k >> 1) < bh;
        if (real) dc = blk[k][0];                              // a dummy block keeps the DC term before it (block 0 is never one)
        out[k * 64 + t] = (short)(real ? blk[k][z] : (t == 0 ? dc : 0));
    }
    out[4 * 64 + t] = colour ? (short)blk[4][z] : (short)0;
    out[5 * 64 + t] = colour ? (short)blk[5][z] : (short)0;
}

// the block whose DC term block b's difference is taken against (the previous block of its component in scan order), -1: none
__device__ __forceinline__ long long je_prev(long long b, int components) {
    if (components == 1) return b - 1;
    const int k = (int)(b % 6);
    if (k >= 1 && k <= 3) return b - 1;
    if (b < 6) return -1;
    return k == 0 ? b - 3 : b - 6;
}

constexpr int JE_ROW = 66;                                     // shorts per staged block: 33 dwords, so the lanes' rows start on different banks

// the tile's coefficient blocks, and the DC term in front of each, into LDS (coalesced)
__device__ __forceinline__ void je_stage_tile(const short* __restrict__ coef, int n, int components, short* zz, int* prev_dc) {
    const int t = threadIdx.x, b0 = blockIdx.x * JE_TILE, nb = min(JE_TILE, n - b0);
    const uint32_t* g = (const uint32_t*)(coef + (size_t)b0 * 64);
    for (int e = t; e < nb * 32; e += JE_TILE) *(uint32_t*)(zz + (e >> 5) * JE_ROW + (e & 31) * 2) = g[e];
    const long long p = je_prev((long long)b0 + t, components);
    prev_dc[t] = (t < nb && p >= 0) ? coef[(size_t)p * 64] : 0;
}

// exclusive scan of one value per thread over the workgroup (256 threads); *total: the sum
template <typename T> __device__ __forceinline__ T je_block_scan(T v, T* sh, T* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const T a = t >= d ? sh[t - d] : (T)0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const T incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(JE_TILE) je_sizes_kernel(const short* __restrict__ coef, int n, int components, unsigned int* __restrict__ local,
                                                           unsigned long long* __restrict__ tile_bits) {
    __shared__ __attribute__((aligned(16))) short zz[JE_TILE * JE_ROW];
    __shared__ int prev_dc[JE_TILE];
    __shared__ JeHuff huff;
    __shared__ unsigned int sh[JE_TILE];
    const int t = threadIdx.x, b = blockIdx.x * JE_TILE + t;
    for (int e = t; e < (int)(sizeof(JeHuff) / 4); e += JE_TILE) ((uint32_t*)&huff)[e] = ((const uint32_t*)&JE_HUFF)[e];
    je_stage_tile(coef, n, components, zz, prev_dc);
    __syncthreads();
    unsigned int bits = 0;
    if (b < n) {
        const int tab = (components == 3 && b % 6 >= 4) ? 1 : 0;
        bits = (unsigned int)je_block_bits(zz + t * JE_ROW, prev_dc[t], huff.dc[tab], huff.ac[tab]);
    }
    unsigned int total;
    const unsigned int off = je_block_scan(bits, sh, &total);
    if (b < n) local[b] = off;
    if (t == 0) tile_bits[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) je_scan_kernel(unsigned long long* __restrict__ v, int n) {
    __shared__ unsigned long long sh[256];
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + t;
        unsigned long long total;
        const unsigned long long off = je_block_scan<unsigned long long>(i < n ? v[i] : 0ULL, sh, &total);
        if (i < n) v[i] = carry + off;
        carry += total;
    }
    if (t == 0) v[n] = carry;
}

__global__ void __launch_bounds__(256) je_offsets_kernel(const unsigned int* __restrict__ local, const unsigned long long* __restrict__ tile_off, int n,
                                                         long long* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < n) out[b] = (long long)(tile_off[b / JE_TILE] + local[b]);
    if (b == n) out[n] = (long long)tile_off[(n + JE_TILE - 1) / JE_TILE];
}

__global__ void __launch_bounds__(JE_TILE) je_pack_kernel(const short* __restrict__ coef, int n, int components, const unsigned int* __restrict__ local,
                                                          const unsigned long long* __restrict__ tile_off, uint32_t* __restrict__ words) {
    __shared__ __attribute__((aligned(16))) short zz[JE_TILE * JE_ROW];
    __shared__ int prev_dc[JE_TILE];
    __shared__ JeHuff huff;
    const int t = threadIdx.x, b = blockIdx.x * JE_TILE + t;
    for (int e = t; e < (int)(sizeof(JeHuff) / 4); e += JE_TILE) ((uint32_t*)&huff)[e] = ((const uint32_t*)&JE_HUFF)[e];
    je_stage_tile(coef, n, components, zz, prev_dc);
    __syncthreads();
    if (b >= n) return;
    const int tab = (components == 3 && b % 6 >= 4) ? 1 : 0;
    JeBits o(words, (long long)(tile_off[blockIdx.x] + local[b]));
    je_block_pack(o, zz + t * JE_ROW, prev_dc[t], huff.dc[tab], huff.ac[tab]);
    if (b == n - 1) {                                          // the scan's last byte is filled with 1-bits
        const int pad = (8 - (int)(tile_off[gridDim.x] & 7)) & 7;
        o.put((1u << pad) - 1u, pad);
    }
    o.finish();
}

// the 8 scan bytes of a thread (the buffer is readable up to the end of the tile) and how many of them are 0xFF; bytes behind the scan do not count
__device__ __forceinline__ unsigned long long je_ff8(const uint8_t* __restrict__ scan, long long bytes, long long i0, int* count) {
    const unsigned long long w = *(const unsigned long long*)(scan + i0);
    int c = 0;
    for (int j = 0; j < 8; ++j) c += (i0 + j < bytes && ((w >> (8 * j)) & 0xFF) == 0xFF) ? 1 : 0;
    *count = c;
    return w;
}

__global__ void __launch_bounds__(256) je_ff_count_kernel(const uint8_t* __restrict__ scan, long long bytes, unsigned long long* __restrict__ tile_ff) {
    __shared__ unsigned int sh[256];
    int c;
    je_ff8(scan, bytes, ((long long)blockIdx.x * 256 + threadIdx.x) * 8, &c);
    unsigned int total;
    je_block_scan<unsigned int>((unsigned int)c, sh, &total);
    if (threadIdx.x == 0) tile_ff[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) je_stuff_kernel(const uint8_t* __restrict__ scan, long long bytes, const unsigned long long* __restrict__ tile_off,
                                                       uint8_t* __restrict__ out) {
    __shared__ unsigned int sh[256];
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    int c;
    const unsigned long long w = je_ff8(scan, bytes, i0, &c);
    unsigned int total;
    const unsigned int before = je_block_scan<unsigned int>((unsigned int)c, sh, &total);
    uint8_t* o = out + i0 + (long long)tile_off[blockIdx.x] + before;
    for (int j = 0; j < 8 && i0 + j < bytes; ++j) {
        const uint8_t v = (uint8_t)(w >> (8 * j));
        *o++ = v;
        if (v == 0xFF) *o++ = 0;
    }
}

}  // namespace

hipError_t launch_je_coef(const uint8_t* src, size_t pitch, int layout, int components, int H, int W, const ThQuant& q, short* coef, hipStream_t s) {
    hipLaunchKernelGGL(je_coef_kernel, dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), dim3(64), 0, s, src, pitch, layout, components, H, W, q,
                       coef);
    return hipGetLastError();
}
hipError_t launch_je_sizes(const short* coef, int n, int components, unsigned int* local, unsigned long long* tile_bits, hipStream_t s) {
    hipLaunchKernelGGL(je_sizes_kernel, dim3((unsigned)((n + JE_TILE - 1) / JE_TILE)), dim3(JE_TILE), 0, s, coef, n, components, local, tile_bits);
    return hipGetLastError();
}
hipError_t launch_je_scan(unsigned long long* v, int n, hipStream_t s) {
    hipLaunchKernelGGL(je_scan_kernel, dim3(1), dim3(256), 0, s, v, n);
    return hipGetLastError();
}
hipError_t launch_je_offsets(const unsigned int* local, const unsigned long long* tile_off, int n, long long* out, hipStream_t s) {
    hipLaunchKernelGGL(je_offsets_kernel, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, s, local, tile_off, n, out);
    return hipGetLastError();
}
hipError_t launch_je_pack(const short* coef, int n, int components, const unsigned int* local, const unsigned long long* tile_off, uint32_t* words,
                          hipStream_t s) {
    hipLaunchKernelGGL(je_pack_kernel, dim3((unsigned)((n + JE_TILE - 1) / JE_TILE)), dim3(JE_TILE), 0, s, coef, n, components, local, tile_off, words);
    return hipGetLastError();
}
hipError_t launch_je_ff_count(const uint8_t* scan, long long bytes, unsigned long long* tile_ff, hipStream_t s) {
    hipLaunchKernelGGL(je_ff_count_kernel, dim3((unsigned)((bytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE)), dim3(256), 0, s, scan, bytes, tile_ff);
    return hipGetLastError();
}
hipError_t launch_je_stuff(const uint8_t* scan, long long bytes, const unsigned long long* tile_off, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(je_stuff_kernel, dim3((unsigned)((bytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE)), dim3(256), 0, s, scan, bytes, tile_off, out);
    return hipGetLastError();
}
