// The extractor's OCR-input down-scaling (enhanced_extractor.py:486-512) on the device: Image.thumbnail((max_dim, max_dim)) in RGB and
// the JPEG file (quality 90 / 95) that easyocr decodes, both to the bit of Pillow 12 / libjpeg-turbo (tests/jpeg_ref.py states each step).
//   th_reduce      ImagingReduce (Reduce.c): box mean ((sum + n / 2) * multiplier) >> 24, partial last column / row over the pixels it holds
//   th_resample_h  ImagingResampleHorizontal_8bpc over the rows the vertical pass reads (22-bit fixed point, clip8)
//   th_resample_v  ImagingResampleVertical_8bpc
//   th_jpeg_mcu    one 16x16 MCU (4:2:0) per 64-lane workgroup: jccolor.c RGB -> YCbCr with the edge replication of jcprepct.c /
//                  jcsample.c, h2v2_downsample, jfdctint.c, quantise / dequantise, jidctint.c with the & RANGE_MASK table -> Y' and
//                  the half-resolution Cb' / Cr' planes
//   th_upsample    h2v2_fancy_upsample (plain replication for a chroma plane at most 2 wide) + jdcolor.c YCbCr -> RGB; gray = Y'
//   th_direct      pages that take no thumbnail: gray -> replicated RGB, RGB / BGR -> RGB + libpng's gray, YCbCr -> RGB + Y
#include "common.h"
#include "kernels.h"
#include "jpeg_dev.h"

namespace {

// channel c (R, G, B) of pixel (y, x) of a page in one of the PAGE_* layouts
__device__ __forceinline__ int th_px(const uint8_t* __restrict__ src, size_t pitch, int layout, int y, int x, int c) {
    const uint8_t* row = src + (size_t)y * pitch;
    switch (layout) {
        case PAGE_GRAY: return row[x];
        case PAGE_BGR: return row[3 * x + 2 - c];
        default: return row[3 * x + c];
    }
}

// division_UINT32 (Reduce.c): 2^32 / (256 * n) in single precision, truncated
__device__ __forceinline__ unsigned int th_reduce_mult(int n) {
    return (unsigned int)(4294967296.0f / (float)(unsigned int)(256 * n));
}

__global__ void __launch_bounds__(256) th_reduce_kernel(const uint8_t* __restrict__ src, size_t pitch, int layout, int H, int W, int fx, int fy,
                                                        uint8_t* __restrict__ dst, int rh, int rw, int C) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= rw || y >= rh) return;
    const int x0 = x * fx, y0 = y * fy, x1 = min(x0 + fx, W), y1 = min(y0 + fy, H);
    const int n = (x1 - x0) * (y1 - y0);
    const unsigned int mult = th_reduce_mult(n), amend = (unsigned int)(n / 2);
    for (int c = 0; c < C; ++c) {
        unsigned int ss = 0;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) ss += (unsigned int)th_px(src, pitch, layout, yy, xx, c);
        dst[((size_t)y * rw + x) * C + c] = (uint8_t)(((ss + amend) * mult) >> 24);
    }
}

__device__ __forceinline__ uint8_t th_clip8(int ss) {
    if (ss >= (1 << TH_PRECISION_BITS << 8)) return 255;
    if (ss <= 0) return 0;
    return (uint8_t)(ss >> TH_PRECISION_BITS);
}

// one thread per output byte (x, c) of rows y0 .. y0 + rows - 1 of the source
__global__ void __launch_bounds__(256) th_resample_h_kernel(const uint8_t* __restrict__ src, size_t pitch, int layout, int y0, int rows, int ow,
                                                            int C, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                            uint8_t* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (e >= ow * C || y >= rows) return;
    const int x = e / C, c = e - x * C;
    const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
    const int* k = kk + (size_t)x * ksize;
    int ss = 1 << (TH_PRECISION_BITS - 1);
    for (int i = 0; i < n; ++i) ss += th_px(src, pitch, layout, y0 + y, xmin + i, c) * k[i];
    dst[(size_t)y * ow * C + e] = th_clip8(ss);
}

// one thread per output byte; rows of `width` bytes, read at `spitch` (row 0 of src is source row y0), written at `dpitch`
__global__ void __launch_bounds__(256) th_resample_v_kernel(const uint8_t* __restrict__ src, size_t spitch, int y0, int width, int oh,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                            uint8_t* __restrict__ dst, size_t dpitch) {
    const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (e >= width || y >= oh) return;
    const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
    const int* k = kk + (size_t)y * ksize;
    int ss = 1 << (TH_PRECISION_BITS - 1);
    for (int i = 0; i < n; ++i) ss += (int)src[(size_t)(ymin - y0 + i) * spitch + e] * k[i];
    dst[(size_t)y * dpitch + e] = th_clip8(ss);
}

// One MCU per workgroup of 64 lanes (one wavefront).  Blocks 0-3 hold Y (2x2), 4 Cb, 5 Cr; a gray page (C == 1: R = G = B, hence
// Cb = Cr = 128 exactly, whose blocks come back as 128 everywhere) runs the four Y blocks only.
__global__ void __launch_bounds__(64) th_jpeg_mcu_kernel(const uint8_t* __restrict__ src, size_t pitch, int C, int H, int W, ThQuant q,
                                                         uint8_t* __restrict__ yp, int wp, uint8_t* __restrict__ cbp, uint8_t* __restrict__ crp) {
    __shared__ int blk[6][64];
    const int t = threadIdx.x, mx = blockIdx.x, my = blockIdx.y;
    const int layout = C == 1 ? PAGE_GRAY : PAGE_RGB;
    const int nblk = C == 1 ? 4 : 6;
    for (int p = 0; p < 4; ++p) {                              // 256 pixels, edge-replicated beyond the page (expand_right / bottom_edge)
        const int id = t + 64 * p, py = id >> 4, px = id & 15;
        const int gy = min(my * 16 + py, H - 1), gx = min(mx * 16 + px, W - 1);
        const int r = th_px(src, pitch, layout, gy, gx, 0);
        const int v = C == 1 ? r : th_y(r, th_px(src, pitch, layout, gy, gx, 1), th_px(src, pitch, layout, gy, gx, 2));
        blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = v - 128;
    }
    if (C != 1) {
        // h2v2_downsample of the edge-expanded rows; the chroma rows past ceil(H / 2) repeat the last one (jcprepct.c pads the
        // downsampled plane, not the input)
        const int cy = t >> 3, cx = t & 7, kc = mx * 8 + cx;
        const int kr = min(my * 8 + cy, (H + 1) / 2 - 1);
        const int r0 = 2 * kr, r1 = min(2 * kr + 1, H - 1), c0 = min(2 * kc, W - 1), c1 = min(2 * kc + 1, W - 1);
        int scb = 0, scr = 0;
        const int ys[2] = {r0, r1}, xs[2] = {c0, c1};
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int R = th_px(src, pitch, layout, ys[a], xs[b], 0), G = th_px(src, pitch, layout, ys[a], xs[b], 1),
                          B = th_px(src, pitch, layout, ys[a], xs[b], 2);
                scb += th_cb(R, G, B);
                scr += th_cr(R, G, B);
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
        for (int i = 0; i < 8; ++i) {                          // quantise (round half away from zero of coef / 8q), dequantise
            const int qv = qt[i * 8 + l], d = 8 * qv, c = col[i * 8];
            const int m = (abs(c) + (d >> 1)) / d;
            col[i * 8] = (c < 0 ? -m : m) * qv;
        }
        idct8(col, 8, true);
    }
    __syncthreads();
    if (b < nblk) {
        int* row = &blk[b][l * 8];
        idct8(row, 1, false);
        if (b < 4) {
            uint8_t* o = yp + (size_t)(my * 16 + (b >> 1) * 8 + l) * wp + mx * 16 + (b & 1) * 8;
            for (int i = 0; i < 8; ++i) o[i] = (uint8_t)row[i];
        } else {
            uint8_t* o = (b == 4 ? cbp : crp) + (size_t)(my * 8 + l) * (wp / 2) + mx * 8;
            for (int i = 0; i < 8; ++i) o[i] = (uint8_t)row[i];
        }
    }
}

// gray == C == 1 pages: Cb = Cr = 128.  ycc != null: the upsampled triple (stage 2) instead of rgb / gray
__global__ void __launch_bounds__(256) th_upsample_kernel(const uint8_t* __restrict__ yp, int wp, const uint8_t* __restrict__ cbp,
                                                          const uint8_t* __restrict__ crp, int H, int W, int gray_only, uint8_t* __restrict__ rgb,
                                                          uint8_t* __restrict__ gray, uint8_t* __restrict__ ycc) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int Y = yp[(size_t)y * wp + x];
    int cb = 128, cr = 128;
    if (!gray_only) {
        const int ch = (H + 1) / 2, cw = (W + 1) / 2;
        cb = th_fancy(cbp, wp / 2, ch, cw, y, x);
        cr = th_fancy(crp, wp / 2, ch, cw, y, x);
    }
    const size_t i = (size_t)y * W + x;
    if (ycc) {
        ycc[3 * i] = (uint8_t)Y;
        ycc[3 * i + 1] = (uint8_t)cb;
        ycc[3 * i + 2] = (uint8_t)cr;
        return;
    }
    jpeg_ycc_to_rgb(Y, cb, cr, rgb + 3 * i);
    gray[i] = (uint8_t)Y;
}

__global__ void __launch_bounds__(256) th_direct_kernel(const uint8_t* __restrict__ src, size_t pitch, int layout, int H, int W,
                                                        uint8_t* __restrict__ rgb, uint8_t* __restrict__ gray) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const uint8_t* p = src + (size_t)y * pitch;
    if (layout == PAGE_YCC4 || layout == PAGE_YCC3) {
        const int s = layout == PAGE_YCC4 ? 4 : 3;
        jpeg_ycc_to_rgb(p[s * x], p[s * x + 1], p[s * x + 2], rgb + 3 * i);
        if (gray) gray[i] = p[s * x];
        return;
    }
    const int r = th_px(src, pitch, layout, y, x, 0), g = th_px(src, pitch, layout, y, x, 1), b = th_px(src, pitch, layout, y, x, 2);
    rgb[3 * i] = (uint8_t)r;
    rgb[3 * i + 1] = (uint8_t)g;
    rgb[3 * i + 2] = (uint8_t)b;
    if (gray) gray[i] = layout == PAGE_GRAY ? (uint8_t)r : (uint8_t)((r * 9797 + g * 19234 + b * 3737) >> 15);   // libpng rgb_to_gray
}

dim3 px_grid(int H, int W) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

}  // namespace

hipError_t launch_th_reduce(const uint8_t* src, size_t pitch, int layout, int H, int W, int fx, int fy, uint8_t* dst, int rh, int rw, int C,
                            hipStream_t s) {
    hipLaunchKernelGGL(th_reduce_kernel, px_grid(rh, rw), dim3(256), 0, s, src, pitch, layout, H, W, fx, fy, dst, rh, rw, C);
    return hipGetLastError();
}
hipError_t launch_th_resample_h(const uint8_t* src, size_t pitch, int layout, int y0, int rows, int ow, int C, const int* bounds, const int* kk,
                                int ksize, uint8_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(th_resample_h_kernel, dim3((unsigned)((ow * C + 255) / 256), (unsigned)rows), dim3(256), 0, s, src, pitch, layout, y0, rows,
                       ow, C, bounds, kk, ksize, dst);
    return hipGetLastError();
}
hipError_t launch_th_resample_v(const uint8_t* src, size_t spitch, int y0, int width, int oh, const int* bounds, const int* kk, int ksize,
                                uint8_t* dst, size_t dpitch, hipStream_t s) {
    hipLaunchKernelGGL(th_resample_v_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)oh), dim3(256), 0, s, src, spitch, y0, width, oh, bounds,
                       kk, ksize, dst, dpitch);
    return hipGetLastError();
}
hipError_t launch_th_jpeg(const uint8_t* src, size_t pitch, int C, int H, int W, const ThQuant& q, uint8_t* yp, int wp, uint8_t* cbp, uint8_t* crp,
                          hipStream_t s) {
    hipLaunchKernelGGL(th_jpeg_mcu_kernel, dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), dim3(64), 0, s, src, pitch, C, H, W, q, yp,
                       wp, cbp, crp);
    return hipGetLastError();
}
hipError_t launch_th_upsample(const uint8_t* yp, int wp, const uint8_t* cbp, const uint8_t* crp, int H, int W, int gray_only, uint8_t* rgb,
                              uint8_t* gray, uint8_t* ycc, hipStream_t s) {
    hipLaunchKernelGGL(th_upsample_kernel, px_grid(H, W), dim3(256), 0, s, yp, wp, cbp, crp, H, W, gray_only, rgb, gray, ycc);
    return hipGetLastError();
}
hipError_t launch_th_direct(const uint8_t* src, size_t pitch, int layout, int H, int W, uint8_t* rgb, uint8_t* gray, hipStream_t s) {
    hipLaunchKernelGGL(th_direct_kernel, px_grid(H, W), dim3(256), 0, s, src, pitch, layout, H, W, rgb, gray);
    return hipGetLastError();
}
