// Device kernels of the extractor's text-region auto-crop (enhanced_extractor.py::_auto_crop_text_region, `crop_for_ocr`):
//   BGR2GRAY -> GaussianBlur 3x3 sigma 0 -> CLAHE 2.0 8x8 -> four threshold cues OR'd (adaptive MEAN 35/10 inv, adaptive GAUSSIAN
//   31/5 inv, Otsu inv, Otsu of the Sobel gradient) -> two CLOSE / OPEN / dilate morphology variants OR'd -> RETR_EXTERNAL contours
//   as the bounding boxes of the external 8-connected components.
// The CLAHE stage is preproc.hip's (pp_clahe_*); everything else is here.  The mask after the threshold cues is packed one bit per
// pixel (32 pixels per dword, rows padded to whole dwords with zero bits), so the morphology reads and writes 1/8 of a byte plane.
// The CPU restatement the tests compare against is tests/autocrop_ref.py.
#include "common.h"
#include "kernels.h"

#include <climits>

namespace {

__device__ __forceinline__ int refl101(int v, int n) {      // BORDER_REFLECT_101 for a 1-pixel halo
    if (v < 0) return n > 1 ? 1 : 0;
    if (v >= n) return n > 1 ? n - 2 : 0;
    return v;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- cvtColor(BGR2GRAY) (channels 3; the 15-bit fixed point of craft_misc.hip::gray_kernel) or the plane itself (channels 1), read
// through a row pitch, and GaussianBlur(3x3, sigma 0): OpenCV's small-kernel table [1/4, 1/2, 1/4] as 8.8 fixed-point taps 64/128/64,
// rows then columns, (sum + 2^15) >> 16, BORDER_REFLECT_101 (oracle/preprocess.py::gaussian_blur3_u8 with these taps)
__global__ void __launch_bounds__(256) ac_gray_blur_kernel(const uint8_t* __restrict__ src, int H, int W, size_t pitch, int channels,
                                                           uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int xs[3] = {refl101(x - 1, W), x, refl101(x + 1, W)};
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int ys[3] = {refl101(y - 1, H), y, refl101(y + 1, H)};
        int acc = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint8_t* row = src + (size_t)ys[r] * pitch;
            int h = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int g;
                if (channels == 3) {
                    const uint8_t* p = row + (size_t)xs[c] * 3;
                    g = ((int)p[2] * 9798 + (int)p[1] * 19235 + (int)p[0] * 3735 + (1 << 14)) >> 15;
                } else {
                    g = row[xs[c]];
                }
                h += (c == 1 ? 128 : 64) * g;
            }
            acc += (r == 1 ? 128 : 64) * h;
        }
        const int v = (acc + (1 << 15)) >> 16;
        dst[(size_t)y * W + x] = (uint8_t)(v > 255 ? 255 : v);
    }
}

// ---- row pass of the two adaptive-threshold means, BORDER_REPLICATE: box sum of 35 (<= 8925) and the 31-tap fixed-point Gaussian row
// value (ufixedpoint16, <= 65280), both as u16 planes
__global__ void __launch_bounds__(256) ac_rows_kernel(const uint8_t* __restrict__ e, int H, int W, uint16_t* __restrict__ rbox,
                                                      uint16_t* __restrict__ rgau, AcTaps taps) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint8_t* row = e + (size_t)y * W;
        int b = 0;
        for (int d = -AC_BOX_R; d <= AC_BOX_R; ++d) b += row[clampi(x + d, 0, W - 1)];
        int g = 0;
#pragma unroll
        for (int d = -AC_GAU_R; d <= AC_GAU_R; ++d) g += taps.k[d + AC_GAU_R] * (int)row[clampi(x + d, 0, W - 1)];
        rbox[(size_t)y * W + x] = (uint16_t)b;
        rgau[(size_t)y * W + x] = (uint16_t)g;
    }
}

// ---- column pass + the per-pixel cues.  part = bit 0: adaptive MEAN (src <= mean - 10) or adaptive GAUSSIAN (src <= gmean - 5);
// grad = saturate(|Sobel dx|) + saturate(|Sobel dy|), saturated (BORDER_REFLECT_101); hist[0..255] += CLAHE values, hist[256..511] += grad
__global__ void __launch_bounds__(256) ac_cols_kernel(const uint8_t* __restrict__ e, const uint16_t* __restrict__ rbox, const uint16_t* __restrict__ rgau,
                                                      int H, int W, AcTaps taps, uint8_t* __restrict__ part, uint8_t* __restrict__ grad,
                                                      unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[512];
    h[threadIdx.x] = 0;
    h[threadIdx.x + 256] = 0;
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < W) {
        const float inv = (float)(1.0 / ((double)AC_BOX * AC_BOX));
        const int xm = refl101(x - 1, W), xp = refl101(x + 1, W);
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            int b = 0;
            for (int d = -AC_BOX_R; d <= AC_BOX_R; ++d) b += rbox[(size_t)clampi(y + d, 0, H - 1) * W + x];
            unsigned int g = 0;
#pragma unroll
            for (int d = -AC_GAU_R; d <= AC_GAU_R; ++d) g += (unsigned)taps.k[d + AC_GAU_R] * rgau[(size_t)clampi(y + d, 0, H - 1) * W + x];
            // boxFilter(normalize) on 8u: ColumnSum<int, uchar> multiplies the integer sum by the float scale and rounds half to even
            int mean = __float2int_rn((float)b * inv);
            mean = mean > 255 ? 255 : mean;
            int gm = (int)((g + (1u << 15)) >> 16);
            gm = gm > 255 ? 255 : gm;
            const int v = e[(size_t)y * W + x];
            const bool cue = (v - mean <= -AC_MEAN_C) || (v - gm <= -AC_GAU_C);
            const uint8_t *r0 = e + (size_t)refl101(y - 1, H) * W, *r1 = e + (size_t)y * W, *r2 = e + (size_t)refl101(y + 1, H) * W;
            const int dx = ((int)r0[xp] - r0[xm]) + 2 * ((int)r1[xp] - r1[xm]) + ((int)r2[xp] - r2[xm]);
            const int dy = ((int)r2[xm] - r0[xm]) + 2 * ((int)r2[x] - r0[x]) + ((int)r2[xp] - r0[xp]);
            const int ax = min(abs(dx), 255), ay = min(abs(dy), 255);
            const int gr = min(ax + ay, 255);
            part[(size_t)y * W + x] = cue ? 1 : 0;
            grad[(size_t)y * W + x] = (uint8_t)gr;
            atomicAdd(&h[v], 1u);
            atomicAdd(&h[256 + gr], 1u);
        }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
    if (h[threadIdx.x + 256]) atomicAdd(&hist[threadIdx.x + 256], h[threadIdx.x + 256]);
}

// ---- getThreshVal_Otsu_8u (imgproc/thresh.cpp): the same double arithmetic in the same order, first maximum kept, bins whose class
// weight is within FLT_EPSILON of 0 or 1 skipped (a single-valued image gives 0).  Thread t < 2 handles histogram t.
__global__ void ac_otsu_kernel(const unsigned int* __restrict__ hist, unsigned long long n, int* __restrict__ thr) {
    const int t = threadIdx.x;
    if (t >= 2) return;
    const unsigned int* h = hist + 256 * t;
    const double scale = 1.0 / (double)n;
    double mu = 0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)h[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0;
    int max_val = 0;
    const double eps = 1.1920928955078125e-07;
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)h[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < eps || fmax(q1, q2) > 1.0 - eps) continue;
        mu1 = (mu1 + (double)i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    thr[t] = max_val;
}

// ---- composite mask, packed: pixel = part | (clahe <= t_clahe: Otsu BINARY_INV) | (grad > t_grad: Otsu BINARY); one dword per thread
__global__ void __launch_bounds__(256) ac_pack_kernel(const uint8_t* __restrict__ e, const uint8_t* __restrict__ part, const uint8_t* __restrict__ grad,
                                                      const int* __restrict__ thr, int H, int W, int WW, uint32_t* __restrict__ bits) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= WW) return;
    const int te = thr[0], tg = thr[1];
    const int x0 = j * 32, nx = min(32, W - x0);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const size_t o = (size_t)y * W + x0;
        uint32_t w = 0;
        for (int k = 0; k < nx; ++k) {
            const bool on = part[o + k] || (int)e[o + k] <= te || (int)grad[o + k] > tg;
            w |= (on ? 1u : 0u) << k;
        }
        bits[(size_t)y * WW + j] = w;
    }
}

// ---- a byte mask (nonzero = set) read through a row pitch, packed the same way (bbocr_op_autocrop_mask_stage): padding bits are 0
__global__ void __launch_bounds__(256) ac_pack_mask_kernel(const uint8_t* __restrict__ src, size_t pitch, int H, int W, int WW,
                                                           uint32_t* __restrict__ bits) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= WW) return;
    const int x0 = j * 32, nx = min(32, W - x0);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint8_t* row = src + (size_t)y * pitch + x0;
        uint32_t w = 0;
        for (int k = 0; k < nx; ++k) w |= (row[k] ? 1u : 0u) << k;
        bits[(size_t)y * WW + j] = w;
    }
}

// ---- rect morphology along rows on the packed mask, radius r < 32: dilate = OR of the shifted words (pixels outside the row are 0),
// erode = AND (pixels outside the row are 1: OpenCV's default border value never lets the border take part); padding bits stay 0
__global__ void __launch_bounds__(256) ac_row_morph_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int H, int W, int WW, int r,
                                                           int erode) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= WW) return;
    const int tail = W - (WW - 1) * 32;                               // valid bits of the last word, 1..32
    const uint32_t lastmask = tail == 32 ? 0xffffffffu : ((1u << tail) - 1u);
    const uint32_t out_of_row = erode ? 0xffffffffu : 0u;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint32_t* row = src + (size_t)y * WW;
        auto word = [&](int q) -> uint32_t {
            if (q < 0 || q >= WW) return out_of_row;
            uint32_t w = row[q];
            if (q == WW - 1 && erode) w |= ~lastmask;
            return w;
        };
        const uint64_t lo = ((uint64_t)word(j) << 32) | word(j - 1);   // pixels x-32 .. x+31 relative to the word's first bit
        const uint64_t hi = ((uint64_t)word(j + 1) << 32) | word(j);
        uint32_t v = (uint32_t)(lo >> 32);
        for (int s = 1; s <= r; ++s) {
            const uint32_t a = (uint32_t)(lo >> (32 - s)), b = (uint32_t)(hi >> s);   // pixel x-s, pixel x+s
            v = erode ? (v & a & b) : (v | a | b);
        }
        if (j == WW - 1) v &= lastmask;
        dst[(size_t)y * WW + j] = v;
    }
}

// ---- the same along columns (rows outside the plane do not take part); or_with (may be null) is OR'd into the result
__global__ void __launch_bounds__(256) ac_col_morph_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int H, int WW, int r, int erode,
                                                           const uint32_t* __restrict__ or_with) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= WW) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int y0 = max(0, y - r), y1 = min(H - 1, y + r);
        uint32_t v = erode ? 0xffffffffu : 0u;
        for (int q = y0; q <= y1; ++q) v = erode ? (v & src[(size_t)q * WW + j]) : (v | src[(size_t)q * WW + j]);
        if (or_with) v |= or_with[(size_t)y * WW + j];
        dst[(size_t)y * WW + j] = v;
    }
}

__device__ __forceinline__ bool fg_at(const uint32_t* __restrict__ bits, int WW, int x, int y) {
    return (bits[(size_t)y * WW + (x >> 5)] >> (x & 31)) & 1u;
}

__device__ __forceinline__ int uf_find(const int* __restrict__ label, int x) {
    int p = label[x];
    while (p != x) {
        x = p;
        p = label[x];
    }
    return x;
}
__device__ __forceinline__ void uf_union(int* __restrict__ label, int a, int b) {
    for (;;) {
        a = uf_find(label, a);
        b = uf_find(label, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(label + b, a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(label + a, b);
            if (old == a) return;
            a = old;
        }
    }
}

// ---- union-find over the whole plane: foreground 8-connected, background 4-connected (the two never meet).  label = flat index.
__global__ void __launch_bounds__(256) ac_ccl_init_kernel(int* __restrict__ label, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) label[(size_t)y * W + x] = y * W + x;
}
__global__ void __launch_bounds__(256) ac_ccl_merge_kernel(const uint32_t* __restrict__ bits, int* __restrict__ label, int H, int W, int WW) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int i = y * W + x;
        const bool f = fg_at(bits, WW, x, y);
        const bool wl = x > 0 && fg_at(bits, WW, x - 1, y) == f;
        if (wl) uf_union(label, i, i - 1);
        if (y > 0) {
            const bool n = fg_at(bits, WW, x, y - 1) == f;
            if (n) {
                uf_union(label, i, i - W);
            } else if (f) {                                          // diagonals only matter when the pixel above is not connected
                if (x > 0 && !wl && fg_at(bits, WW, x - 1, y - 1)) uf_union(label, i, i - W - 1);
                if (x + 1 < W && fg_at(bits, WW, x + 1, y - 1)) uf_union(label, i, i - W + 1);
            }
        }
    }
}
__global__ void __launch_bounds__(256) ac_ccl_compress_kernel(int* __restrict__ label, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int i = y * W + x;
        label[i] = uf_find(label, i);
    }
}
// flag[root] = 1: the background component touches the image edge (outer background)
__global__ void __launch_bounds__(256) ac_outer_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ label, uint8_t* __restrict__ flag,
                                                       int H, int W, int WW) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        if ((x == 0 || y == 0 || x == W - 1 || y == H - 1) && !fg_at(bits, WW, x, y)) flag[label[y * W + x]] = 1;
    }
}
// flag[root] = 2: the foreground component touches the edge or is 4-adjacent to the outer background (a RETR_EXTERNAL contour)
__global__ void __launch_bounds__(256) ac_external_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ label, uint8_t* __restrict__ flag,
                                                          int H, int W, int WW) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        if (!fg_at(bits, WW, x, y)) continue;
        const int i = y * W + x;
        bool ext = x == 0 || y == 0 || x == W - 1 || y == H - 1;
        if (!ext) {
            const int nb[4] = {i - 1, i + 1, i - W, i + W};
            const int nx[4] = {x - 1, x + 1, x, x}, ny[4] = {y, y, y - 1, y + 1};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!fg_at(bits, WW, nx[k], ny[k]) && flag[label[nb[k]]] == 1) ext = true;
        }
        if (ext) flag[label[i]] = 2;
    }
}
// every external root gets a component number k < cap (label[root] = n + k) and its box is reset
__global__ void __launch_bounds__(256) ac_enum_kernel(int* __restrict__ label, const uint8_t* __restrict__ flag, int H, int W, int* __restrict__ count,
                                                      int cap, int* __restrict__ boxes) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int n = H * W;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int i = y * W + x;
        if (label[i] != i || flag[i] != 2) continue;
        const int k = atomicAdd(count, 1);
        if (k >= cap) continue;                                     // the host reports the overflow
        label[i] = n + k;
        boxes[4 * k + 0] = INT_MAX;
        boxes[4 * k + 1] = INT_MAX;
        boxes[4 * k + 2] = -1;
        boxes[4 * k + 3] = -1;
    }
}
__device__ __forceinline__ int comp_of(const int* __restrict__ label, int i, int n) {   // component number of a foreground pixel, or -1
    const int r = label[i];
    if (r >= n) return r - n;
    const int v = label[r];
    return v >= n ? v - n : -1;
}
// boundingRect: min / max atomics, issued only by pixels on the matching side of a run (left / right / top / bottom neighbour not set)
__global__ void __launch_bounds__(256) ac_boxes_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ label, int H, int W, int WW,
                                                       int* __restrict__ boxes) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int n = H * W;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        if (!fg_at(bits, WW, x, y)) continue;
        const bool l = x == 0 || !fg_at(bits, WW, x - 1, y), r = x == W - 1 || !fg_at(bits, WW, x + 1, y);
        const bool t = y == 0 || !fg_at(bits, WW, x, y - 1), b = y == H - 1 || !fg_at(bits, WW, x, y + 1);
        if (!(l || r || t || b)) continue;
        const int k = comp_of(label, y * W + x, n);
        if (k < 0) continue;
        if (l) atomicMin(&boxes[4 * k + 0], x);
        if (t) atomicMin(&boxes[4 * k + 1], y);
        if (r) atomicMax(&boxes[4 * k + 2], x);
        if (b) atomicMax(&boxes[4 * k + 3], y);
    }
}
// test views: a packed mask as 0 / 255 bytes; the external-component mask (255 on every pixel of an external component)
__global__ void __launch_bounds__(256) ac_unpack_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ label, int H, int W, int WW,
                                                        uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int n = H * W;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        bool on = fg_at(bits, WW, x, y);
        if (on && label) on = comp_of(label, y * W + x, n) >= 0;
        dst[(size_t)y * W + x] = on ? 255 : 0;
    }
}

inline dim3 pix_grid(int W, int H, int rows_max = 4096) { return dim3((W + 255) / 256, H < rows_max ? H : rows_max); }

}  // namespace

hipError_t launch_ac_gray_blur(const uint8_t* src, int H, int W, size_t pitch, int channels, uint8_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(ac_gray_blur_kernel, pix_grid(W, H), dim3(256), 0, s, src, H, W, pitch, channels, dst);
    return hipGetLastError();
}
hipError_t launch_ac_cues(const uint8_t* e, int H, int W, const AcTaps& taps, uint16_t* rbox, uint16_t* rgau, uint8_t* part, uint8_t* grad,
                          unsigned int* hist, int* thr, hipStream_t s) {
    hipLaunchKernelGGL(ac_rows_kernel, pix_grid(W, H), dim3(256), 0, s, e, H, W, rbox, rgau, taps);
    // 128 row groups: the 512 per-workgroup histogram flushes stay a small fraction of the pass
    hipLaunchKernelGGL(ac_cols_kernel, pix_grid(W, H, 128), dim3(256), 0, s, e, rbox, rgau, H, W, taps, part, grad, hist);
    hipLaunchKernelGGL(ac_otsu_kernel, dim3(1), dim3(64), 0, s, hist, (unsigned long long)H * W, thr);
    return hipGetLastError();
}
hipError_t launch_ac_pack(const uint8_t* e, const uint8_t* part, const uint8_t* grad, const int* thr, int H, int W, int WW, uint32_t* bits, hipStream_t s) {
    hipLaunchKernelGGL(ac_pack_kernel, pix_grid(WW, H), dim3(256), 0, s, e, part, grad, thr, H, W, WW, bits);
    return hipGetLastError();
}
hipError_t launch_ac_pack_mask(const uint8_t* src, size_t pitch, int H, int W, int WW, uint32_t* bits, hipStream_t s) {
    hipLaunchKernelGGL(ac_pack_mask_kernel, pix_grid(WW, H), dim3(256), 0, s, src, pitch, H, W, WW, bits);
    return hipGetLastError();
}
hipError_t launch_ac_rect(const uint32_t* src, uint32_t* tmp, uint32_t* dst, int H, int W, int WW, int rx, int ry, int erode, const uint32_t* or_with,
                          hipStream_t s) {
    hipLaunchKernelGGL(ac_row_morph_kernel, pix_grid(WW, H), dim3(256), 0, s, src, tmp, H, W, WW, rx, erode);
    hipLaunchKernelGGL(ac_col_morph_kernel, pix_grid(WW, H), dim3(256), 0, s, tmp, dst, H, WW, ry, erode, or_with);
    return hipGetLastError();
}
hipError_t launch_ac_components(const uint32_t* bits, int H, int W, int WW, int* label, uint8_t* flag, int* count, int cap, int* boxes, hipStream_t s) {
    const dim3 g = pix_grid(W, H);
    hipLaunchKernelGGL(ac_ccl_init_kernel, g, dim3(256), 0, s, label, H, W);
    hipLaunchKernelGGL(ac_ccl_merge_kernel, g, dim3(256), 0, s, bits, label, H, W, WW);
    hipLaunchKernelGGL(ac_ccl_compress_kernel, g, dim3(256), 0, s, label, H, W);
    hipLaunchKernelGGL(ac_outer_kernel, g, dim3(256), 0, s, bits, label, flag, H, W, WW);
    hipLaunchKernelGGL(ac_external_kernel, g, dim3(256), 0, s, bits, label, flag, H, W, WW);
    hipLaunchKernelGGL(ac_enum_kernel, g, dim3(256), 0, s, label, flag, H, W, count, cap, boxes);
    hipLaunchKernelGGL(ac_boxes_kernel, g, dim3(256), 0, s, bits, label, H, W, WW, boxes);
    return hipGetLastError();
}
hipError_t launch_ac_unpack(const uint32_t* bits, const int* label, int H, int W, int WW, uint8_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(ac_unpack_kernel, pix_grid(W, H), dim3(256), 0, s, bits, label, H, W, WW, dst);
    return hipGetLastError();
}
