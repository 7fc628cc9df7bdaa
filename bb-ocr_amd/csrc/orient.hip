// page_orient: one uint8 page re-written in one of the eight EXIF orientations (ImageOps.exif_transpose = OpenCV's ExifTransform), with the
// colour conversion cv2.imread implies on the way (GRAY replicated, RGB <-> BGR, libjpeg's YCbCr -> RGB).  An HBM-bound byte kernel:
//   A  a workgroup owns an ORIENT_TILE x ORIENT_TILE pixel tile.  It reads the tile's bytes along SOURCE rows as the aligned dwords that
//      cover them (a dword that reaches over the start or end of the source row is assembled from its valid bytes) into LDS, a source
//      row per LDS row, each shifted by its global address & 3 so that an aligned global dword is an aligned LDS dword;
//   B  one pixel per thread is read from that image, converted and written where it belongs in the DESTINATION tile, a destination row
//      per LDS row, shifted by the destination row's global address & 3.  Both LDS pitches are an odd number of dwords (65 and 49): the
//      64 lanes of a transposing orientation, which write one column, fall on distinct banks (17 * lane mod 32);
//   C  the destination tile leaves along DESTINATION rows as whole aligned dwords; the dwords that the tile shares with its neighbours
//      (3-byte pixels: a tile's row starts and ends on any byte) are written byte by byte, only the bytes the tile owns.
// No thread touches a column of global memory, in any orientation.  The LDS traffic is a few per cent of its rate (3 one-byte stores
// per pixel); what the kernel costs is its global traffic: 64 x 4 B in and 64 x 3 B out per tile row, cut at both ends by 128-byte lines.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int OR_T = ORIENT_TILE;
constexpr int OR_RAW_PITCH = OR_T * 4 + 4;                      // 3 bytes of shift + 64 four-byte pixels, rounded up: 65 dwords
constexpr int OR_OUT_PITCH = OR_T * 3 + 4;                      // 3 + 192: 49 dwords

struct OrientArgs {
    const uint8_t* src;
    uint8_t* dst;
    size_t spitch, dpitch;
    int H, W;                                                   // the SOURCE page
    int swap, fx, fy;                                           // rows <-> columns, then mirror the destination's columns / rows
    int tiles_minor;                                            // tiles along the DESTINATION's rows: consecutive workgroups are neighbours there
};

template <int LAYOUT, int DST> __global__ void __launch_bounds__(256) page_orient_kernel(const OrientArgs a) {
    constexpr int SB = page_px_bytes(LAYOUT), DC = page_px_bytes(DST);
    __shared__ __attribute__((aligned(16))) uint8_t raw[OR_T * OR_RAW_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t out[OR_T * OR_OUT_PITCH];
    const int t = threadIdx.x;
    const int major = (int)blockIdx.x / a.tiles_minor, minor = (int)blockIdx.x - major * a.tiles_minor;
    // the tile in the source: `minor` runs along the destination's rows, i.e. along source rows, or down source columns when swapped
    const int x0 = (a.swap ? major : minor) * OR_T, y0 = (a.swap ? minor : major) * OR_T;
    const int tw = min(OR_T, a.W - x0), th = min(OR_T, a.H - y0);
    const int xb = x0 * SB, span = tw * SB, rowbytes = a.W * SB;
    const uint8_t* s0 = a.src + (size_t)y0 * a.spitch;
    const int sa0 = (int)(((size_t)s0 + (size_t)xb) & 3), sp3 = (int)(a.spitch & 3);

    // ---- A: the tile's source bytes, aligned dword by aligned dword.  Every load of a thread is issued before the first LDS store, so that
    // a workgroup keeps its whole tile in flight (one load at a time per wave leaves the memory latency exposed)
    const int ndw = (span + 6) >> 2;                            // dwords that cover shift + span, for every shift
    constexpr int PER_THREAD = (OR_T * ((OR_T * SB + 6) >> 2) + 255) / 256;
    unsigned v[PER_THREAD];
    bool edge = false;                                          // this thread holds a dword that reaches over the source row
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const int idx = t + 256 * i, r = idx / ndw, k = idx - r * ndw;
        const int o = xb - ((sa0 + r * sp3) & 3) + 4 * k;       // byte of the source row this dword starts at (-3 .. )
        const bool full = r < th && o >= 0 && o + 4 <= rowbytes && o < xb + span;
        v[i] = full ? *(const unsigned*)(s0 + (size_t)r * a.spitch + o) : 0u;
        edge |= r < th && o < xb + span && !full;
    }
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const int idx = t + 256 * i, r = idx / ndw, k = idx - r * ndw;
        if (r < th) *(unsigned*)(raw + r * OR_RAW_PITCH + 4 * k) = v[i];
    }
    if (edge) {                                                 // first / last dword of a row of the IMAGE: its valid bytes only
        for (int i = 0; i < PER_THREAD; ++i) {
            const int idx = t + 256 * i, r = idx / ndw, k = idx - r * ndw;
            const int o = xb - ((sa0 + r * sp3) & 3) + 4 * k;
            if (r >= th || o >= xb + span || (o >= 0 && o + 4 <= rowbytes)) continue;
            const uint8_t* row = s0 + (size_t)r * a.spitch;
            unsigned w = 0;
            for (int b = 0; b < 4; ++b)
                if (o + b >= 0 && o + b < rowbytes) w |= (unsigned)row[o + b] << (8 * b);
            *(unsigned*)(raw + r * OR_RAW_PITCH + 4 * k) = w;
        }
    }
    __syncthreads();

    // ---- B: convert, and place every pixel in the destination tile
    const int Hd = a.swap ? a.W : a.H, Wd = a.swap ? a.H : a.W;
    const int u0 = a.swap ? x0 : y0, v0 = a.swap ? y0 : x0;
    const int nr = a.swap ? tw : th, nc = a.swap ? th : tw;     // the destination tile: rows, pixels per row
    const int dy0 = a.fy ? Hd - (u0 + nr) : u0, dx0 = a.fx ? Wd - (v0 + nc) : v0;
    uint8_t* d0 = a.dst + (size_t)dy0 * a.dpitch + (size_t)dx0 * DC;
    const int da0 = (int)((size_t)d0 & 3), dp3 = (int)(a.dpitch & 3);
#pragma unroll 4
    for (int p = t; p < OR_T * OR_T; p += 256) {
        const int r = p / OR_T, c = p % OR_T;
        if (r >= th || c >= tw) continue;
        const uint8_t* q = raw + r * OR_RAW_PITCH + ((sa0 + r * sp3) & 3) + c * SB;
        uint8_t px[3];                                          // R, G, B (gray: the sample three times)
        if (LAYOUT == PAGE_GRAY) {
            px[0] = px[1] = px[2] = q[0];
        } else if (LAYOUT == PAGE_RGB) {
            px[0] = q[0]; px[1] = q[1]; px[2] = q[2];
        } else if (LAYOUT == PAGE_BGR) {
            px[0] = q[2]; px[1] = q[1]; px[2] = q[0];
        } else {
            jpeg_ycc_to_rgb(q[0], q[1], q[2], px);
        }
        const int lu = a.swap ? c : r, lv = a.swap ? r : c;
        const int lr = a.fy ? nr - 1 - lu : lu, lc = a.fx ? nc - 1 - lv : lv;
        uint8_t* w = out + lr * OR_OUT_PITCH + ((da0 + lr * dp3) & 3) + lc * DC;
        if (DST == PAGE_GRAY) {
            w[0] = px[0];
        } else if (DST == PAGE_RGB) {
            w[0] = px[0]; w[1] = px[1]; w[2] = px[2];
        } else {
            w[0] = px[2]; w[1] = px[1]; w[2] = px[0];
        }
    }
    __syncthreads();

    // ---- C: the destination tile, aligned dword by aligned dword; shared dwords byte by byte
    const int L = nc * DC, ndo = (L + 6) >> 2;
#pragma unroll 4
    for (int idx = t; idx < nr * ndo; idx += 256) {
        const int r = idx / ndo, k = idx - r * ndo;
        const int ad = (da0 + r * dp3) & 3, lo = 4 * k;         // the tile's bytes are [ad, ad + L) of this LDS row
        if (lo >= ad + L) continue;
        const unsigned v = *(const unsigned*)(out + r * OR_OUT_PITCH + lo);
        uint8_t* g = d0 + (size_t)r * a.dpitch + (lo - ad);
        if (lo >= ad && lo + 4 <= ad + L) {
            *(unsigned*)g = v;
        } else {
            for (int b = 0; b < 4; ++b)
                if (lo + b >= ad && lo + b < ad + L) g[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

template <int LAYOUT> hipError_t orient_dst(const OrientArgs& a, int dst_layout, unsigned grid, hipStream_t s) {
    if (dst_layout == PAGE_BGR) hipLaunchKernelGGL((page_orient_kernel<LAYOUT, PAGE_BGR>), dim3(grid), dim3(256), 0, s, a);
    else if (dst_layout == PAGE_RGB) hipLaunchKernelGGL((page_orient_kernel<LAYOUT, PAGE_RGB>), dim3(grid), dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

bool page_orient_pair_ok(int layout, int dst_layout) {
    if (layout < PAGE_GRAY || layout > PAGE_YCC3) return false;
    return dst_layout == PAGE_BGR || dst_layout == PAGE_RGB || (dst_layout == PAGE_GRAY && layout == PAGE_GRAY);
}

hipError_t launch_page_orient(const uint8_t* src, int H, int W, size_t pitch, int layout, int orientation, int dst_layout, uint8_t* dst,
                              size_t dst_pitch, hipStream_t s) {
    if (!page_orient_pair_ok(layout, dst_layout) || orientation < 1 || orientation > 8 || H < 1 || W < 1) return hipErrorInvalidValue;
    // orientation -> (swap, mirror columns, mirror rows) of the table in bbocr.h: 2 = mirror columns, 3 = both, 4 = mirror rows, 5 = transpose,
    // 6 = transpose + mirror columns (90 degrees clockwise), 7 = transpose + both, 8 = transpose + mirror rows
    static const int kFx[9] = {0, 0, 1, 1, 0, 0, 1, 1, 0}, kFy[9] = {0, 0, 0, 1, 1, 0, 0, 1, 1};
    OrientArgs a{src, dst, pitch, dst_pitch, H, W, orientation >= 5, kFx[orientation], kFy[orientation], 0};
    const int tiles_x = (W + OR_T - 1) / OR_T, tiles_y = (H + OR_T - 1) / OR_T;
    a.tiles_minor = a.swap ? tiles_y : tiles_x;
    const unsigned grid = (unsigned)tiles_x * (unsigned)tiles_y;
    switch (layout) {
        case PAGE_GRAY:
            if (dst_layout == PAGE_GRAY) {
                hipLaunchKernelGGL((page_orient_kernel<PAGE_GRAY, PAGE_GRAY>), dim3(grid), dim3(256), 0, s, a);
                return hipGetLastError();
            }
            return orient_dst<PAGE_GRAY>(a, dst_layout, grid, s);
        case PAGE_BGR: return orient_dst<PAGE_BGR>(a, dst_layout, grid, s);
        case PAGE_RGB: return orient_dst<PAGE_RGB>(a, dst_layout, grid, s);
        case PAGE_YCC4: return orient_dst<PAGE_YCC4>(a, dst_layout, grid, s);
        default: return orient_dst<PAGE_YCC3>(a, dst_layout, grid, s);
    }
}
