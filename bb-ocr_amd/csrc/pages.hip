// Pages of mixed shapes (bbocr_readtext_pages): ONE launch copies every page of a call -- whatever its shape, start address and row
// pitch -- tight into the staging buffers the detector and the recogniser read: RGB as [nb][H][W][3] per shape group, and the gray
// plane (the caller's, or cv2's BGR2GRAY of the RGB pixels as launch_gray derives it) as [H][W].
// Bandwidth-bound: a flat list of tiles of PK_TILE_PX pixels over all pages (a 5712x4284 photograph and a 300x200 crop in one call
// give 5,975 + 15 workgroups, not a grid sized by the larger page); a lane moves 16 pixels = 3 + 1 sixteen-byte stores where the page's
// pointers, pitches and staging offsets are multiples of 16, else the workgroup walks the tile byte by byte, lanes on consecutive bytes.
#include "common.h"
#include "kernels.h"

// which of a page's two copies may use 16-byte accesses.  A group of 16 pixels starts at a multiple of 16 in the page's raster order:
// with tight rows it may run over a row end (the bytes are contiguous); with a pitch it must not, so W % 16 == 0 is asked for as well.
// The destination is judged by its ADDRESS, staging base + offset: bbocr_op_pack_pages takes caller-owned staging buffers at any byte
int pack_page_vec(const PackPage& g, const uint8_t* rgb_staging, const uint8_t* gray_staging) {
    auto al = [](long long v) { return (v & 15) == 0; };
    auto at = [](const uint8_t* p) { return (long long)(uintptr_t)p; };
    auto rows_ok = [&](long long pitch, int px) { return pitch == (long long)g.W * px || (al(pitch) && g.W % 16 == 0); };
    const bool rgb = al(at(g.rgb)) && al(at(rgb_staging) + g.rgb_off) && rows_ok(g.rgb_pitch, 3);
    const bool gray = al(at(gray_staging) + g.gray_off) && (g.gray ? al(at(g.gray)) && rows_ok(g.gray_pitch, 1) : rgb);
    return (rgb ? 1 : 0) | (gray ? 2 : 0);
}

__global__ void __launch_bounds__(256) pack_pages_kernel(const PackPage* __restrict__ pages, int n, uint8_t* __restrict__ rgb_staging,
                                                         uint8_t* __restrict__ gray_staging) {
    // the page of this tile: the last one whose first tile is <= blockIdx.x (wave-uniform binary search over the table)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pages[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PackPage g = pages[lo];
    const int npx = g.H * g.W;                                    // < 2^30 (checked on the host)
    const int t0 = ((int)blockIdx.x - g.tile0) * PK_TILE_PX;
    if (t0 >= npx) return;
    const int t1 = t0 + PK_TILE_PX < npx ? t0 + PK_TILE_PX : npx;
    uint8_t* drgb = rgb_staging + g.rgb_off;
    uint8_t* dgray = gray_staging + g.gray_off;
    const int full = t0 + ((t1 - t0) & ~15);                      // pixels [t0, full): whole groups of 16; [full, t1): the page's last few
    const int p0 = t0 + (int)threadIdx.x * 16;
    const bool mine = p0 < full;
    const int row = p0 / g.W, col = p0 - row * g.W;               // (only used where the page's vec bits vouch for the group)
    u32x4 q[3];
    const bool vrgb = g.vec & 1, vgray = g.vec & 2;
    if (vrgb) {
        if (mine) {
            const u32x4* s = (const u32x4*)(g.rgb + (long long)row * g.rgb_pitch + (long long)col * 3);
            q[0] = s[0]; q[1] = s[1]; q[2] = s[2];
            u32x4* d = (u32x4*)(drgb + (long long)p0 * 3);
            d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
        }
    }
    // byte path of the RGB copy: the whole tile, or only the pixels behind the last whole group
    {
        const int b0 = (vrgb ? full : t0), nb = (t1 - b0) * 3;
        for (int i = threadIdx.x; i < nb; i += 256) {
            const int px = b0 + i / 3, ch = i - (i / 3) * 3;
            const int r = px / g.W, c = px - r * g.W;
            drgb[(long long)b0 * 3 + i] = g.rgb[(long long)r * g.rgb_pitch + (long long)c * 3 + ch];
        }
    }
    if (vgray) {
        if (mine) {
            u32x4 o;
            if (g.gray) {
                o = *(const u32x4*)(g.gray + (long long)row * g.gray_pitch + col);
            } else {                                              // from the 48 bytes in registers (vgray implies vrgb here)
                uint8_t b[48];
                __builtin_memcpy(b, q, 48);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned int w = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int px = j * 4 + k;
                        w |= (unsigned int)bgr2gray_px(b[px * 3], b[px * 3 + 1], b[px * 3 + 2]) << (8 * k);
                    }
                    o[j] = w;
                }
            }
            *(u32x4*)(dgray + p0) = o;
        }
    }
    {
        const int b0 = (vgray ? full : t0);
        for (int px = b0 + threadIdx.x; px < t1; px += 256) {
            const int r = px / g.W, c = px - r * g.W;
            uint8_t v;
            if (g.gray) {
                v = g.gray[(long long)r * g.gray_pitch + c];
            } else {
                const uint8_t* s = g.rgb + (long long)r * g.rgb_pitch + (long long)c * 3;
                v = bgr2gray_px(s[0], s[1], s[2]);
            }
            dgray[px] = v;
        }
    }
}

hipError_t launch_pack_pages(const PackPage* pages_dev, int n, int ntiles, uint8_t* rgb_staging, uint8_t* gray_staging, hipStream_t s) {
    if (n <= 0 || ntiles <= 0 || ntiles > PK_MAX_TILES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_pages_kernel, dim3(ntiles), dim3(256), 0, s, pages_dev, n, rgb_staging, gray_staging);
    return hipGetLastError();
}
