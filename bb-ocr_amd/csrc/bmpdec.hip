// The device BMP decoder (bbocr_bmp_decode): ONE launch over a batch, whatever mix of shapes and depths it holds (bmpdec.h).  bd_output:
// a workgroup per row (blockIdx.x strides over the rows, the lanes over the row's pixels: no division per pixel); the lanes unpack bits, nibbles, bytes, 16-bit words or 3- and 4-byte groups from the stored row -- the rows of a
// bottom-up file are read last first --, look an index up in the file's own table (an index without an entry: black) and write both planes
// by reader.decode_file's rule.  Every byte read lies inside the file: bbocr_host_bmp_plan has checked the table and the rows against its
// length.  No launch writes outside a destination's rows.
#include "bmpdec.h"

namespace {

__global__ __launch_bounds__(256) void bd_output(const BdDesc* descs) {
    const BdDesc& d = descs[blockIdx.y];
    for (size_t y = blockIdx.x; y < (size_t)d.H; y += gridDim.x) {
        const uint8_t* row = d.rows + (d.top_down ? y : (size_t)d.H - 1 - y) * (size_t)d.stride;
        uint8_t* rgb_row = d.rgb + y * (size_t)d.pitch_rgb;
        uint8_t* gray_row = d.gray + y * (size_t)d.pitch_gray;
        for (size_t x = threadIdx.x; x < (size_t)d.W; x += 256) {
            int r, g, b, gray = -1;
            if (d.bits <= 8) {
                const int v = d.bits == 8 ? row[x] : (d.bits == 4 ? (row[x >> 1] >> ((x & 1) ? 0 : 4)) & 15 : (row[x >> 3] >> (7 - (int)(x & 7))) & 1);
                if (d.mode == 0) {
                    r = g = b = 0;
                    if (v < d.colors) {
                        const uint8_t* e = d.table + (size_t)v * (size_t)d.entry;
                        b = e[0], g = e[1], r = e[2];
                    }
                } else {
                    r = g = b = gray = d.mode == 1 ? v * 255 : v;              // Pillow's modes 1 and L: the gray plane is the sample
                }
            } else if (d.bits == 16) {
                const int px = row[2 * x] | (row[2 * x + 1] << 8);
                b = (px & 31) * 255 / 31;
                g = d.six_bit_green ? ((px >> 5) & 63) * 255 / 63 : ((px >> 5) & 31) * 255 / 31;
                r = ((px >> (d.six_bit_green ? 11 : 10)) & 31) * 255 / 31;
            } else {
                const uint8_t* p = row + x * (size_t)(d.bits >> 3);
                r = p[d.r_at], g = p[d.g_at], b = p[d.b_at];
            }
            if (gray < 0) gray = (9797 * r + 19234 * g + 3737 * b) >> 15;
            uint8_t* o = rgb_row + 3 * x;
            o[0] = (uint8_t)r;
            o[1] = (uint8_t)g;
            o[2] = (uint8_t)b;
            gray_row[x] = (uint8_t)gray;
        }
    }
}

}  // namespace

hipError_t launch_bd_output(const BdDesc* d, int n, int max_rows, hipStream_t st) {
    const int blocks = max_rows;                                         // a workgroup per row of the tallest file, at most 16384
    for (int at = 0; at < n; at += 32768) {                              // the grid's second dimension holds at most 65535 files
        const int m = n - at < 32768 ? n - at : 32768;
        hipLaunchKernelGGL(bd_output, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)), (unsigned)m), dim3(256), 0, st, d + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
