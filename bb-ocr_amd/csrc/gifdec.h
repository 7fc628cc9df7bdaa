// What gifdec.cpp and gifdec.hip share: one file of a GIF decode batch as the kernels read it, and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gif_lzw.h"

struct GdDesc {                  // one file
    const uint8_t* payload;      // the de-framed code stream
    const uint8_t* table;        // 768 bytes: the RGB plane's lookup
    uint32_t* head;              // [4]: pieces found, the scan's error bits, 0, 0 -- followed by the piece table
    GiflPiece* pieces;           // [cap]
    uint32_t* lengths;           // [cap]: each piece's decoded bytes, clipped at need
    int* errors;                 // [cap]
    uint32_t* offsets;           // [cap + 1]: the exclusive prefix sum, saturated at need; the last: the total
    uint8_t* stream;             // need bytes: the indices in stored row order
    uint8_t* rgb;                // [canvas_h][canvas_w][3], rows pitch_rgb bytes apart
    uint8_t* gray;               // [canvas_h][canvas_w], rows pitch_gray bytes apart
    long long pitch_rgb, pitch_gray;
    int* status;                 // the file's: GIFL_ERR_* bits
    unsigned long long nbits;    // 8 * payload bytes
    uint32_t cap, need;          // need = w * h
    int m, x0, y0, w, h, cw, ch, interlace, background, mode_l;
};

hipError_t launch_gd_scan(const GdDesc* d, int n, hipStream_t st);
hipError_t launch_gd_lengths(const GdDesc* d, int n, size_t max_cap, hipStream_t st);
hipError_t launch_gd_offsets(const GdDesc* d, int n, hipStream_t st);
hipError_t launch_gd_decode(const GdDesc* d, int n, size_t max_cap, hipStream_t st);
hipError_t launch_gd_output(const GdDesc* d, int n, unsigned long long max_pixels, hipStream_t st);
