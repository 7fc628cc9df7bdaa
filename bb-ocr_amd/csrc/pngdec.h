// What pngdec.cpp and pngdec.hip share: one file of a PNG decode batch as the kernels read it, and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "png_inflate.h"

// the status word's bits behind png_inflate.h's PNGI_ERR_*
enum { PD_ERR_FILTER = 2048, PD_ERR_PALETTE = 4096 };
constexpr int PD_UNFILTER_THREADS = 512;      // rows of one band of pd_unfilter

struct PdDesc {
    const uint8_t* z;            // the zlib stream (the IDAT payloads back to back), z_bytes of them
    uint8_t* raw;                // H * (1 + row_bytes) bytes: the inflated stream, unfiltered in place
    const uint8_t* palette;      // 768 bytes (colour type 3)
    uint8_t* rgb;                // [H][W][3], rows pitch_rgb bytes apart
    uint8_t* gray;               // [H][W], rows pitch_gray bytes apart
    long long pitch_rgb, pitch_gray;
    int* status;
    unsigned z_bytes, raw_bytes;
    int W, H, depth, color_type, channels, bpp, row_bytes, palette_entries;
};

hipError_t launch_pd_inflate(const PdDesc* d, int n, hipStream_t s);
hipError_t launch_pd_unfilter(const PdDesc* d, int n, hipStream_t s);
hipError_t launch_pd_output(const PdDesc* d, int n, unsigned long long max_pixels, hipStream_t s);
