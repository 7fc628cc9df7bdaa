// What bmpdec.cpp and bmpdec.hip share: one file of a BMP decode batch as the kernel reads it, and the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct BdDesc {                  // one file
    const uint8_t* rows;         // H rows of `stride` bytes in stored order: file + data_offset
    const uint8_t* table;        // `colors` entries of `entry` bytes, B G R first: file + table_offset (1, 4, 8 bits)
    uint8_t* rgb;                // [H][W][3], rows pitch_rgb bytes apart
    uint8_t* gray;               // [H][W], rows pitch_gray bytes apart
    long long pitch_rgb, pitch_gray, stride;
    int W, H, bits, mode, colors, entry, top_down, r_at, g_at, b_at, six_bit_green, reserved;
};

hipError_t launch_bd_output(const BdDesc* d, int n, int max_rows, hipStream_t st);
