// What tiffdec.cpp and tiffdec.hip share: one file and one strip of a TIFF decode batch as the kernels read them, and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "png_inflate.h"
#include "tiff_codecs.h"
#include "tiff_fax.h"

enum { TD_RAW = 0, TD_PACKBITS = 1, TD_LZW = 2, TD_DEFLATE = 3, TD_FAX = 4 };

struct TdDesc {                  // one file
    uint8_t* stream;             // H * row_bytes bytes: the strips' output back to back, the predictor reversed in place
    const uint8_t* palette;      // 768 bytes (photometric 3)
    uint8_t* rgb;                // [H][W][3], rows pitch_rgb bytes apart
    uint8_t* gray;               // [H][W], rows pitch_gray bytes apart
    long long pitch_rgb, pitch_gray;
    int* status;                 // the file's: every strip ORs its bits in
    int W, H, bits, samples, photometric, predictor, row_bytes, reserved;
};

struct TdStrip {                 // one strip: a wavefront of td_strips
    const uint8_t* src;          // its stored bytes
    uint8_t* dst;                // into its file's stream
    int* file_status;
    int* status;                 // the strip's own word
    unsigned src_bytes, need;    // need = rows_in_strip * row_bytes
    int codec, reserved;
    int fax_width;               // TD_FAX: the row's pixels (need = rows_in_strip * ceil(fax_width / 8))
    int fax_mode;                // TD_FAX: the scheme (2, 3, 4) | T4Options << 8 | FillOrder << 16
};

// lds_bytes: what the batch's codecs need per wavefront (td_strips_lds); fax_width: the widest CCITT file of the batch, 0 for none
size_t td_strips_lds(bool any_lzw, bool any_deflate, int fax_width = 0);
hipError_t launch_td_strips(const TdStrip* s, int n, size_t lds_bytes, hipStream_t st);
hipError_t launch_td_predictor(const TdDesc* d, int n, int max_rows, hipStream_t st);
hipError_t launch_td_output(const TdDesc* d, int n, unsigned long long max_pixels, hipStream_t st);
