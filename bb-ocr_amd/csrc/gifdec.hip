// The device GIF decoder (bbocr_gif_decode): five launches over a batch, whatever mix of shapes, piece counts and code sizes it holds
// (gifdec.h, gif_lzw.h).
//   gd_scan      one wavefront per file: from the last clear the lanes compute the positions of the next 64 codes in closed form, read
//                their codes and ballot for the first clear or end code (or the payload's end) -> the piece table.
//   gd_lengths   one wavefront per piece: gif_lzw.h's walk with the entries' lengths alone in LDS (8 KB) -> the piece's decoded byte count,
//                clipped at w * h, and its error bits.  Every lane runs the walk on the same values.
//   gd_offsets   one wavefront per file: a wave scan over the lengths -> each piece's offset into the index stream, and the file's status.
//   gd_decode    one wavefront per piece: the walk again with (offset, length) entries in LDS (32 KB), match copies shared out among the
//                lanes into the file's index stream at the piece's offset, clipped at w * h.
//   gd_output    fully parallel: de-interlace, placement on the canvas, table lookup, both planes by reader.decode_file's rule.
// Order comes from the launch boundaries alone: no workgroup waits for another.  A file whose status word is not 0 is skipped by the later
// launches.  No launch writes outside the file's own tables, its stream or its destinations' rows.
#include "gifdec.h"
#include "wave_copy.h"

namespace {

constexpr int kWave = 64;

struct GiflWave : WaveCopy {                              // a workgroup of ONE wavefront: wave_copy.h's output policy, and the scan's ballot
    template <typename F> __device__ static void first_stop(F&& f, int& lane, int& end) {
        const int c = f((int)threadIdx.x);
        const unsigned long long stops = __ballot(c >= 0);
        if (!stops) {
            lane = -1;
            return;
        }
        lane = __ffsll((long long)stops) - 1;
        end = __shfl(c, lane);
    }
    __device__ static bool leader() { return threadIdx.x == 0; }
};

__device__ inline uint64_t piece_bit(const GiflPiece& p) { return ((uint64_t)p.bit_hi << 32) | p.bit_lo; }

__global__ __launch_bounds__(kWave) void gd_scan(const GdDesc* descs) {
    const GdDesc& d = descs[blockIdx.x];
    uint32_t count = 0;
    const int err = gifl_scan<GiflWave>(d.payload, d.nbits, d.m, d.pieces, d.cap, &count);
    if (threadIdx.x == 0) {
        d.head[0] = count;
        d.head[1] = (uint32_t)err;
        d.head[2] = d.head[3] = 0;
    }
}

__global__ __launch_bounds__(kWave) void gd_lengths(const GdDesc* descs) {
    __shared__ uint16_t len[GIFL_ENTRIES];
    const GdDesc& d = descs[blockIdx.y];
    const uint32_t count = d.head[0];
    for (uint32_t p = blockIdx.x; p < count; p += gridDim.x) {
        const GiflPiece pc = d.pieces[p];
        uint32_t produced = 0;
        const int err = gifl_piece<GiflWave, false>(d.payload, d.nbits, d.m, piece_bit(pc), pc.codes, nullptr, d.need, GiflLengths{len}, &produced);
        if (threadIdx.x == 0) {
            d.lengths[p] = produced;
            d.errors[p] = err;
        }
    }
}

__global__ __launch_bounds__(kWave) void gd_offsets(const GdDesc* descs) {
    const GdDesc& d = descs[blockIdx.x];
    const uint32_t count = d.head[0];
    const int lane = (int)threadIdx.x;
    const unsigned long long need = d.need;
    unsigned long long cum = 0;
    int status = (int)d.head[1];
    bool done = false;
    for (uint32_t base = 0; base < count; base += kWave) {
        const uint32_t i = base + (uint32_t)lane;
        const bool in = i < count;
        const unsigned long long len = in ? d.lengths[i] : 0;
        unsigned long long incl = len;
        for (int step = 1; step < kWave; step <<= 1) {                     // the wave's inclusive scan
            const unsigned long long up = __shfl_up(incl, step);
            if (lane >= step) incl += up;
        }
        const unsigned long long before = cum + incl - len;
        if (in) d.offsets[i] = (uint32_t)(before < need ? before : need);
        const bool full = in && before + len >= need;
        int bad = 0;                                                       // what ends the file here, if the frame is not full by then
        if (in && !full) bad = d.errors[i] ? d.errors[i] : (d.pieces[i].end != GIFL_END_CLEAR ? (int)GIFL_ERR_SHORT : 0);
        const unsigned long long stops = __ballot(full || bad != 0);
        if (!done && !status && stops) {
            const int first = __ffsll((long long)stops) - 1;
            const int b = __shfl(bad, first);
            if (b) status |= b;
            else done = true;
        }
        cum += __shfl(incl, kWave - 1);
    }
    if (!done && !status) status |= GIFL_ERR_SHORT;
    if (lane == 0) {
        d.offsets[count] = (uint32_t)(cum < need ? cum : need);
        *d.status = status;
    }
}

__global__ __launch_bounds__(kWave) void gd_decode(const GdDesc* descs) {
    __shared__ GiflEntry entries[GIFL_ENTRIES];
    const GdDesc& d = descs[blockIdx.y];
    if (*d.status) return;
    const uint32_t count = d.head[0];
    for (uint32_t p = blockIdx.x; p < count; p += gridDim.x) {
        const uint32_t off = d.offsets[p];
        if (off >= d.need) return;                                         // the frame is full: so it is for every later piece
        const GiflPiece pc = d.pieces[p];
        uint32_t produced = 0;
        gifl_piece<GiflWave, true>(d.payload, d.nbits, d.m, piece_bit(pc), pc.codes, d.stream + off, d.need - off, GiflStrings{entries}, &produced);
        __syncthreads();                                                   // the table is the next piece's
    }
}

__device__ inline int stored_row(int y, int h, int interlace) {
    if (!interlace) return y;
    const int n0 = (h + 7) / 8, n1 = (h + 3) / 8, n2 = (h + 1) / 4;
    if ((y & 7) == 0) return y >> 3;
    if ((y & 7) == 4) return n0 + (y >> 3);
    if ((y & 3) == 2) return n0 + n1 + (y >> 2);
    return n0 + n1 + n2 + (y >> 1);
}

__global__ __launch_bounds__(256) void gd_output(const GdDesc* descs) {
    const GdDesc& d = descs[blockIdx.y];
    if (*d.status) return;
    const size_t total = (size_t)d.cw * (size_t)d.ch;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (size_t)d.cw), x = (int)(i - (size_t)y * (size_t)d.cw);
        const int fx = x - d.x0, fy = y - d.y0;
        int v = d.background;
        if (fx >= 0 && fx < d.w && fy >= 0 && fy < d.h) v = d.stream[(size_t)stored_row(fy, d.h, d.interlace) * (size_t)d.w + (size_t)fx];
        const int r = d.table[3 * v], g = d.table[3 * v + 1], b = d.table[3 * v + 2];
        uint8_t* o = d.rgb + (size_t)y * (size_t)d.pitch_rgb + 3 * (size_t)x;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
        d.gray[(size_t)y * (size_t)d.pitch_gray + (size_t)x] = (uint8_t)(d.mode_l ? v : (9797 * r + 19234 * g + 3737 * b) >> 15);
    }
}

unsigned piece_blocks(size_t max_cap) { return (unsigned)(max_cap < 1 ? 1 : (max_cap > 1024 ? 1024 : max_cap)); }

// one launch per 32768 files: the grid's second dimension holds at most 65535
template <typename K> hipError_t per_file_rows(K kernel, unsigned blocks_x, unsigned threads, const GdDesc* d, int n, hipStream_t st) {
    for (int at = 0; at < n; at += 32768) {
        const int m = n - at < 32768 ? n - at : 32768;
        hipLaunchKernelGGL(kernel, dim3(blocks_x, (unsigned)m), dim3(threads), 0, st, d + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_gd_scan(const GdDesc* d, int n, hipStream_t st) {
    hipLaunchKernelGGL(gd_scan, dim3((unsigned)n), dim3(kWave), 0, st, d);
    return hipGetLastError();
}

hipError_t launch_gd_lengths(const GdDesc* d, int n, size_t max_cap, hipStream_t st) { return per_file_rows(gd_lengths, piece_blocks(max_cap), kWave, d, n, st); }

hipError_t launch_gd_offsets(const GdDesc* d, int n, hipStream_t st) {
    hipLaunchKernelGGL(gd_offsets, dim3((unsigned)n), dim3(kWave), 0, st, d);
    return hipGetLastError();
}

hipError_t launch_gd_decode(const GdDesc* d, int n, size_t max_cap, hipStream_t st) { return per_file_rows(gd_decode, piece_blocks(max_cap), kWave, d, n, st); }

hipError_t launch_gd_output(const GdDesc* d, int n, unsigned long long max_pixels, hipStream_t st) {
    const unsigned long long blocks = (max_pixels + 1023) / 1024;        // four pixels per thread, more in the largest files
    return per_file_rows(gd_output, (unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)), 256, d, n, st);
}
