// Baseline JPEG decoding on the device (SOF0, Huffman, one interleaved scan, YCbCr 4:2:0, 4:4:4, 4:2:2, 4:4:0 or grey), to the bit of
// libjpeg-turbo: the entropy stage by speculative decoding with self-synchronisation (Weissenberger & Schmidt), then thumb.hip's decoder
// half (jpeg_dev.h).  The first three kernels are jpeg_spec.h's passes, which jpegprog.hip runs too, over this file's jd_run (JdCodec).
//   jd_sync     one lane per S-bit subsequence: decode from the assumed state (block 0 of the MCU, coefficient 0), then take the left
//               neighbour's exit state and decode again until no state of the workgroup changes; launched once more per workgroup
//               a segment spans, a launch returning at once when the launch before it changed nothing
//   jd_scan     exclusive scan of the block counts: first output block of every subsequence
//   jd_write    decode from the exact entry states into the zeroed coefficient buffer (natural order); checks what the file promised
//   jd_dc       per component and restart segment: running sum of the DC differences
//   jd_idct     dequantise + jidctint.c (8 x 8) or jidctred.c (4 x 4, 2 x 2, 1 x 1: a decode at scale 1/2, 1/4 or 1/8, Pillow's draft) per
//               block into the component planes
//   jd_output   the chroma planes brought to the output's size (fancy h2v2, h2v1, h1v2, replication, or as they are) -> YCbCr triples
//               (3 or 4 bytes per pixel) or the grey plane, into the caller's tensor
// The last two run once per requested output over the same coefficients.  What a scale and a sampling mean for them -- each component's
// block edge, its place in the MCU, its plane and the upsampling rule -- is data: JpegDesc::comp, filled by jpegdec.cpp's jpeg_geometry.
// An MCU holds hs x vs luma blocks (row after row), then one Cb and one Cr block: 2 x 2 for 4:2:0, 1 x 1 / 2 x 1 / 1 x 2 for the others.
// The bytes are untrusted: every stream read is clamped to its segment (past the end: 1-bits), every store is index-checked, every loop
// has a trip count fixed by the host's plan (S, lanes per workgroup, items per segment).
#include "common.h"
#include "jpeg_spec.h"
#include "jpeg_dev.h"

namespace {

// 16 bits at bit p of the segment whose bytes are [b0, b1); past the end: ones
__device__ __forceinline__ unsigned jd_peek16(const uint8_t* __restrict__ data, unsigned b0, unsigned b1, unsigned p) {
    const unsigned k = p >> 3;
    unsigned w = 0;
    for (int i = 0; i < 3; ++i) {
        const unsigned a = k + i;
        w = (w << 8) | ((a >= b0 && a < b1) ? (unsigned)data[a] : 0xFFu);
    }
    return (w >> (8 - (p & 7))) & 0xFFFFu;
}

// component of block b of an MCU
__device__ __forceinline__ int jd_comp(const JpegDesc& d, int b) {
    const int nl = d.hs * d.vs;
    return d.bpm == 1 ? 0 : (b < nl ? 0 : b - nl + 1);
}

// Decode from st while its bit is before `end` and fewer than max_blocks blocks are complete.  Returns the blocks completed; *invalid: a
// look-ahead without a code was met (the state's bit is then `end`).  coef != null: coefficients of block first_block + n are stored
// (DC terms as differences).  At most S + 32 symbols: each takes at least one bit.
__device__ int jd_run(const JpegDesc& d, const JpegHuff* T, unsigned b0, unsigned b1, JpegState& st, unsigned end, int max_blocks, short* coef,
                      int first_block, bool* invalid) {
    unsigned p = st.p;
    int b = st.b, z = st.z, n = 0;
    *invalid = false;
    const uint8_t* __restrict__ data = d.data;
    for (int it = 0; it < d.S + 32 && p < end && n < max_blocks; ++it) {
        const int c = jd_comp(d, b);
        const int ti = z == 0 ? (c == 0 ? d.tab_dc[0] : (c == 1 ? d.tab_dc[1] : d.tab_dc[2])) : (c == 0 ? d.tab_ac[0] : (c == 1 ? d.tab_ac[1] : d.tab_ac[2]));
        const JpegHuff& H = T[ti & 3];
        const unsigned v = jd_peek16(data, b0, b1, p);
        int len = 0, sym = 0;
        const unsigned e = H.look[v >> 7];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255);
        } else {
            for (int l = 10; l <= 16; ++l) {
                const int code = (int)(v >> (16 - l));
                if (code <= H.maxcode[l]) {
                    len = l;
                    sym = H.val[(code + H.valoff[l]) & 255];
                    break;
                }
            }
            if (!len) {
                *invalid = true;
                p = end;
                break;
            }
        }
        p += len;
        int sz = sym & 15;
        bool done = false;
        if (z != 0) {
            const int r = sym >> 4;
            if (sz == 0) {                                     // ZRL skips 16 zeros, every other run length ends the block
                z = r == 15 ? z + 16 : 64;
                done = true;
            } else {
                z += r;
            }
        }
        if (!done) {
            int val = 0;
            if (sz) {
                const int bits = (int)(jd_peek16(data, b0, b1, p) >> (16 - sz));
                p += sz;
                val = bits >= (1 << (sz - 1)) ? bits : bits - (1 << sz) + 1;
            }
            const int blk = first_block + n;
            if (coef && z <= 63 && (unsigned)blk < (unsigned)d.nblocks) coef[(size_t)blk * 64 + JPEG_ZZ[z]] = (short)val;
            z += 1;
        }
        if (z > 63) {
            z = 0;
            b = b + 1 == d.bpm ? 0 : b + 1;
            n += 1;
        }
    }
    st.p = p;
    st.b = b;
    st.z = z;
    return n;
}

// The baseline scan as jpeg_spec.h's passes see it: units are MCUs of bpm blocks, a segment starts at coefficient 0 of block 0 and
// must end there, the write pass records the first block of every subsequence (stage 0 of bbocr_op_jpeg_stage).
struct JdCodec {
    using Desc = JpegDesc;
    struct Lds { JpegHuff* T; };                                 // T[4] of the kernel's LDS
    static __device__ __forceinline__ bool cut(const JpegDesc&) { return true; }
    static __device__ __forceinline__ void load(const JpegDesc& d, const Lds& lds, int t, int nt) {
        const int* src = (const int*)d.huff;
        int* dst = (int*)lds.T;
        for (int i = t; i < (int)(4 * sizeof(JpegHuff) / 4); i += nt) dst[i] = src[i];
        __syncthreads();
    }
    static __device__ __forceinline__ int unit_blocks(const JpegDesc& d) { return d.bpm; }
    static __device__ __forceinline__ int units(const JpegDesc& d) { return d.nmcu; }
    static __device__ __forceinline__ JpegState start(const JpegDesc&, unsigned p) { return JpegState{p, 0, 0}; }
    static __device__ __forceinline__ int run(const JpegDesc& d, const Lds& lds, int, const JpegSub& s, JpegState& st, int max_blocks, bool store,
                                              long long first, bool* invalid, bool* over) {
        *over = false;
        return jd_run(d, lds.T, s.b0, s.b1, st, s.end, max_blocks, store ? d.coef : nullptr, (int)min(first, (long long)d.nblocks), invalid);
    }
    static __device__ __forceinline__ bool at_end(const JpegDesc&, const JpegState& st, const JpegSub&) { return st.b == 0 && st.z == 0; }
    static __device__ __forceinline__ void note_first(const JpegDesc& d, int i, long long first) { d.first[i] = (int)min(first, (long long)d.nblocks); }
};

__global__ void __launch_bounds__(JD_LANES) jd_sync_kernel(const JpegDesc* __restrict__ descs, int pass) {
    __shared__ JpegHuff T[4];
    __shared__ unsigned long long ex[JD_LANES];
    const JpegDesc d = descs[blockIdx.y];
    jpeg_sync_pass<JdCodec>(d, {T}, ex, pass);
}

// one workgroup per file
__global__ void __launch_bounds__(256) jd_scan_kernel(const JpegDesc* __restrict__ descs) {
    __shared__ long long sh[256];
    const JpegDesc d = descs[blockIdx.x];
    jpeg_prefix_pass<JdCodec>(d, sh);
}

__global__ void __launch_bounds__(JD_LANES) jd_write_kernel(const JpegDesc* __restrict__ descs) {
    __shared__ JpegHuff T[4];
    const JpegDesc d = descs[blockIdx.y];
    jpeg_write_pass<JdCodec>(d, {T});
}

// one workgroup per (segment, component, file): inclusive sum of the DC differences in MCU order
__global__ void __launch_bounds__(256) jd_dc_kernel(const JpegDesc* __restrict__ descs) {
    __shared__ int sh[256];
    const JpegDesc d = descs[blockIdx.z];
    const int seg = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    if (seg >= d.nseg || c >= d.ncomp) return;
    const int m0 = seg * d.ri, nm = min(d.ri, d.nmcu - m0);
    const int nl = d.hs * d.vs, per = (d.ncomp == 3 && c == 0) ? nl : 1;
    const int items = nm * per;
    int carry = 0;
    for (int base = 0; base < items; base += 256 * 8) {
        int v[8], sum = 0;
        for (int e = 0; e < 8; ++e) {
            const int k = base + t * 8 + e;
            int x = 0;
            if (k < items) {
                const int blk = (m0 + k / per) * d.bpm + (d.ncomp == 3 ? (c == 0 ? k % per : nl - 1 + c) : 0);
                if ((unsigned)blk < (unsigned)d.nblocks) x = d.coef[(size_t)blk * 64];
            }
            sum += x;
            v[e] = sum;
        }
        sh[t] = sum;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int a = t >= o ? sh[t - o] : 0;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        const int excl = carry + sh[t] - sum;
        for (int e = 0; e < 8; ++e) {
            const int k = base + t * 8 + e;
            if (k < items) {
                const int blk = (m0 + k / per) * d.bpm + (d.ncomp == 3 ? (c == 0 ? k % per : nl - 1 + c) : 0);
                if ((unsigned)blk < (unsigned)d.nblocks) d.coef[(size_t)blk * 64] = (short)(excl + v[e]);
            }
        }
        carry += sh[255];
        __syncthreads();
    }
}

// A block's 8 x 8 words in LDS with rows JD_ROW words apart and blocks JD_BLK: a half-wave's 4 blocks x 8 lanes then touch 32 different
// banks ((8 b + l) mod 32 in the column pass, (8 b + 9 l) mod 32 in the row pass and the dequantising stores); rows 8 words apart would
// put the 4 blocks of a half-wave on one bank.
constexpr int JD_ROW = 9, JD_BLK = 72;

// Eight blocks per wavefront, eight lanes per block (a row, then a column, then a row again: thumb.hip's order).  A lane dequantises one row
// of coefficients (one 16-byte load), runs one column of the first pass (the columns the second pass never reads are skipped, as in
// jidctred.c), then the lanes below the block's edge n run one row each of the second pass and store it as one word of n bytes.  jdmaster.c
// gives every component its own DCT_scaled_size, so the blocks of one wavefront may differ in n: comp[c] says which, and where block jj of
// component c of an MCU goes -- (jj / bw, jj % bw) of the MCU's bh x bw blocks in a plane of `pitch` samples a row.
__global__ void __launch_bounds__(64) jd_idct_kernel(const JpegDesc* __restrict__ descs) {
    __shared__ int blk[8][JD_BLK];
    const JpegDesc& d = descs[blockIdx.y];                              // in place: comp[c] and plane[c] are read at a lane's own c
    const int t = threadIdx.x, b = t >> 3, l = t & 7;
    const int id = blockIdx.x * 8 + b;
    if ((int)blockIdx.x * 8 >= d.nblocks) return;
    const bool valid = id < d.nblocks;
    const int j = valid ? id % d.bpm : 0, mcu = valid ? id / d.bpm : 0;
    const int c = jd_comp(d, j);
    const JpegComp g = d.comp[c];
    const int n = g.n;
    if (valid && (n > 1 || l == 0)) {                                   // n == 1: the DC term alone is read
        const uint4 raw = *(const uint4*)(d.coef + (size_t)id * 64 + l * 8);     // 16-byte aligned: blocks are 128 bytes apart
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
        const unsigned short* q = d.quant + c * 64 + l * 8;
        for (int i = 0; i < 4; ++i) {
            blk[b][l * JD_ROW + 2 * i] = (int)(short)(w[i] & 0xFFFFu) * (int)q[2 * i];
            blk[b][l * JD_ROW + 2 * i + 1] = (int)(short)(w[i] >> 16) * (int)q[2 * i + 1];
        }
    }
    __syncthreads();
    if (valid) {
        int* col = &blk[b][l];
        if (n == 8) idct8(col, JD_ROW, true);
        else if (n == 4) { if (l != 4) idct4(col, JD_ROW, true); }
        else if (n == 2) { if (l == 0 || (l & 1)) idct2(col, JD_ROW, true); }
    }
    __syncthreads();
    if (valid && l < n) {
        int* row = &blk[b][l * JD_ROW];
        if (n == 8) idct8(row, 1, false);
        else if (n == 4) idct4(row, 1, false);
        else if (n == 2) idct2(row, 1, false);
        else row[0] = idct1(row[0]);
        const int jj = c == 0 ? j : 0;                                  // the block's index within its component
        const int mx = mcu % d.mcux, my = mcu / d.mcux;
        // pitch and both offsets are multiples of n, the planes 256-byte aligned: the word below is aligned
        uint8_t* o = d.plane[c] + (size_t)((my * g.bh + jj / g.bw) * n + l) * g.pitch + (mx * g.bw + jj % g.bw) * n;
        if (n == 8) {
            uint2 v;
            v.x = (unsigned)row[0] | ((unsigned)row[1] << 8) | ((unsigned)row[2] << 16) | ((unsigned)row[3] << 24);
            v.y = (unsigned)row[4] | ((unsigned)row[5] << 8) | ((unsigned)row[6] << 16) | ((unsigned)row[7] << 24);
            *(uint2*)o = v;
        } else if (n == 4) {
            *(unsigned*)o = (unsigned)row[0] | ((unsigned)row[1] << 8) | ((unsigned)row[2] << 16) | ((unsigned)row[3] << 24);
        } else if (n == 2) {
            *(unsigned short*)o = (unsigned short)(row[0] | (row[1] << 8));
        } else {
            o[0] = (uint8_t)row[0];
        }
    }
}

// The planes -> YCbCr triples (3 or 4 bytes per pixel) or the grey plane, OW x OH pixels into the caller's tensor: one pixel per lane.
// comp[c].up says how a chroma sample is found (jdsample.c); every chroma read stays inside the valid extent, not the padded plane.
__global__ void __launch_bounds__(256) jd_output_kernel(const JpegDesc* __restrict__ descs) {
    const JpegDesc d = descs[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= d.OW || y >= d.OH) return;
    unsigned v[3] = {d.plane[0][(size_t)y * d.comp[0].pitch + x], 0, 0};
    if (d.ncomp == 1) {
        d.out[(size_t)y * d.pitch + x] = (uint8_t)v[0];
        return;
    }
    for (int c = 1; c < 3; ++c) {
        const uint8_t* __restrict__ pl = d.plane[c];
        const JpegComp& g = d.comp[c];
        switch (g.up) {
        case JD_UP_H2V2_FANCY: v[c] = (unsigned)th_fancy(pl, g.pitch, g.valid_rows, g.valid_cols, y, x); break;
        case JD_UP_H2V1_FANCY: v[c] = (unsigned)th_fancy_h2v1(pl, g.pitch, g.valid_cols, y, x); break;
        case JD_UP_H1V2_FANCY: v[c] = (unsigned)th_fancy_h1v2(pl, g.pitch, g.valid_rows, y, x); break;
        case JD_UP_REPLICATE: v[c] = pl[(size_t)(y / d.comp[0].bh) * g.pitch + x / d.comp[0].bw]; break;   // one sample per luma MCU cell
        default: v[c] = pl[(size_t)y * g.pitch + x];                    // the plane has the output's sampling
        }
    }
    uint8_t* o = d.out + (size_t)y * d.pitch + (size_t)x * d.px;
    if (d.px == 4 && ((d.pitch | (long long)(size_t)d.out) & 3) == 0) {
        *(unsigned*)o = v[0] | (v[1] << 8) | (v[2] << 16) | (255u << 24);
    } else {
        o[0] = (uint8_t)v[0];
        o[1] = (uint8_t)v[1];
        o[2] = (uint8_t)v[2];
        if (d.px == 4) o[3] = 255;
    }
}

}  // namespace

hipError_t launch_jd_sync(const JpegDesc* descs, int n, int max_groups, int pass, hipStream_t s) {
    hipLaunchKernelGGL(jd_sync_kernel, dim3((unsigned)max_groups, (unsigned)n), dim3(JD_LANES), 0, s, descs, pass);
    return hipGetLastError();
}
hipError_t launch_jd_scan(const JpegDesc* descs, int n, hipStream_t s) {
    hipLaunchKernelGGL(jd_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, descs);
    return hipGetLastError();
}
hipError_t launch_jd_write(const JpegDesc* descs, int n, int max_groups, hipStream_t s) {
    hipLaunchKernelGGL(jd_write_kernel, dim3((unsigned)max_groups, (unsigned)n), dim3(JD_LANES), 0, s, descs);
    return hipGetLastError();
}
hipError_t launch_jd_dc(const JpegDesc* descs, int n, int max_seg, hipStream_t s) {
    hipLaunchKernelGGL(jd_dc_kernel, dim3((unsigned)max_seg, 3u, (unsigned)n), dim3(256), 0, s, descs);
    return hipGetLastError();
}
hipError_t launch_jd_idct(const JpegDesc* descs, int n, int max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)((max_blocks + 7) / 8), (unsigned)n), dim3(64), 0, s, descs);
    return hipGetLastError();
}
hipError_t launch_jd_output(const JpegDesc* descs, int n, int max_h, int max_w, hipStream_t s) {
    hipLaunchKernelGGL(jd_output_kernel, dim3((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)n), dim3(256), 0, s, descs);
    return hipGetLastError();
}
