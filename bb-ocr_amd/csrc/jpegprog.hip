// Progressive JPEG decoding on the device: the entropy stages of the scans of one dependency level over a batch (jpegdec.cpp).
//   first scans (DC first, AC first)   jpegdec.hip's speculative scheme -- jpeg_spec.h's passes, here over jpegprog.h's jp_run_first
//               (JpCodec) --: jp_sync (one lane per S-bit
//               subsequence decodes from the assumed state, then from its left neighbour's exit state until no state changes), jp_prefix
//               (first block of every subsequence), jp_write (decode from the exact states into the coefficient buffer), jp_dc (a DC
//               scan's running sums per component and restart segment, shifted by Al).  A DC block ends after its symbol; the blocks of
//               an end-of-band run take no bits and are counted at its symbol, so the state is (bit, block in the unit, place in the band)
//   DC refinement   a parallel pass, one lane per unit: raw bits at known places
//   AC refinement   serial per restart segment, one lane per (scan, segment): the correction bits a block takes depend on its history,
//               so the stream cannot be entered in the middle
// The IDCT and the output stage that follow are jpegdec.hip's.
#include "common.h"
#include "jpegprog.h"

namespace {

__device__ __forceinline__ bool jp_first(const JpScan& sc) { return sc.nseg > 0 && sc.Ah == 0; }

// A first scan as jpeg_spec.h's passes see it: units are MCUs or the component's blocks, a segment starts at the band's first
// coefficient of block 0 and must end there with less than a byte left; an end-of-band run may leave the segment (`over`).
struct JpCodec {
    using Desc = JpScan;
    struct Lds { JpegHuff* T; unsigned char* ZZ; };            // T[3], ZZ[64] of the kernel's LDS
    static __device__ __forceinline__ bool cut(const JpScan& sc) { return jp_first(sc); }
    static __device__ __forceinline__ void load(const JpScan& sc, const Lds& lds, int t, int nt) {
        const int ncs = min(max(sc.ncs, 0), 3);
        const int* src = (const int*)sc.huff;
        int* dst = (int*)lds.T;
        for (int i = t; i < ncs * (int)(sizeof(JpegHuff) / 4); i += nt) dst[i] = src[i];
        if (t < 64) lds.ZZ[t] = JPEG_ZZ[t];
        __syncthreads();
    }
    static __device__ __forceinline__ int unit_blocks(const JpScan& sc) { return jp_unit_total(sc); }
    static __device__ __forceinline__ int units(const JpScan& sc) { return sc.nunits; }
    static __device__ __forceinline__ JpegState start(const JpScan& sc, unsigned p) { return jp_start(sc, p); }
    static __device__ __forceinline__ int run(const JpScan& sc, const Lds& lds, int bpu, const JpegSub& s, JpegState& st, int max_blocks, bool store,
                                              long long first, bool* invalid, bool* over) {
        return jp_run_first(sc, lds.T, lds.ZZ, bpu, s.b0, s.b1, st, s.end, max_blocks, store, first, invalid, over);
    }
    static __device__ __forceinline__ bool at_end(const JpScan& sc, const JpegState& st, const JpegSub& s) { return jp_at_end(sc, st, s.b1); }
    static __device__ __forceinline__ void note_first(const JpScan&, int, long long) {}
};

// the descriptor in place: a copy would live in scratch
__global__ void __launch_bounds__(JD_LANES) jp_sync_kernel(const JpScan* __restrict__ scans, int pass) {
    __shared__ JpegHuff T[3];
    __shared__ unsigned char ZZ[64];
    __shared__ unsigned long long ex[JD_LANES];
    jpeg_sync_pass<JpCodec>(scans[blockIdx.y], {T, ZZ}, ex, pass);
}

// one workgroup per scan
__global__ void __launch_bounds__(256) jp_prefix_kernel(const JpScan* __restrict__ scans) {
    __shared__ long long sh[256];
    jpeg_prefix_pass<JpCodec>(scans[blockIdx.x], sh);
}

__global__ void __launch_bounds__(JD_LANES) jp_write_kernel(const JpScan* __restrict__ scans) {
    __shared__ JpegHuff T[3];
    __shared__ unsigned char ZZ[64];
    jpeg_write_pass<JpCodec>(scans[blockIdx.y], {T, ZZ});
}

// one wavefront per (segment, scan component, scan) of a DC first scan: inclusive sum of the differences in scan order, 64 at a time
__global__ void __launch_bounds__(64) jp_dc_kernel(const JpScan* __restrict__ scans) {
    const JpScan& sc = scans[blockIdx.z];
    const int seg = blockIdx.x, ci = blockIdx.y, t = threadIdx.x;
    if (!jp_first(sc) || sc.Ss != 0 || seg >= sc.nseg || ci >= sc.ncs) return;
    JP_GLOBAL short* coef = (JP_GLOBAL short*)sc.coef;
    const int items = min(sc.ri, sc.nunits - seg * sc.ri) * jp_unit_blocks(sc, ci), Al = sc.Al;
    unsigned carry = 0;
    for (int base = 0; base < items; base += 64) {
        const int i = base + t;
        const long long blk = i < items ? jp_dc_item_block(sc, seg, ci, i) : -1;
        const bool in = blk >= 0 && blk < sc.nblocks;
        unsigned v = in ? (unsigned)(int)coef[blk * 64] : 0u;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned a = __shfl_up(v, o, 64);
            if (t >= o) v += a;
        }
        v += carry;
        if (in) coef[blk * 64] = (short)(v << Al);
        carry = __shfl(v, 63, 64);
    }
}

// The correction bits of the coefficients in `passed`, read side by side: the i-th of them (in zig-zag order) takes bit i behind the
// reader's position, which lies in the 96 bits the reader holds -- at most 63 of them behind an offset below 32.
__device__ __forceinline__ void jp_correct_wave(JpBits& s, unsigned long long passed, int lane, int p1, int& v, bool& changed) {
    const int n = __builtin_popcountll(passed);
    if (!n) return;
    jp_peek(s, 1);                                              // brings the window to the position
    if ((passed >> lane) & 1) {
        const unsigned q = ((s.p - s.wb * 8u) & 31u) + (unsigned)__builtin_popcountll(passed & ((1ull << lane) - 1));
        const unsigned bit = q < 64 ? (unsigned)(s.win >> (63 - q)) & 1u : (s.ahead >> (95 - q)) & 1u;
        if (bit && !(v & p1)) {
            v += v < 0 ? -p1 : p1;
            changed = true;
        }
    }
    s.p += (unsigned)n;
}

// One restart segment of an AC refinement (decode_mcu_AC_refine) by one wavefront: lane l holds the block's coefficient at zig-zag
// position l, so the block's history is one ballot.  Every lane follows the stream -- the symbols are serial -- and resolves a symbol with
// jp_refine_walk's mask arithmetic; the corrections of the coefficients a symbol passes, and those of a block inside an end-of-band run,
// are applied by their lanes at once.  The next block is fetched while this one is decoded; a lane stores its coefficient when it changed.
__device__ int jp_ac_refine_wave(const JpScan& sc, const JpegHuff& H, const unsigned char* ZZ, int seg, int lane) {
    if (sc.ri < 1 || sc.bw < 1 || sc.ch < 1 || sc.cv < 1 || sc.Ss < 1 || sc.Se > 63) return JD_ERR_COUNT;
    const JP_GLOBAL int* seg_byte = (const JP_GLOBAL int*)sc.seg_byte;
    JP_GLOBAL short* coef = (JP_GLOBAL short*)sc.coef;
    JpBits s = jp_open(sc.data, (unsigned)seg_byte[seg], (unsigned)seg_byte[seg + 1]);
    const long long u0 = (long long)seg * sc.ri;
    const int nu = (int)(sc.nunits - u0 < sc.ri ? sc.nunits - u0 : sc.ri);
    const int Ss = sc.Ss, Se = sc.Se, p1 = 1 << sc.Al, zz = ZZ[lane];
    int eobrun = 0, err = 0;
    long long blk = nu > 0 ? jp_block(sc, (int)u0, 0, 0) : -1;
    int ahead = blk >= 0 && blk < sc.nblocks ? (int)coef[blk * 64 + zz] : 0;
    for (int i = 0; i < nu && !err; ++i) {
        const long long cur = blk;
        int v = ahead;
        if (i + 1 < nu) {
            blk = jp_block(sc, (int)u0 + i + 1, 0, 0);
            ahead = blk >= 0 && blk < sc.nblocks ? (int)coef[blk * 64 + zz] : 0;
        }
        if (!(cur >= 0 && cur < sc.nblocks)) { err = JD_ERR_COUNT; break; }                   // never, for a plan of jpeg_parse.h
        const unsigned long long nz = __ballot(v != 0);
        bool changed = false;
        int k = Ss;
        if (eobrun == 0) {
            for (; k <= Se; ++k) {
                const int sym = jp_symbol(H, s);
                if (sym < 0) { err = JD_ERR_CODE; break; }
                const int r = sym >> 4, sz = sym & 15;
                bool place = false, negative = false;
                if (sz) {
                    if (sz != 1) { err = JD_ERR_CODE; break; }
                    place = true;
                    negative = !jp_get(s, 1);
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += (int)jp_get(s, r);
                    break;
                }
                const JpWalk w = jp_refine_walk(nz, k, Se, r);
                jp_correct_wave(s, w.passed, lane, p1, v, changed);
                k = w.target;
                if (place) {
                    if (k > Se) { err = JD_ERR_CODE; break; }
                    if (lane == k) {
                        v = negative ? -p1 : p1;
                        changed = true;
                    }
                }
            }
        }
        if (err) break;
        if (eobrun > 0) {
            if (k <= Se) jp_correct_wave(s, jp_refine_walk(nz, k, Se, 64).passed, lane, p1, v, changed);
            --eobrun;
        }
        if (changed) coef[cur * 64 + zz] = (short)v;
    }
    if (!err && (eobrun != 0 || s.p > s.b1 * 8u || s.b1 * 8u - s.p >= 8u)) err = JD_ERR_COUNT;
    return err;
}

// the refinements of a level: a DC refinement one lane per unit, an AC refinement one wavefront per restart segment
__global__ void __launch_bounds__(64) jp_scan_kernel(const JpScan* __restrict__ scans) {
    __shared__ JpegHuff T[1];
    __shared__ unsigned char ZZ[64];
    const JpScan& sc = scans[blockIdx.y];                       // in place: a copy of the descriptor would live in scratch
    const int t = threadIdx.x;
    if (sc.Ah == 0 || sc.nseg < 1) return;                      // a first scan: the kernels above
    if (sc.Ss == 0) {                                           // raw bits at known places
        const int u = blockIdx.x * 64 + t;
        if (u < sc.nunits) {
            const int err = jp_dc_refine_unit(sc, u);
            if (err) atomicOr(sc.status, err);
        }
        return;
    }
    const int seg = blockIdx.x;
    if (seg >= sc.nseg) return;
    const int* src = (const int*)sc.huff;
    int* dst = (int*)T;
    for (int i = t; i < (int)(sizeof(JpegHuff) / 4); i += 64) dst[i] = src[i];
    ZZ[t] = JPEG_ZZ[t];
    __syncthreads();
    const int err = jp_ac_refine_wave(sc, T[0], ZZ, seg, t);
    if (err && t == 0) atomicOr(sc.status, err);
}

}  // namespace

hipError_t launch_jp_scan(const JpScan* scans, int n, int max_groups, hipStream_t s) {
    hipLaunchKernelGGL(jp_scan_kernel, dim3((unsigned)max_groups, (unsigned)n), dim3(64), 0, s, scans);
    return hipGetLastError();
}
hipError_t launch_jp_first(const JpScan* scans, int n, int max_groups, int passes, int max_seg, hipStream_t s) {
    for (int pass = 0; pass < passes; ++pass) hipLaunchKernelGGL(jp_sync_kernel, dim3((unsigned)max_groups, (unsigned)n), dim3(64), 0, s, scans, pass);
    hipLaunchKernelGGL(jp_prefix_kernel, dim3((unsigned)n), dim3(256), 0, s, scans);
    hipLaunchKernelGGL(jp_write_kernel, dim3((unsigned)max_groups, (unsigned)n), dim3(64), 0, s, scans);
    hipLaunchKernelGGL(jp_dc_kernel, dim3((unsigned)max_seg, 3u, (unsigned)n), dim3(64), 0, s, scans);
    return hipGetLastError();
}
