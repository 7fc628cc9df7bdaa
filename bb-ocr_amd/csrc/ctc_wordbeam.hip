// decoder='wordbeamsearch' on the device, for contexts of at most 128 classes: ctc_wordbeam.cpp's definition (the host search there is what
// these kernels are held to, text for text) between the CTC row kernel and the read-back of the text, with no host wait in between.
//
//   word_segments_kernel   one wave per SEQUENCE: the rows' arg-max (ctc_rows_kernel's idx) -> the sequence's word groups, the maximal runs of
//                          rows whose arg-max is not the space.  A ballot per 64 rows marks the rows of a group; a group ENDS at position t
//                          (exclusive) where the bit below t is set and t's own is not -- the bit below lane 0 is the carry out of the chunk
//                          before, and positions run to T itself, so a group that reaches row 63, 64 or the last row ends like any other.
//                          The lane at a group's end knows its start: one past the highest clear bit below it, or the start carried into
//                          the chunk.  Two walks: the first counts the sequence's groups, one atomic add reserves their places in the
//                          global segment table (places of one sequence are contiguous and in order; the order of the sequences' blocks
//                          in the table is the order of arrival, which nothing depends on), the second writes {first row, T}.
//   ctc_wordbeam_kernel    one wave per SEGMENT, taken by a grid-stride loop over the device's segment count: ctc_beam_steps.h's loop (the
//                          one ctc_beam_kernel runs) over the segment's rows, whose last step ranks min(BBOCR_WORD_CANDIDATES, #entries)
//                          positions of its entry table.  In rank order the wave forms the collapsed text of entry (b, k) -- lab(b) plus
//                          the extension symbol -- in an LDS line, hashes it and probes the dictionary (word_dict.h's lookup, the symbols
//                          compared wave-wide); the first hit ends the loop wave-uniformly, no hit falls back to rank 0.  The word goes to
//                          the segment's own rows of the row-indexed text buffer, its length to the segment table.
//   word_join_kernel       one wave per sequence: its words, one space class between them, into the sequence's rows of a SECOND buffer (a
//                          segment's rows overlap the output's), and the length.
//   row_argmax_kernel      the arg-max of probability rows, for callers that hold no idx (bbocr_op_ctc_wordbeam)
//   dict_lookup_kernel     one wave per query string: the table's lookup alone (bbocr_op_dict_lookup)
//
// As in ctc_beam.hip every loop has a trip count fixed by T, W, C, tstride, the candidate count, the segment capacity or the recorded probe
// bound, every LDS and global index is bounded by a launch argument, and a segment or table the host would have refused touches nothing but
// its length.
#include "bbocr.h"
#include "common.h"
#include "kernels.h"
#include "ctc_beam_steps.h"
#include "word_dict.h"

#include <algorithm>

namespace {

struct WdWave {          // word_dict.h's policy for one wave: lanes compare 64 symbols at a time, everyone gets the same answer
    template <class A, class B> __device__ static bool equal(const A* a, const B* b, int n) {
        bool mism = false;
        for (int i = threadIdx.x & 63; i < n; i += 64) mism = mism || (int)a[i] != (int)b[i];
        return !__any(mism);
    }
};

constexpr int kWordGridMax = 8192;             // workgroups of ctc_wordbeam_kernel at most: the loop strides over the rest

__host__ __device__ inline int word_nsel(int W) { return W > BBOCR_WORD_CANDIDATES ? W : BBOCR_WORD_CANDIDATES; }
__host__ __device__ inline size_t word_lds_words(int W, int C, int tstride) {
    return beam_dev::beam_lds_words(W, word_nsel(W), C, tstride) + (size_t)(tstride / 4);       // + the collapsed text's line
}

// one 64-row chunk of a sequence's arg-max row: m marks the rows of a group, ends the positions (t0 + lane <= T) where a group ends
__device__ inline void segment_chunk(const int* __restrict__ ip, int T, int t0, int space, unsigned long long carry, unsigned long long& m,
                                     unsigned long long& ends) {
    const int t = t0 + (int)threadIdx.x;
    const bool in = t < T && ip[t] != space;
    m = __ballot(in);
    ends = ((m << 1) | carry) & ~m & __ballot(t <= T);
}

}   // namespace

__global__ void __launch_bounds__(256) row_argmax_kernel(const float* __restrict__ probs, size_t rows, int C, int cs, int* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const size_t row = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= rows) return;
    const float* p = probs + row * cs;
    float bp = lane < C ? p[lane] : -INFINITY;
    int bi = lane;
    if (lane + 64 < C && p[lane + 64] > bp) { bp = p[lane + 64]; bi = lane + 64; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float op = __shfl_xor(bp, o);
        const int oi = __shfl_xor(bi, o);
        if (op > bp || (op == bp && oi < bi)) { bp = op; bi = oi; }
    }
    if (lane == 0) idx[row] = bi < C ? bi : 0;
}

__global__ void __launch_bounds__(64) word_segments_kernel(const int* __restrict__ idx, size_t rows, const int2* __restrict__ seqs, int nseq, int space,
                                                           int2* __restrict__ segs, int seg_cap, int2* __restrict__ seq_seg, int* __restrict__ counter) {
    const int seq = blockIdx.x;
    const int lane = threadIdx.x;
    if (seq >= nseq) return;
    const int2 sd = seqs[seq];
    const int T = sd.y;
    if (sd.x < 0 || T < 0 || (size_t)sd.x + (size_t)T > rows) {          // a table the host would have refused: no segment
        if (lane == 0) seq_seg[seq] = make_int2(0, 0);
        return;
    }
    const int* ip = idx + (size_t)sd.x;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    int count = 0;
    unsigned long long carry = 0ULL, m, ends;
    for (int t0 = 0; t0 <= T; t0 += 64) {
        segment_chunk(ip, T, t0, space, carry, m, ends);
        count += __popcll(ends);
        carry = m >> 63;
    }
    int base = 0;
    if (lane == 0 && count > 0) base = atomicAdd(counter, count);
    base = __shfl(base, 0);
    if (base < 0 || base > seg_cap) base = seg_cap;
    if (lane == 0) seq_seg[seq] = make_int2(base, min(count, seg_cap - base));
    int nend = 0, open_start = 0;
    carry = 0ULL;
    for (int t0 = 0; t0 <= T; t0 += 64) {
        segment_chunk(ip, T, t0, space, carry, m, ends);
        if ((ends >> lane) & 1ULL) {
            const unsigned long long z = ~m & lt;                           // rows below this lane that belong to no group
            const int start = z ? t0 + 64 - __clzll((long long)z) : (carry ? open_start : t0);
            const int k = base + nend + __popcll(ends & lt);
            if (k < seg_cap) segs[k] = make_int2(sd.x + start, t0 + lane - start);
        }
        nend += __popcll(ends);
        if (m >> 63) {
            const unsigned long long z = ~m;
            open_start = z ? t0 + 64 - __clzll((long long)z) : (carry ? open_start : t0);
        }
        carry = m >> 63;
    }
}

__global__ void __launch_bounds__(64) ctc_wordbeam_kernel(const float* __restrict__ probs, size_t rows, int C, int cs, const int2* __restrict__ segs,
                                                          const int* __restrict__ counter, int seg_cap, int W, int tstride, float thr,
                                                          const WdSlot* __restrict__ slots, unsigned int nslots, int probe,
                                                          const unsigned char* __restrict__ pool, unsigned int pool_n, int* __restrict__ out_text,
                                                          int* __restrict__ seg_len) {
    extern __shared__ unsigned int lds[];
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const int nsel = word_nsel(W);
    BEAM_LDS_VIEWS(lds, W, nsel, C, tstride);
    unsigned char* line = (unsigned char*)(labs + (size_t)2 * W * tw);          // tstride bytes: the collapsed text of one candidate
    const int nseg = min(max(*counter, 0), seg_cap);
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int2 sg = segs[s];
        const int T = sg.y;
        if (sg.x < 0 || T < 1 || T > tstride || (size_t)sg.x + (size_t)T > rows) {       // a segment the host rule cannot make: nothing but the length
            if (lane == 0) seg_len[s] = 0;
            continue;
        }
        int cur, nb, stride, nfinal;
        beam_search_steps<true>(lds, probs + (size_t)sg.x * cs, T, C, cs, W, nsel, tstride, thr, BBOCR_WORD_CANDIDATES, cur, nb, stride, nfinal);
        const int* len = B_LEN(cur);
        // the collapsed text of ranked candidate r -> line, its length: the labelling is lab(b) (+ the extension class), class 0 and symbols
        // equal to their predecessor in the labelling dropped
        auto form = [&](int r) {
            const int pos = sel[r];
            const int b = min(max(pos / stride, 0), W - 1), k = pos - (pos / stride) * stride;
            const int L = min(max(len[b], 0), tstride - (k > 0 ? 1 : 0));
            const int c = k > 0 ? cand_cls[k - 1] : 0;
            const int Lx = L + (k > 0 ? 1 : 0);                                  // <= T <= tstride
            const unsigned char* lab = (const unsigned char*)B_LAB(cur, b);
            int outn = 0;
            for (int i0 = 0; i0 < Lx; i0 += 64) {
                const int i = i0 + lane;
                const int sy = i < L ? (int)lab[i] : c;
                const int pv = i > 0 && i < Lx ? (i - 1 < L ? (int)lab[i - 1] : c) : -1;
                const bool keep = i < Lx && sy != 0 && sy != pv;
                const unsigned long long km = __ballot(keep);
                if (keep) line[outn + __popcll(km & lt)] = (unsigned char)sy;    // < Lx <= tstride
                outn += __popcll(km);
            }
            __syncthreads();
            return outn;
        };
        int hit = -1, n = 0, formed = -1;
        for (int r = 0; r < nfinal; ++r) {
            n = form(r);
            formed = r;
            const bool member = wd_lookup<WdWave>(slots, nslots, probe, pool, pool_n, line, n, wd_hash(line, n));
            __syncthreads();
            if (member) { hit = r; break; }                                       // wave-uniform: every lane computed the same answer
        }
        if (nfinal > 0) {
            if (hit < 0) hit = 0;
            if (formed != hit) n = form(hit);
            for (int i = lane; i < n && i < T; i += 64) out_text[(size_t)sg.x + i] = (int)line[i];
        } else {
            n = 0;
        }
        if (lane == 0) seg_len[s] = min(n, T);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) word_join_kernel(const int2* __restrict__ seqs, int nseq, size_t rows, const int2* __restrict__ segs,
                                                       const int* __restrict__ seg_len, const int2* __restrict__ seq_seg, int seg_cap, int space,
                                                       const int* __restrict__ text_in, int* __restrict__ out_text, int* __restrict__ out_len) {
    const int seq = blockIdx.x;
    const int lane = threadIdx.x;
    if (seq >= nseq) return;
    const int2 sd = seqs[seq];
    const int T = sd.y;
    if (sd.x < 0 || T < 0 || (size_t)sd.x + (size_t)T > rows) {
        if (lane == 0) out_len[seq] = 0;
        return;
    }
    const int2 ss = seq_seg[seq];
    const int cnt = min(max(ss.y, 0), (T + 1) / 2);
    int* op = out_text + (size_t)sd.x;
    int pos = 0;
    for (int k = 0; k < cnt; ++k) {
        const int g = ss.x + k;
        if (g < 0 || g >= seg_cap) break;
        const int2 sg = segs[g];
        if (k > 0) {                                                              // a word that collapsed to nothing still brings its separator
            if (lane == 0 && pos < T) op[pos] = space;
            ++pos;
        }
        const bool inside = sg.x >= 0 && sg.y >= 0 && (size_t)sg.x + (size_t)sg.y <= rows;
        const int n = inside ? min(max(seg_len[g], 0), sg.y) : 0;
        for (int i = lane; i < n; i += 64)
            if (pos + i < T) op[pos + i] = text_in[(size_t)sg.x + i];
        pos += n;
    }
    if (lane == 0) out_len[seq] = min(pos, T);
}

__global__ void __launch_bounds__(64) dict_lookup_kernel(const WdSlot* __restrict__ slots, unsigned int nslots, int probe,
                                                         const unsigned char* __restrict__ pool, unsigned int pool_n, const unsigned char* __restrict__ qsym,
                                                         const int* __restrict__ qoff, int nq, int qtotal, int* __restrict__ found) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int a = qoff[q], b = qoff[q + 1];
    bool member = false;
    if (a >= 0 && b >= a && b <= qtotal && b - a <= WD_WORD_MAX)
        member = wd_lookup<WdWave>(slots, nslots, probe, pool, pool_n, qsym + a, b - a, wd_hash(qsym + a, b - a));
    if (threadIdx.x == 0) found[q] = member ? 1 : 0;
}

size_t ctc_wordbeam_lds_bytes(int beam_width, int C, int max_T) {
    const int tstride = (std::max(max_T, 1) + 3) & ~3;
    return word_lds_words(beam_width, C, tstride) * 4;
}

bool ctc_wordbeam_on_device(int beam_width, int C, int max_T) {
    return beam_width >= 1 && beam_width <= BBOCR_BEAM_DEVICE_MAX && C >= 1 && C <= 128 && max_T >= 0 && max_T <= (1 << 20) &&
           ctc_wordbeam_lds_bytes(beam_width, C, max_T) <= kCtcBeamLdsLimit;
}

hipError_t launch_row_argmax(const float* probs, size_t rows, int C, int cs, int* idx, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (!probs || !idx || C < 1 || C > 128 || cs < C || rows > (size_t)INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row_argmax_kernel, dim3((unsigned int)((rows + 3) / 4)), dim3(256), 0, s, probs, rows, C, cs, idx);
    return hipGetLastError();
}

hipError_t launch_word_segments(const int* idx, size_t rows, const int* seqs_dev, int nseq, int space, int* segs, int seg_cap, int* seq_seg, int* counter,
                                hipStream_t s) {
    if (nseq <= 0) return hipSuccess;
    if (!idx || !seqs_dev || !segs || !seq_seg || !counter || seg_cap < 0 || rows > (size_t)INT32_MAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(word_segments_kernel, dim3(nseq), dim3(64), 0, s, idx, rows, (const int2*)seqs_dev, nseq, space, (int2*)segs, seg_cap, (int2*)seq_seg,
                       counter);
    return hipGetLastError();
}

hipError_t launch_ctc_wordbeam(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int space,
                               const WordDictDev& d, const int* segs, int seg_cap, const int* seq_seg, const int* counter, int* seg_len, int* seg_text,
                               int* out_text, int* out_len, hipStream_t s) {
    if (nseq <= 0) return hipSuccess;
    if (!probs || !seqs_dev || !segs || !seq_seg || !counter || !seg_len || !seg_text || !out_text || !out_len || seg_cap < 0 || cs < C ||
        rows > (size_t)INT32_MAX || !d.slots || !d.pool || d.nslots == 0 || (d.nslots & (d.nslots - 1)) != 0 || d.probe < 0 ||
        !ctc_wordbeam_on_device(beam_width, C, max_T))
        return hipErrorInvalidValue;
    const int tstride = (std::max(max_T, 1) + 3) & ~3;
    const float thr = (float)(0.5 / (double)C);
    if (seg_cap > 0)
        hipLaunchKernelGGL(ctc_wordbeam_kernel, dim3(std::min(seg_cap, kWordGridMax)), dim3(64), ctc_wordbeam_lds_bytes(beam_width, C, max_T), s, probs, rows,
                           C, cs, (const int2*)segs, counter, seg_cap, beam_width, tstride, thr, (const WdSlot*)d.slots, d.nslots, d.probe, d.pool, d.pool_n,
                           seg_text, seg_len);
    hipLaunchKernelGGL(word_join_kernel, dim3(nseq), dim3(64), 0, s, (const int2*)seqs_dev, nseq, rows, (const int2*)segs, (const int*)seg_len,
                       (const int2*)seq_seg, seg_cap, space, (const int*)seg_text, out_text, out_len);
    return hipGetLastError();
}

hipError_t launch_dict_lookup(const WordDictDev& d, const unsigned char* qsym, const int* qoff, int nq, int qtotal, int* found, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (!d.slots || !d.pool || d.nslots == 0 || (d.nslots & (d.nslots - 1)) != 0 || d.probe < 0 || !qsym || !qoff || !found || qtotal < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dict_lookup_kernel, dim3(nq), dim3(64), 0, s, (const WdSlot*)d.slots, d.nslots, d.probe, d.pool, d.pool_n, qsym, qoff, nq, qtotal,
                       found);
    return hipGetLastError();
}

#undef BEAM_LDS_VIEWS
#undef B_TOTAL
#undef B_NONBLANK
#undef B_BLANK
#undef B_LEN
#undef B_LAST
#undef B_HASH
#undef B_PHASH
#undef B_LAB
