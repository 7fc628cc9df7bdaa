// CTC beam-search decode on the device for recognisers of MORE than 128 classes (bbocr_config_v2::beam_wide): 128 < C <= BBOCR_REC_CLASSES_MAX,
// beamWidth <= BBOCR_BEAM_DEVICE_MAX.  The text is ctc_beam.cpp::ctc_beam_search_host's for every input, as ctc_beam.hip's is for C <= 128.
//
// What the search reads of a row: its candidate classes (p[c] >= 0.5/C, the blank included) -- few on a trained model -- and two more values
// whether or not they are candidates: p[0] (pr_b) and p[last symbol] of each live beam (pr_nb).  So the work is split in two:
//
//   ctc_beam_cand_kernel   one wave per ROW, all rows in parallel: the row's candidate count n_t and its first min(n_t, kBeamWideCand)
//                          candidates in ascending class order as {class, p} pairs (1 KB per row, against 4 * cs bytes of probabilities).
//   ctc_beam_wide_kernel   one wave per SEQUENCE: ctc_beam_kernel restated statement by statement, with
//                            * candidate RANK in the place of the class index: entry position b * (1 + n) + k is beam b's copy (k = 0) or its
//                              extension by the k-th candidate in ascending class order -- the host's insertion order;
//                            * labellings as 16-bit symbols, two per LDS word;
//                            * class -> rank by comparing the <= 128 candidate classes across the wave (there is no cand_rank[C] table);
//                            * p[0] and every live beam's p[last] gathered from the full row in device memory, once per step.
//                          The float32 association, the stable "lower position wins" ranking, the identity of labellings symbol by symbol (no
//                          parent pointers) and the merge of a copy with an extension are ctc_beam_kernel's.
//
// A sequence with a row of more than kBeamWideCand candidates is NOT searched: its length is written as -1 and the caller searches it on the
// host from the probabilities, which are still resident (recognizer.cpp::ctc_beam_wide_fallback).
//
// Every loop has a trip count fixed by T, W, kBeamWideCand, C or tstride; every LDS index is bounded by those (the launch sizes the LDS block
// from them).
#include "bbocr.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace {

constexpr int K = kBeamWideCand;
static_assert(K == 128, "two candidates per lane: ctc_beam_wide_kernel loads cand[lane] and cand[lane + 64]");
constexpr int kFixedWords = 2 * K + 4;                            // cand_cls[K] | cand_p[K] | p[0] (+ 3 words of padding)
constexpr int kStateFields = 7;                                   // total, nonblank, blank, len, last, hash, phash (x 2 buffers)
constexpr int kStepFields = 4;                                    // mpar[W], mrank[W], sel[W], plast[W]
constexpr unsigned int kHash0 = 2166136261u;
constexpr int kCandWaves = 4;                                     // rows per workgroup of ctc_beam_cand_kernel

__host__ __device__ inline size_t beam_wide_lds_words(int W, int tstride) {
    return (size_t)kFixedWords + (size_t)(2 * kStateFields + kStepFields) * W + (size_t)W * (1 + K) + (size_t)2 * W * (tstride / 2);
}

__device__ inline unsigned int hash_push(unsigned int h, int c) { return (h ^ (unsigned int)(c + 1)) * 16777619u; }

}   // namespace

__global__ void __launch_bounds__(64 * kCandWaves) ctc_beam_cand_kernel(const float* __restrict__ probs, size_t rows, int C, int cs, float thr,
                                                                        int* __restrict__ cand_n, int2* __restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * kCandWaves + (threadIdx.x >> 6);
    if (row >= rows) return;                                      // wave-uniform
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const float* p = probs + row * (size_t)cs;
    int2* out = cand + row * (size_t)K;
    int n = 0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const float v = c < C ? p[c] : 0.f;
        const bool is = c < C && v >= thr;
        const unsigned long long m = __ballot(is);
        const int r = n + __popcll(m & lt);
        if (is && r < K) out[r] = make_int2(c, __float_as_int(v));
        n += __popcll(m);
    }
    if (lane == 0) cand_n[row] = n;
}

__global__ void __launch_bounds__(64) ctc_beam_wide_kernel(const float* __restrict__ probs, size_t rows, int C, int cs,
                                                           const int* __restrict__ cand_n, const int2* __restrict__ cand,
                                                           const int2* __restrict__ seqs, int nseq, int W, int tstride,
                                                           int* __restrict__ out_text, int* __restrict__ out_len) {
    extern __shared__ unsigned int lds[];
    const int seq = blockIdx.x;
    const int lane = threadIdx.x;
    if (seq >= nseq) return;
    const int2 sd = seqs[seq];
    const int T = sd.y;
    if (sd.x < 0 || T < 0 || T > tstride || (size_t)sd.x + (size_t)T > rows) {     // a table the host would have refused: touch nothing but the length
        if (lane == 0) out_len[seq] = 0;
        return;
    }
    {   // a row with more candidates than the list holds: the host searches this sequence
        bool over = false;
        for (int t = lane; t < T; t += 64) over = over || cand_n[(size_t)sd.x + t] > K;
        if (__any(over)) {
            if (lane == 0) out_len[seq] = -1;
            return;
        }
    }
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const int tw = tstride >> 1;                                  // words per labelling, two symbols each

    int* cand_cls = (int*)lds;                                    // k -> class
    float* cand_p = (float*)(lds + K);                            // k -> p[class]
    float* prow0 = (float*)(lds + 2 * K);                         // p[0]
    unsigned int* st = lds + kFixedWords;
    int* mpar = (int*)(st + 2 * kStateFields * W);                // beam b's copy is the same entry as the extension of beam mpar[b] by last[b] ...
    int* mrank = mpar + W;                                        // ... which is candidate mrank[b] of this step
    int* sel = mrank + W;                                         // ranked entry positions of the step
    float* plast = (float*)(sel + W);                             // p[last[b]] of the full row (0 for the empty labelling)
    float* tot = plast + W;
    unsigned int* labs = (unsigned int*)(tot + (size_t)W * (1 + K));
#define B_TOTAL(q) ((float*)(st + ((q) * kStateFields + 0) * W))
#define B_NONBLANK(q) ((float*)(st + ((q) * kStateFields + 1) * W))
#define B_BLANK(q) ((float*)(st + ((q) * kStateFields + 2) * W))
#define B_LEN(q) ((int*)(st + ((q) * kStateFields + 3) * W))
#define B_LAST(q) ((int*)(st + ((q) * kStateFields + 4) * W))
#define B_HASH(q) (st + ((q) * kStateFields + 5) * W)
#define B_PHASH(q) (st + ((q) * kStateFields + 6) * W)
#define B_LAB(q, b) (labs + ((size_t)(q) * W + (b)) * tw)

    int cur = 0, nb = 1;
    if (lane == 0) {                                              // the empty labelling: prBlank = prTotal = 1
        B_TOTAL(0)[0] = 1.f; B_NONBLANK(0)[0] = 0.f; B_BLANK(0)[0] = 1.f;
        B_LEN(0)[0] = 0; B_LAST(0)[0] = -1; B_HASH(0)[0] = kHash0; B_PHASH(0)[0] = 0u;
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* total = B_TOTAL(cur);
        const float* nonblank = B_NONBLANK(cur);
        const float* blank = B_BLANK(cur);
        const int* len = B_LEN(cur);
        const int* last = B_LAST(cur);
        const unsigned int* hash = B_HASH(cur);
        const unsigned int* phash = B_PHASH(cur);
        const int nxt = cur ^ 1;

        // ---- the row's candidate classes, ascending, and the two values the copies read whether or not they are candidates
        const size_t row = (size_t)sd.x + (size_t)t;
        const float* p = probs + row * (size_t)cs;
        const int n = min(max(cand_n[row], 0), K);
        const int2* cr = cand + row * (size_t)K;
        if (lane < n) { const int2 e = cr[lane]; cand_cls[lane] = e.x; cand_p[lane] = __int_as_float(e.y); }
        if (lane + 64 < n) { const int2 e = cr[lane + 64]; cand_cls[lane + 64] = e.x; cand_p[lane + 64] = __int_as_float(e.y); }
        if (lane < nb) {
            const int c = last[lane];
            plast[lane] = (len[lane] > 0 && c >= 0 && c < C) ? p[c] : 0.f;
        }
        if (lane == 0) prow0[0] = p[0];
        __syncthreads();

        // ---- which copies meet an extension: lab(b) == lab(b') + [last(b)], decided on the symbols
        for (int b = 0; b < nb; ++b) {
            const int L = len[b], c = last[b];
            int found = -1, rk = -1;
            if (L >= 1 && c >= 0) {                               // class -> rank: at most one candidate is class c
                const unsigned long long q0 = __ballot(lane < n && cand_cls[lane] == c);
                const unsigned long long q1 = __ballot(lane + 64 < n && cand_cls[lane + 64] == c);
                rk = q0 ? __ffsll((long long)q0) - 1 : (q1 ? 64 + __ffsll((long long)q1) - 1 : -1);
            }
            if (rk >= 0) {
                const unsigned int ph = phash[b];
                unsigned long long mask = __ballot(lane < nb && len[lane] == L - 1 && hash[lane] == ph);
                const int nsym = L - 1;
                const unsigned int* lb = B_LAB(cur, b);
                for (int it = 0; it < nb && mask != 0ULL; ++it) {
                    const int bp = __ffsll((long long)mask) - 1;
                    mask &= mask - 1ULL;
                    const unsigned int* lp = B_LAB(cur, bp);
                    bool mism = false;
                    for (int w0 = 0; w0 * 2 < nsym; w0 += 64) {
                        const int w = w0 + lane;
                        if (w < tw && w * 2 < nsym) {
                            unsigned int x = lb[w] ^ lp[w];
                            if (nsym - w * 2 < 2) x &= 0xFFFFu;
                            mism = mism || x != 0u;
                        }
                    }
                    if (!__any(mism)) { found = bp; break; }      // live labellings are distinct: at most one can match
                }
            }
            if (lane == 0) { mpar[b] = found; mrank[b] = rk; }
        }
        __syncthreads();

        // ---- the entry table in insertion order
        const int stride = 1 + n;
        const int nE = nb * stride;
        const float pblank = prow0[0];
        for (int pos = lane; pos < nE; pos += 64) {
            const int b = pos / stride, k = pos - b * stride;
            float v;
            if (k == 0) {
                const float pr_nb = len[b] > 0 ? nonblank[b] * plast[b] : 0.f;
                const float pr_b = total[b] * pblank;
                v = pr_b + pr_nb;
            } else {
                const float pc = cand_p[k - 1];
                v = last[b] == cand_cls[k - 1] ? pc * blank[b] : pc * total[b];
            }
            tot[pos] = v;
        }
        __syncthreads();
        int nmerge;
        {
            const bool has = lane < nb && mpar[lane] >= 0;
            if (has) {
                const int pc = lane * stride, pe = mpar[lane] * stride + 1 + mrank[lane];
                const float m = tot[pc] + tot[pe];                // (pr_b + pr_nb) + ext; float addition commutes, so either touch order gives this
                if (pe < pc) { tot[pe] = m; tot[pc] = -2.f; }
                else { tot[pc] = m; tot[pe] = -2.f; }
            }
            nmerge = __popcll(__ballot(has));
        }
        __syncthreads();

        // ---- stable ranking: the top min(W, #entries) by total, the lower position first among equals.  Each lane keeps the best of its own
        // positions; the lane that owned a pick strikes it out and looks again.
        int npick = min(W, nE - nmerge);
        float bt = -1.f;
        int bpos = 0x7fffffff;
        for (int pos = lane; pos < nE; pos += 64) {
            const float v = tot[pos];
            if (v > bt) { bt = v; bpos = pos; }
        }
        for (int r = 0; r < npick; ++r) {
            float wt = bt;
            int wp = bpos;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ot = __shfl_xor(wt, o);
                const int op = __shfl_xor(wp, o);
                if (ot > wt || (ot == wt && op < wp)) { wt = ot; wp = op; }
            }
            if (wp < 0 || wp >= nE) { npick = r; break; }         // only totals that are not numbers can end here; wave-uniform
            if (lane == 0) sel[r] = wp;
            if ((wp & 63) == lane) {
                tot[wp] = -2.f;
                bt = -1.f;
                bpos = 0x7fffffff;
                for (int pos = lane; pos < nE; pos += 64) {
                    const float v = tot[pos];
                    if (v > bt) { bt = v; bpos = pos; }
                }
            }
        }
        __syncthreads();

        // ---- the picked entries become the next step's beams, in ranked order
        for (int r = 0; r < npick; ++r) {
            const int pos = sel[r];
            const int b = pos / stride, k = pos - b * stride;
            const int L = len[b];
            const int c = k > 0 ? cand_cls[k - 1] : last[b];
            // the other half of a merged entry: the extended beam of a copy, the copied beam of an extension
            int other = -1;
            if (k == 0) other = mpar[b];
            else {
                const unsigned long long mm = __ballot(lane < nb && mpar[lane] == b && last[lane] == c);
                if (mm) other = __ffsll((long long)mm) - 1;
            }
            if (lane == 0) {
                const int cb = k == 0 ? b : other;                // beam whose copy contributes (-1: none)
                const int eb = k == 0 ? other : b;                // beam whose extension by c contributes (-1: none)
                float nbv = 0.f, blv = 0.f, tv = 0.f;
                if (cb >= 0) {
                    const float pr_nb = len[cb] > 0 ? nonblank[cb] * plast[cb] : 0.f;
                    const float pr_b = total[cb] * pblank;
                    nbv = pr_nb;
                    blv = pr_b;
                    tv = pr_b + pr_nb;
                }
                if (eb >= 0) {
                    const float pc = k > 0 ? cand_p[k - 1] : cand_p[mrank[b]];   // p[c]; k == 0: c = last[b] is candidate mrank[b] (mpar[b] >= 0)
                    const float ext = last[eb] == c ? pc * blank[eb] : pc * total[eb];
                    if (cb >= 0) { nbv = nbv + ext; tv = tv + ext; }
                    else { nbv = ext; tv = ext; }
                }
                B_TOTAL(nxt)[r] = tv;
                B_NONBLANK(nxt)[r] = nbv;
                B_BLANK(nxt)[r] = blv;
                B_LEN(nxt)[r] = k == 0 ? L : L + 1;
                B_LAST(nxt)[r] = c;
                B_HASH(nxt)[r] = k == 0 ? hash[b] : hash_push(hash[b], c);
                B_PHASH(nxt)[r] = k == 0 ? phash[b] : hash[b];
            }
            const unsigned int* src = B_LAB(cur, b);
            unsigned int* dst = B_LAB(nxt, r);
            const int nw = ((k == 0 ? L : L + 1) + 1) >> 1;       // L + 1 <= t + 1 <= T <= tstride
            for (int w = lane; w < nw && w < tw; w += 64) {
                unsigned int v = w * 2 < L ? src[w] : 0u;
                if (k > 0 && w == (L >> 1)) {
                    const int sh = 16 * (L & 1);
                    v = (v & ~(0xFFFFu << sh)) | ((unsigned int)c << sh);
                }
                dst[w] = v;
            }
        }
        __syncthreads();
        cur = nxt;
        nb = npick;
    }

    // ---- the best labelling of the last step, collapsed: class 0 and symbols equal to their predecessor dropped
    const int L = nb > 0 ? B_LEN(cur)[0] : 0;
    const unsigned short* best = (const unsigned short*)B_LAB(cur, 0);
    int* op = out_text + (size_t)sd.x;
    int outn = 0;
    for (int i0 = 0; i0 < L; i0 += 64) {
        const int i = i0 + lane;
        const int s = i < L ? (int)best[i] : 0;
        const int pv = (i > 0 && i < L) ? (int)best[i - 1] : -1;
        const bool keep = i < L && s != 0 && s != pv;
        const unsigned long long km = __ballot(keep);
        if (keep) op[outn + __popcll(km & lt)] = s;               // < L <= T: inside the sequence's own rows
        outn += __popcll(km);
    }
    if (lane == 0) out_len[seq] = outn;
#undef B_TOTAL
#undef B_NONBLANK
#undef B_BLANK
#undef B_LEN
#undef B_LAST
#undef B_HASH
#undef B_PHASH
#undef B_LAB
}

size_t ctc_beam_wide_lds_bytes(int beam_width, int max_T) {
    const int tstride = (std::max(max_T, 1) + 1) & ~1;
    return beam_wide_lds_words(beam_width, tstride) * 4;
}

bool ctc_beam_wide_on_device(int beam_width, int C, int max_T) {
    return beam_width >= 1 && beam_width <= BBOCR_BEAM_DEVICE_MAX && C > 128 && C <= BBOCR_REC_CLASSES_MAX && max_T >= 0 && max_T <= (1 << 20) &&
           ctc_beam_wide_lds_bytes(beam_width, max_T) <= kCtcBeamLdsLimit;
}

hipError_t launch_ctc_beam_wide(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int* cand_n,
                                int* cand, int* out_text, int* out_len, hipStream_t s) {
    if (nseq <= 0) return hipSuccess;
    if (!probs || !seqs_dev || !cand_n || !cand || !out_text || !out_len || cs < C || rows > (size_t)INT32_MAX ||
        !ctc_beam_wide_on_device(beam_width, C, max_T))
        return hipErrorInvalidValue;
    const int tstride = (std::max(max_T, 1) + 1) & ~1;
    const float thr = (float)(0.5 / (double)C);
    if (rows > 0)
        hipLaunchKernelGGL(ctc_beam_cand_kernel, dim3((unsigned int)((rows + kCandWaves - 1) / kCandWaves)), dim3(64 * kCandWaves), 0, s, probs, rows, C, cs,
                           thr, cand_n, (int2*)cand);
    hipLaunchKernelGGL(ctc_beam_wide_kernel, dim3(nseq), dim3(64), ctc_beam_wide_lds_bytes(beam_width, max_T), s, probs, rows, C, cs, (const int*)cand_n,
                       (const int2*)cand, (const int2*)seqs_dev, nseq, beam_width, tstride, out_text, out_len);
    return hipGetLastError();
}
