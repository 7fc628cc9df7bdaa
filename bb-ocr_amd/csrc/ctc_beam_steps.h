// The step loop of the device beam search, shared by ctc_beam_kernel (ctc_beam.hip: one wave per sequence) and ctc_wordbeam_kernel
// (ctc_wordbeam.hip: one wave per word group).  ctc_beam.hip's header comment describes what it restates and how; this file is the ONE copy
// of it.  The callers differ in what they do behind the last step:
//   kWord == false   every step ends with its top min(W, #entries) entries moved into the other beam buffer; the caller reads beam 0.
//   kWord == true    the LAST step stops behind its ranking, which then covers min(ncand, #entries) positions (sel[0 .. nfinal)): the beams
//                    that entered the step are still in buffer `cur`, position pos = b * stride + k of the entry table is beam b's copy
//                    (k == 0) or its extension by cand_cls[k - 1] -- the caller forms the labellings it wants from those.
//
// LDS block (32-bit words): prow[128] | cand_cls[128] | cand_rank[128] | state[2][kStateFields][W] | mpar[W] | sel[nsel] | tot[W * (1 + C)] |
// labs[2][W][tstride / 4].  nsel = W for ctc_beam_kernel, max(W, ncand) for the word search.
//
// Every loop has a trip count fixed by T, W, C or tstride; every LDS index is bounded by those (the launch sizes the LDS block from them).
#pragma once
#include "common.h"

namespace beam_dev {

constexpr int kFixedWords = 3 * 128;                              // prow[128] | cand_cls[128] | cand_rank[128]
constexpr int kStateFields = 7;                                   // total, nonblank, blank, len, last, hash, phash (x 2 buffers)
constexpr unsigned int kHash0 = 2166136261u;

__host__ __device__ inline size_t beam_lds_words(int W, int nsel, int C, int tstride) {
    return (size_t)kFixedWords + (size_t)(2 * kStateFields + 1) * W /* + mpar[W] */ + (size_t)nsel + (size_t)W * (1 + C) + (size_t)2 * W * (tstride / 4);
}

__device__ inline unsigned int hash_push(unsigned int h, int c) { return (h ^ (unsigned int)(c + 1)) * 16777619u; }

}   // namespace beam_dev

// the views of the LDS block; `lds`, W, nsel, C and tstride are the caller's
#define BEAM_LDS_VIEWS(lds, W, nsel, C, tstride)                                                                                       \
    const int tw = (tstride) >> 2;                                /* words per labelling */                                           \
    float* prow = (float*)(lds);                                                                                                       \
    int* cand_cls = (int*)((lds) + 128);                          /* k -> class */                                                     \
    int* cand_rank = (int*)((lds) + 256);                         /* class -> k, -1: not a candidate of this step */                   \
    unsigned int* st = (lds) + beam_dev::kFixedWords;                                                                                  \
    int* mpar = (int*)(st + 2 * beam_dev::kStateFields * (W));    /* beam b's copy is the same entry as the extension of beam mpar[b] by last[b] */ \
    int* sel = mpar + (W);                                        /* ranked entry positions of the step */                             \
    float* tot = (float*)(sel + (nsel));                                                                                               \
    unsigned int* labs = (unsigned int*)(tot + (size_t)(W) * (1 + (C)))
#define B_TOTAL(q) ((float*)(st + ((q) * beam_dev::kStateFields + 0) * W))
#define B_NONBLANK(q) ((float*)(st + ((q) * beam_dev::kStateFields + 1) * W))
#define B_BLANK(q) ((float*)(st + ((q) * beam_dev::kStateFields + 2) * W))
#define B_LEN(q) ((int*)(st + ((q) * beam_dev::kStateFields + 3) * W))
#define B_LAST(q) ((int*)(st + ((q) * beam_dev::kStateFields + 4) * W))
#define B_HASH(q) (st + ((q) * beam_dev::kStateFields + 5) * W)
#define B_PHASH(q) (st + ((q) * beam_dev::kStateFields + 6) * W)
#define B_LAB(q, b) (labs + ((size_t)(q) * W + (b)) * tw)

// T steps over the rows at `rows0` (row stride cs).  Out: cur (the buffer that holds the result's beams), nb (their number); kWord and T >= 1:
// the beams that ENTERED the last step, stride (1 + the last step's candidate count) and nfinal (ranked positions in sel).  The caller has
// checked that T <= tstride and that the rows lie inside the table.
template <bool kWord>
__device__ __forceinline__ void beam_search_steps(unsigned int* lds, const float* __restrict__ rows0, int T, int C, int cs, int W, int nsel, int tstride,
                                                  float thr, int ncand_final, int& cur, int& nb, int& stride_final, int& nfinal) {
    using beam_dev::hash_push;
    using beam_dev::kHash0;
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    BEAM_LDS_VIEWS(lds, W, nsel, C, tstride);

    cur = 0;
    nb = 1;
    stride_final = 1;
    nfinal = 0;
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

        // ---- the row and its candidate classes, ascending
        const float* p = rows0 + (size_t)t * cs;
        const float p0 = lane < C ? p[lane] : 0.f;
        const float p1 = lane + 64 < C ? p[lane + 64] : 0.f;
        const bool c0 = lane < C && p0 >= thr, c1 = lane + 64 < C && p1 >= thr;
        const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
        const int n0 = __popcll(m0), n = n0 + __popcll(m1);
        const int r0 = __popcll(m0 & lt), r1 = n0 + __popcll(m1 & lt);
        prow[lane] = p0;
        prow[lane + 64] = p1;
        cand_rank[lane] = c0 ? r0 : -1;
        cand_rank[lane + 64] = c1 ? r1 : -1;
        if (c0) cand_cls[r0] = lane;
        if (c1) cand_cls[r1] = lane + 64;
        __syncthreads();

        // ---- which copies meet an extension: lab(b) == lab(b') + [last(b)], decided on the bytes
        for (int b = 0; b < nb; ++b) {
            const int L = len[b], c = last[b];
            int found = -1;
            if (L >= 1 && c >= 0 && c < C && cand_rank[c] >= 0) {
                const unsigned int ph = phash[b];
                unsigned long long mask = __ballot(lane < nb && len[lane] == L - 1 && hash[lane] == ph);
                const int nbytes = L - 1;
                const unsigned int* lb = B_LAB(cur, b);
                for (int it = 0; it < nb && mask != 0ULL; ++it) {
                    const int bp = __ffsll((long long)mask) - 1;
                    mask &= mask - 1ULL;
                    const unsigned int* lp = B_LAB(cur, bp);
                    bool mism = false;
                    for (int w0 = 0; w0 * 4 < nbytes; w0 += 64) {
                        const int w = w0 + lane;
                        if (w < tw && w * 4 < nbytes) {
                            unsigned int x = lb[w] ^ lp[w];
                            const int rem = nbytes - w * 4;
                            if (rem < 4) x &= (1u << (8 * rem)) - 1u;
                            mism = mism || x != 0u;
                        }
                    }
                    if (!__any(mism)) { found = bp; break; }      // live labellings are distinct: at most one can match
                }
            }
            if (lane == 0) mpar[b] = found;
        }
        __syncthreads();

        // ---- the entry table in insertion order
        const int stride = 1 + n;
        const int nE = nb * stride;
        for (int pos = lane; pos < nE; pos += 64) {
            const int b = pos / stride, k = pos - b * stride;
            float v;
            if (k == 0) {
                const float pr_nb = len[b] > 0 ? nonblank[b] * prow[last[b]] : 0.f;
                const float pr_b = total[b] * prow[0];
                v = pr_b + pr_nb;
            } else {
                const int c = cand_cls[k - 1];
                v = last[b] == c ? prow[c] * blank[b] : prow[c] * total[b];
            }
            tot[pos] = v;
        }
        __syncthreads();
        int nmerge;
        {
            const bool has = lane < nb && mpar[lane] >= 0;
            if (has) {
                const int pc = lane * stride, pe = mpar[lane] * stride + 1 + cand_rank[last[lane]];
                const float m = tot[pc] + tot[pe];                // (pr_b + pr_nb) + ext; float addition commutes, so either touch order gives this
                if (pe < pc) { tot[pe] = m; tot[pc] = -2.f; }
                else { tot[pc] = m; tot[pe] = -2.f; }
            }
            nmerge = __popcll(__ballot(has));
        }
        __syncthreads();

        // ---- stable ranking: the top min(W, #entries) by total, the lower position first among equals (the word search's last step: the
        // top min(ncand_final, #entries)).  Each lane keeps the best of its own positions; the lane that owned a pick strikes it out and
        // looks again.
        const bool final_word = kWord && t == T - 1;
        int npick = min(final_word ? ncand_final : W, nE - nmerge);
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
        if (final_word) {                                         // the caller tests these candidates against its dictionary
            stride_final = stride;
            nfinal = npick;
            return;
        }

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
                    const float pr_nb = len[cb] > 0 ? nonblank[cb] * prow[last[cb]] : 0.f;
                    const float pr_b = total[cb] * prow[0];
                    nbv = pr_nb;
                    blv = pr_b;
                    tv = pr_b + pr_nb;
                }
                if (eb >= 0) {
                    const float ext = last[eb] == c ? prow[c] * blank[eb] : prow[c] * total[eb];
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
            const int nw = ((k == 0 ? L : L + 1) + 3) >> 2;       // L + 1 <= t + 1 <= T <= tstride
            for (int w = lane; w < nw && w < tw; w += 64) {
                unsigned int v = w * 4 < L ? src[w] : 0u;
                if (k > 0 && w == (L >> 2)) {
                    const int sh = 8 * (L & 3);
                    v = (v & ~(0xFFu << sh)) | ((unsigned int)c << sh);
                }
                dst[w] = v;
            }
        }
        __syncthreads();
        cur = nxt;
        nb = npick;
    }
}
