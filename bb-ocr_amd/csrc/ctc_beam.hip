// CTC beam-search decode on the device: readtext(decoder='beamsearch') with beamWidth <= BBOCR_BEAM_DEVICE_MAX.
//
// Restates ctc_beam.cpp::ctc_beam_search_host (easyocr/utils.py::ctcBeamSearch without a language model) statement by statement, so that the
// text is the host's for every input, not approximately: float32 arithmetic in the host's association (the Makefile's -ffp-contract=off keeps
// pr_b + pr_nb an add of two products, and f32 subnormals are kept), the host's candidate rule (p[c] >= 0.5/C, the blank included), the host's
// stable ranking by total over the dictionary's insertion order, and the host's IDENTITY of dictionary entries: two entries are one when their
// labellings are equal symbol by symbol.
//
// One wave per sequence, a sequential loop over its T rows.  Everything the search keeps lives in LDS:
//   * the <= W live labellings as byte strings (C <= 128), double-buffered: [2][W][tstride];
//   * the live beams' state (total, nonblank, blank, length, last symbol, hash, hash of the labelling without its last symbol);
//   * the step's entry table: position b * (1 + n) + k is beam b's copy (k = 0) or its extension by the k-th candidate class in ascending
//     order (n candidates) -- exactly the host's insertion order, so "stable" is "lower position wins a tie".
// Within one step only a copy and an extension can be the same entry (copies are distinct live labellings, extensions of distinct beams or by
// distinct classes differ): copy(b) == ext(b', c) iff lab(b) == lab(b') + [c].  That is decided by comparing the bytes, wave-wide; the running
// hash only selects which pairs are worth comparing.  A prefix tree with parent pointers would NOT decide it: a labelling can leave the
// beam while its child stays and be re-created from the grandparent a step later under a new node.  The merged entry sits at the position of
// its first touch (the lower of the two), the other position is struck out.
//
// Every loop has a trip count fixed by T, W, C or tstride; every LDS index is bounded by those (the launch sizes the LDS block from them).
#include "bbocr.h"
#include "common.h"
#include "kernels.h"
#include "ctc_beam_steps.h"          // the step loop itself: shared with ctc_wordbeam.hip

#include <algorithm>

__global__ void __launch_bounds__(64) ctc_beam_kernel(const float* __restrict__ probs, size_t rows, int C, int cs, const int2* __restrict__ seqs,
                                                      int nseq, int W, int tstride, float thr, int* __restrict__ out_text,
                                                      int* __restrict__ out_len) {
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
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    BEAM_LDS_VIEWS(lds, W, W, C, tstride);
    int cur, nb, stride_final, nfinal;
    beam_search_steps<false>(lds, probs + (size_t)sd.x * cs, T, C, cs, W, W, tstride, thr, 0, cur, nb, stride_final, nfinal);

    // ---- the best labelling of the last step, collapsed: class 0 and symbols equal to their predecessor dropped
    const int L = nb > 0 ? B_LEN(cur)[0] : 0;
    const unsigned char* best = (const unsigned char*)B_LAB(cur, 0);
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
}

size_t ctc_beam_lds_bytes(int beam_width, int C, int max_T) {
    const int tstride = (std::max(max_T, 1) + 3) & ~3;
    return beam_dev::beam_lds_words(beam_width, beam_width, C, tstride) * 4;
}

bool ctc_beam_on_device(int beam_width, int C, int max_T) {
    return beam_width >= 1 && beam_width <= BBOCR_BEAM_DEVICE_MAX && C >= 1 && C <= 128 && max_T >= 0 && max_T <= (1 << 20) &&
           ctc_beam_lds_bytes(beam_width, C, max_T) <= kCtcBeamLdsLimit;
}

hipError_t launch_ctc_beam(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int* out_text,
                           int* out_len, hipStream_t s) {
    if (nseq <= 0) return hipSuccess;
    if (!probs || !seqs_dev || !out_text || !out_len || cs < C || !ctc_beam_on_device(beam_width, C, max_T)) return hipErrorInvalidValue;
    const int tstride = (std::max(max_T, 1) + 3) & ~3;
    const float thr = (float)(0.5 / (double)C);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(nseq), dim3(64), ctc_beam_lds_bytes(beam_width, C, max_T), s, probs, rows, C, cs, (const int2*)seqs_dev,
                       nseq, beam_width, tstride, thr, out_text, out_len);
    return hipGetLastError();
}
