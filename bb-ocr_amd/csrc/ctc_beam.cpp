// CTC beam-search decode (host side of readtext(decoder='beamsearch')).
//
// Restates easyocr/utils.py::ctcBeamSearch(mat, classes, ignore_idx, lm=None, beamWidth) as called by
// CTCLabelConverter.decode_beamsearch from easyocr/recognition.py::recognizer_predict; the reference call site
// pipeline_demo/extractor/enhanced_extractor.py:520 keeps the default decoder ('greedy'), so this is SURVEY.md §8 row f4.
// The probabilities come from the device (ctc_rows_kernel: softmax, ignore mask, renormalisation); the search itself is a
// sequential walk over T with <= beamWidth live labellings and a handful of candidate classes per step -- dictionary work
// with an ordering contract, so it stays on the host, one sequence per worker thread.
//
// Upstream's behaviour kept bit for bit (float32 arithmetic throughout, as numpy does with a float32 `mat`):
//   * a step's candidate classes are all c with mat[t][c] >= 0.5/C, INCLUDING the blank (class 0), which is then an ordinary
//     symbol of the labelling;
//   * beams are ranked by prTotal (prText == 1 without a language model) with a STABLE descending sort over the insertion
//     order of the step's dictionary;
//   * the result drops class 0 and every symbol equal to its predecessor in the labelling.
#include "kernels.h"
#include "hostpool.h"

#include "ctc_beam_host.h"          // BeamState and the step loop: shared with the word search (ctc_wordbeam_host.h)

#include <atomic>
#include <thread>

void ctc_beam_search_host(const float* mat, int T, int C, int cs, int beam_width, std::vector<int>& text) {
    BeamState last;
    ctc_beam_steps_host(mat, T, C, cs, beam_width, last);
    text.clear();
    const std::vector<int> order = last.ranked();
    if (order.empty()) return;
    ctc_beam_collapse(last.entries[order[0]].lab, text);
}

void ctc_beam_search_batch(const float* probs, const int* seqs /* {first row, T} per sequence */, int nseq, int C, int cs, int beam_width,
                           std::vector<std::vector<int>>& texts, HostPool* pool) {
    texts.assign((size_t)nseq, {});
    auto one = [&](int i) { ctc_beam_search_host(probs + (size_t)seqs[2 * i] * cs, seqs[2 * i + 1], C, cs, beam_width, texts[i]); };
    if (pool) pool->parallel_for(nseq, one);
    else for (int i = 0; i < nseq; ++i) one(i);
}
