// The host word beam search of one sequence, as ctc_wordbeam.cpp's header comment defines it.  Standard headers, word_dict.h and the host
// beam search's step loop only: tools/wordbeam_hostcheck.cpp builds it without the device toolchain.
#pragma once
#include "ctc_beam_host.h"
#include "word_dict.h"

// one word group: the beam search's loop over its rows, then the first of the final step's BBOCR_WORD_CANDIDATES best entries whose collapsed
// text is a word of the dictionary -- candidate 0 when none is
inline void ctc_wordbeam_word_host(const float* mat, int T, int C, int cs, int beam_width, const WdTable* dict, std::vector<int>& word) {
    BeamState last;
    ctc_beam_steps_host(mat, T, C, cs, beam_width, last);
    word.clear();
    const std::vector<int> order = last.ranked();
    if (order.empty()) return;
    const int ncand = std::min<int>(BBOCR_WORD_CANDIDATES, (int)order.size());
    std::vector<int> text;
    for (int r = 0; dict && r < ncand; ++r) {
        ctc_beam_collapse(last.entries[order[r]].lab, text);
        if (!text.empty() && wd_contains(*dict, text.data(), (int)text.size())) {
            word = text;
            return;
        }
    }
    ctc_beam_collapse(last.entries[order[0]].lab, word);
}

// one sequence mat [T, cs]: its word groups, each searched on its own rows, joined by one `space` class
inline void ctc_wordbeam_search_host(const float* mat, int T, int C, int cs, int beam_width, int space, const WdTable* dict, std::vector<int>& text) {
    text.clear();
    if (T <= 0) return;
    std::vector<int> a((size_t)T), seg((size_t)(T + 1) / 2 * 2 + 2), word;
    for (int t = 0; t < T; ++t) a[t] = wd_argmax(mat + (size_t)t * cs, C);
    const int n = wd_segments(a.data(), 0, T, space, seg.data());
    for (int k = 0; k < n; ++k) {
        ctc_wordbeam_word_host(mat + (size_t)seg[2 * k] * cs, seg[2 * k + 1], C, cs, beam_width, dict, word);
        if (k > 0) text.push_back(space);
        text.insert(text.end(), word.begin(), word.end());
    }
}
