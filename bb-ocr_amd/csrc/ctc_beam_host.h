// The state and the step loop of the host beam search (ctc_beam.cpp states what they restate): the ONE copy of the loop, which
// ctc_beam_search_host ends by taking the best entry and the word search (ctc_wordbeam_host.h) by testing the final entries against a
// dictionary.  Standard headers only, so that tools/wordbeam_hostcheck.cpp can build it without the device toolchain.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

struct Beam {
    std::vector<int> lab;
    float total = 0.f, nonblank = 0.f, blank = 0.f;
};

struct BeamState {
    std::vector<Beam> entries;                    // dictionary values in insertion order
    std::map<std::vector<int>, int> index;        // labelling -> position in entries
    int at(const std::vector<int>& lab) {         // addBeam
        auto it = index.find(lab);
        if (it != index.end()) return it->second;
        const int i = (int)entries.size();
        entries.emplace_back();
        entries.back().lab = lab;
        index.emplace(lab, i);
        return i;
    }
    std::vector<int> ranked() const {             // BeamState.sort
        std::vector<int> o(entries.size());
        for (size_t i = 0; i < o.size(); ++i) o[i] = (int)i;
        std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return entries[a].total > entries[b].total; });
        return o;
    }
};

// T steps of ctcBeamSearch over mat [T, cs] -> the last step's dictionary, unpruned
inline void ctc_beam_steps_host(const float* mat, int T, int C, int cs, int beam_width, BeamState& last) {
    last = BeamState();
    {
        const int i = last.at({});
        last.entries[i].blank = 1.f;
        last.entries[i].total = 1.f;
    }
    const float thr = (float)(0.5 / (double)C);
    std::vector<int> cand, lab2;
    for (int t = 0; t < T; ++t) {
        const float* p = mat + (size_t)t * cs;
        cand.clear();
        for (int c = 0; c < C; ++c)
            if (p[c] >= thr) cand.push_back(c);
        BeamState curr;
        const std::vector<int> order = last.ranked();
        const int nb = std::min<int>(beam_width, (int)order.size());
        for (int b = 0; b < nb; ++b) {
            const Beam& src = last.entries[order[b]];
            const float pr_nb = src.lab.empty() ? 0.f : src.nonblank * p[src.lab.back()];
            const float pr_b = src.total * p[0];
            {
                Beam& e = curr.entries[curr.at(src.lab)];
                e.nonblank += pr_nb;
                e.blank += pr_b;
                e.total += pr_b + pr_nb;
            }
            for (int c : cand) {
                lab2 = src.lab;
                lab2.push_back(c);
                const float ext = (!src.lab.empty() && src.lab.back() == c) ? p[c] * src.blank : p[c] * src.total;
                Beam& e = curr.entries[curr.at(lab2)];
                e.nonblank += ext;
                e.total += ext;
            }
        }
        last = std::move(curr);
    }
}

// drop class 0 and every symbol equal to its predecessor in the labelling
inline void ctc_beam_collapse(const std::vector<int>& lab, std::vector<int>& text) {
    text.clear();
    for (size_t i = 0; i < lab.size(); ++i)
        if (lab[i] != 0 && !(i > 0 && lab[i - 1] == lab[i])) text.push_back(lab[i]);
}
