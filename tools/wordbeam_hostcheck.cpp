// Stand-alone host program around csrc/word_dict.h and the host word beam search (csrc/ctc_wordbeam_host.h over ctc_beam_host.h): no HIP,
// nothing loaded into python.  tools/wordbeam_hostcheck.py builds it with -fsanitize=address,undefined and feeds it the cases of
// tests/ctc_wordbeam_cases.py with the Python restatement's answers.
//
// Input: whitespace-separated integers, records until a 0:
//   1 C T width space n_words { len sym* }* { T * C float32 bit patterns } n_text sym*        a search case and its expected text
//   2 n_words n_slots n_queries { len sym* }* { len sym* member }* longest_probe               a table, queries with their membership, its probe run
// Output: one line per record ("ok ..." or "MISMATCH ..."), then "<n> failures".
#include "ctc_wordbeam_host.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

static std::vector<int> read_string(std::istream& in) {
    int n = 0;
    in >> n;
    std::vector<int> s((size_t)std::max(n, 0));
    for (int& v : s) in >> v;
    return s;
}

static bool read_words(std::istream& in, int n_words, std::vector<uint16_t>& sym, std::vector<int>& off) {
    sym.clear();
    off.assign(1, 0);
    for (int i = 0; i < n_words; ++i) {
        for (int v : read_string(in)) sym.push_back((uint16_t)v);
        off.push_back((int)sym.size());
    }
    return (bool)in;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: wordbeam_hostcheck CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    int failures = 0, rec = 0, kind = 0;
    std::vector<uint16_t> sym;
    std::vector<int> off;
    while (in >> kind && kind != 0) {
        ++rec;
        if (kind == 1) {
            int C, T, width, space, n_words;
            in >> C >> T >> width >> space >> n_words;
            if (!read_words(in, n_words, sym, off)) return 2;
            const int cs = C + 3;                                  // a stride of its own: the columns behind C are never read
            std::vector<float> rows((size_t)T * cs, 7.f);
            for (int t = 0; t < T; ++t)
                for (int c = 0; c < C; ++c) {
                    uint32_t bits;
                    in >> bits;
                    memcpy(&rows[(size_t)t * cs + c], &bits, 4);
                }
            const std::vector<int> want = read_string(in);
            WdTable dict;
            bool ok = wd_build(sym.data(), off.data(), n_words, C, space, 0, dict);
            std::vector<int> got;
            if (ok) ctc_wordbeam_search_host(rows.data(), T, C, cs, width, space, &dict, got);
            // the segment rule on its own, and the search with no dictionary against the per-group beam search
            std::vector<int> a((size_t)T), seg((size_t)(T + 1) / 2 * 2 + 2), plain, word, none;
            for (int t = 0; t < T; ++t) a[t] = wd_argmax(&rows[(size_t)t * cs], C);
            const int ns = wd_segments(a.data(), 0, T, space, seg.data());
            for (int k = 0; k < ns; ++k) {
                BeamState st;
                ctc_beam_steps_host(&rows[(size_t)seg[2 * k] * cs], seg[2 * k + 1], C, cs, width, st);
                ctc_beam_collapse(st.entries[st.ranked()[0]].lab, word);
                if (k) plain.push_back(space);
                plain.insert(plain.end(), word.begin(), word.end());
            }
            ctc_wordbeam_search_host(rows.data(), T, C, cs, width, space, nullptr, none);
            ok = ok && got == want && none == plain && (int)got.size() <= T;
            failures += !ok;
            printf("%s search %d: C %d T %d width %d words %d groups %d text %zu\n", ok ? "ok" : "MISMATCH", rec, C, T, width, n_words, ns, got.size());
        } else if (kind == 2) {
            int n_words, n_slots, n_q, probe;
            in >> n_words >> n_slots >> n_q;
            if (!read_words(in, n_words, sym, off)) return 2;
            WdTable t;
            bool ok = wd_build(sym.data(), off.data(), n_words, 128, -1, (uint32_t)n_slots, t);
            int hits = 0;
            for (int q = 0; q < n_q; ++q) {
                const std::vector<int> s = read_string(in);
                int member;
                in >> member;
                const bool got = ok && wd_contains(t, s.data(), (int)s.size());
                std::vector<int> text((size_t)s.size() + 1);
                uint32_t h = 0;
                const int n = wd_collapse_hash(s.data(), (int)s.size(), text.data(), &h);       // (a query is a text: the hash of its collapse is its own
                ok = ok && got == (member != 0) && (n != (int)s.size() || h == wd_hash(s.data(), n));     //  whenever nothing collapses)
                hits += got;
            }
            in >> probe;
            ok = ok && t.longest_probe == probe;
            failures += !ok;
            printf("%s table %d: words %d kept %d slots %zu probe %d queries %d members %d\n", ok ? "ok" : "MISMATCH", rec, n_words, t.words, t.slots.size(),
                   t.longest_probe, n_q, hits);
        } else {
            return 2;
        }
        if (!in) return 2;
    }
    // tables the builder must refuse, and a lookup bounded by a probe count of 0
    {
        const uint16_t s0[] = {0}, s1[] = {5, 3}, s2[] = {200};
        const int o1[] = {0, 1}, o2[] = {0, 2}, o0[] = {0, 0};
        WdTable t;
        bool ok = !wd_build(s0, o1, 1, 8, 3, 0, t) && !wd_build(s1, o2, 1, 8, 3, 0, t) && !wd_build(s2, o1, 1, 97, 43, 0, t) && !wd_build(s1, o0, 1, 8, 7, 0, t) &&
                  !wd_build(s1, o2, 1, 8, 7, 3, t) && wd_build(s1, o2, 1, 8, 7, 0, t) && t.words == 1;
        const int q[] = {5, 3};
        ok = ok && wd_contains(t, q, 2) && !wd_contains(t, q, 1) && !wd_contains(t, q, 0) &&
             !wd_lookup<WdSerial>(t.slots.data(), (uint32_t)t.slots.size(), 0, t.pool.data(), (uint32_t)t.pool.size(), q, 2, wd_hash(q, 2));
        failures += !ok;
        printf("%s refusals\n", ok ? "ok" : "MISMATCH");
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
