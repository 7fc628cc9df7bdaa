// The dictionary side of decoder='wordbeamsearch', compiled for host and device alike as gif_lzw.h / tiff_fax.h are: the hash of a
// class-index string, the open-addressing set of words and its bounded lookup, the rule that cuts a sequence's arg-max row into word groups,
// and the collapse of a labelling.  ctc_wordbeam.cpp states what the decoder is; ctc_wordbeam.hip runs these functions wave-wide;
// tools/wordbeam_hostcheck.cpp runs them under a sanitizer.
//
// The set: nslots (a power of two, by default the first one >= 2 * words) slots of {hash, offset, length} into ONE pool of symbols, linear
// probing from hash & (nslots - 1), no deletions -- so every slot between a word's home and its place is occupied.  A slot of length 0 is
// empty (no word is empty).  The build records the longest probe run (slots looked at to find the word placed farthest from its home); a
// lookup walks exactly that many slots at most, never "until an empty slot" on a table it has not built itself: an empty slot only ends the
// walk early.  MEMBERSHIP is decided by comparing the symbols; the hash picks the slots worth comparing, and a slot whose offset / length
// leave the pool is skipped, not read.
//
// Execution policy X of wd_lookup / wd_collapse (as tiff_codecs.h's):
//   X::equal(a, b, n)       a[0 .. n) == b[0 .. n), the same answer for everyone who asks
//   WdSerial below is the host's (and a single thread's); ctc_wordbeam.hip has the wave's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WD_HD __host__ __device__
#else
#define WD_HD
#endif

#ifndef BBOCR_WORD_CANDIDATES
#define BBOCR_WORD_CANDIDATES 20       /* include/bbocr.h: upstream's wordsearch(classes, ignore_idx, 20, dict_list) */
#endif

constexpr int WD_WORD_MAX = 1024;              // symbols of the longest admissible word
constexpr uint32_t WD_HASH0 = 2166136261u;

struct WdSlot {
    uint32_t hash, off, len;                   // len == 0: empty
};

WD_HD inline uint32_t wd_hash_push(uint32_t h, int c) { return (h ^ (uint32_t)(c + 1)) * 16777619u; }

template <class S> WD_HD inline uint32_t wd_hash(const S* sym, int n) {
    uint32_t h = WD_HASH0;
    for (int i = 0; i < n; ++i) h = wd_hash_push(h, (int)sym[i]);
    return h;
}

struct WdSerial {
    template <class A, class B> WD_HD static bool equal(const A* a, const B* b, int n) {
        for (int i = 0; i < n; ++i)
            if ((int)a[i] != (int)b[i]) return false;
        return true;
    }
};

// is sym[0 .. n) (hash h) a word of the table?  probe: the build's longest probe run -- the loop's whole trip count
template <class X, class P, class Q>
WD_HD inline bool wd_lookup(const WdSlot* slots, uint32_t nslots, int probe, const P* pool, uint32_t pool_n, const Q* sym, int n, uint32_t h) {
    if (n <= 0 || nslots == 0 || (nslots & (nslots - 1)) != 0 || !slots || !pool) return false;     // the empty text is never a member
    for (int i = 0; i < probe; ++i) {
        const WdSlot s = slots[(h + (uint32_t)i) & (nslots - 1)];
        if (s.len == 0) return false;
        if (s.hash != h || s.len != (uint32_t)n || s.off > pool_n || s.len > pool_n - s.off) continue;
        if (X::equal(pool + s.off, sym, n)) return true;
    }
    return false;
}

// the word groups of one sequence: a[t] = idx[first + t], groups are the maximal runs of consecutive t with a[t] != space.  Writes {first row,
// T} per group into seg (room for (T + 1) / 2 pairs: groups are at least one space row apart) -> their number
WD_HD inline int wd_segments(const int* idx, int first, int T, int space, int* seg) {
    int n = 0, start = -1;
    for (int t = 0; t <= T; ++t) {
        const bool in = t < T && idx[(size_t)first + t] != space;
        if (in && start < 0) start = t;
        if (!in && start >= 0) {
            seg[2 * n] = first + start;
            seg[2 * n + 1] = t - start;
            ++n;
            start = -1;
        }
    }
    return n;
}

// a row's arg-max, lowest index among equals (numpy argmax; what ctc_rows_kernel writes as idx)
WD_HD inline int wd_argmax(const float* p, int C) {
    int bi = 0;
    float bp = p[0];
    for (int c = 1; c < C; ++c)
        if (p[c] > bp) { bp = p[c]; bi = c; }
    return bi;
}

// the collapse of a labelling: class 0 and every symbol equal to its predecessor IN THE LABELLING dropped -> the text's length; *hash: its hash
template <class S, class O> WD_HD inline int wd_collapse_hash(const S* lab, int L, O* out, uint32_t* hash) {
    int n = 0;
    uint32_t h = WD_HASH0;
    for (int i = 0; i < L; ++i) {
        const int s = (int)lab[i];
        if (s != 0 && !(i > 0 && (int)lab[i - 1] == s)) {
            out[n++] = (O)s;
            h = wd_hash_push(h, s);
        }
    }
    if (hash) *hash = h;
    return n;
}

#include <vector>

// the host's table; the device gets `slots` as they are and `pool` narrowed to bytes (contexts of at most 128 classes)
struct WdTable {
    std::vector<WdSlot> slots;
    std::vector<uint16_t> pool;
    int words = 0;                 // distinct words kept
    int longest_probe = 0;
    int unmatchable = 0;           // kept words with two adjacent equal symbols: matched only through a labelling with a blank symbol between the pair
    int space = -1;                // the class of ' '
};

// words[i] = symbols[word_off[i] .. word_off[i + 1]); every symbol in 1 .. C - 1 and none the space class, length 1 .. WD_WORD_MAX.  nslots 0:
// the first power of two >= 2 * n_words, else a power of two above the number of words (tests force long probe runs with it).  Duplicates are
// kept once.  false: a bad table, t untouched.
inline bool wd_build(const uint16_t* symbols, const int* word_off, int n_words, int C, int space, uint32_t nslots, WdTable& t) {
    if (n_words < 0 || (n_words > 0 && (!symbols || !word_off)) || n_words > (1 << 26)) return false;
    for (int i = 0; i < n_words; ++i) {
        const long long a = word_off[i], b = word_off[i + 1];
        if (a < 0 || b - a < 1 || b - a > WD_WORD_MAX || (i == 0 && a != 0)) return false;
        for (long long k = a; k < b; ++k)
            if (symbols[k] < 1 || (int)symbols[k] >= C || (int)symbols[k] == space) return false;
    }
    if (nslots == 0) {
        nslots = 1;
        while (nslots < 2u * (uint32_t)n_words) nslots <<= 1;
    }
    if ((nslots & (nslots - 1)) != 0 || nslots <= (uint32_t)n_words) return false;
    WdTable w;
    w.space = space;
    w.slots.assign(nslots, WdSlot{0u, 0u, 0u});
    for (int i = 0; i < n_words; ++i) {
        const uint16_t* s = symbols + word_off[i];
        const int n = word_off[i + 1] - word_off[i];
        const uint32_t h = wd_hash(s, n);
        if (wd_lookup<WdSerial>(w.slots.data(), nslots, w.longest_probe, w.pool.data(), (uint32_t)w.pool.size(), s, n, h)) continue;
        uint32_t k = 0;
        while (w.slots[(h + k) & (nslots - 1)].len != 0) ++k;          // ends: fewer words than slots
        w.slots[(h + k) & (nslots - 1)] = WdSlot{h, (uint32_t)w.pool.size(), (uint32_t)n};
        w.pool.insert(w.pool.end(), s, s + n);
        if ((int)k + 1 > w.longest_probe) w.longest_probe = (int)k + 1;
        ++w.words;
        for (int j = 1; j < n; ++j)
            if (s[j] == s[j - 1]) { ++w.unmatchable; break; }
    }
    if (w.pool.empty()) w.pool.push_back(0);                            // a pointer to hand out
    t = std::move(w);
    return true;
}

inline bool wd_contains(const WdTable& t, const int* sym, int n) {
    return t.words > 0 &&
           wd_lookup<WdSerial>(t.slots.data(), (uint32_t)t.slots.size(), t.longest_probe, t.pool.data(), (uint32_t)t.pool.size(), sym, n, wd_hash(sym, n));
}
