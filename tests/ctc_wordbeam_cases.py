"""Inputs for the word-beam-search tests (test_ctc_wordbeam_cpu.py, test_gpu_ctc_wordbeam.py): seeded case families that each aim at one way
the device search (csrc/ctc_wordbeam.hip) can differ from the host's (csrc/ctc_wordbeam.cpp, which states the decoder), and a Python
restatement, wordbeam_search_py, that shows the inputs do aim there: every family carries its claims (the rank of the hit, the entry
count, the probe length), and check_claims() holds them against the restatement alone.

A case is ``(rows [T, C] float32, beam width, dictionary)``; the dictionary is a tuple of words, a word a tuple of class indices.  The
space class of a case is space_of(C).  Everything is seeded; nothing here needs a GPU or the library.
"""
import ctypes as C

import numpy as np

import ctc_beam_cases as beam

CS = beam.CS
F = np.float32
WORD_CANDIDATES = 20            # include/bbocr.h BBOCR_WORD_CANDIDATES
WORD_MAX = 1024                 # csrc/word_dict.h WD_WORD_MAX
HASH0, PRIME = 2166136261, 16777619


def space_of(Cn):
    """the class of ' ': english_g2's 43 at 97 classes, the last class of a small alphabet"""
    return 43 if Cn == 97 else Cn - 1


def decoy(Cn):
    """a word no text of these cases can equal (longer than every group): keeps a dictionary non-empty where a case wants no hit"""
    return tuple([1, 2] * 30)


# ------------------------------------------------------------------------------------------------ the restatement
def final_entries_py(rows, width):
    """ctc_beam_search_host's loop in float32 (beam.beam_search_py's, statement by statement) -> the LAST step's dictionary, ranked: a list of
    [labelling, total, touched by a copy, touched by an extension]"""
    T, Cn = rows.shape
    thr = F(0.5 / Cn)
    last = {(): [(), F(1), F(0), F(1), False, False]}
    for t in range(T):
        p = rows[t]
        cand = [int(c) for c in np.nonzero(p >= thr)[0]]
        live = sorted(last.values(), key=lambda e: -e[1])[:width]          # sorted() is stable
        curr = {}
        for src in live:
            lab = src[0]
            pr_nb = src[2] * p[lab[-1]] if lab else F(0)
            pr_b = src[1] * p[0]
            e = curr.setdefault(lab, [lab, F(0), F(0), F(0), False, False])
            e[2] = e[2] + pr_nb
            e[3] = e[3] + pr_b
            e[1] = e[1] + (pr_b + pr_nb)
            e[4] = True
            for c in cand:
                ext = p[c] * src[3] if (lab and lab[-1] == c) else p[c] * src[1]
                e = curr.setdefault(lab + (c,), [lab + (c,), F(0), F(0), F(0), False, False])
                e[2] = e[2] + ext
                e[1] = e[1] + ext
                e[5] = True
        last = curr
    return [[e[0], e[1], e[4], e[5]] for e in sorted(last.values(), key=lambda e: -e[1])]


def word_py(rows, width, words):
    """one word group -> (text, info): info = entries of the final step, the candidates' collapsed texts and labellings, the hit's rank"""
    ranked = final_entries_py(rows, width)
    cands = ranked[:WORD_CANDIDATES]
    texts = [tuple(beam.collapse(list(e[0]))) for e in cands]
    info = {"entries": len(ranked), "ranked": ranked, "texts": texts, "hit": None}
    for r, t in enumerate(texts):
        if t and t in words:
            info["hit"] = r
            return list(t), info
    return list(texts[0]), info


def segments_py(a, space):
    """the word-group rule on one sequence's arg-max row -> [(first, T)]"""
    out, start = [], None
    for t, v in enumerate(list(a) + [space]):
        if v != space and start is None:
            start = t
        if v == space and start is not None:
            out.append((start, t - start))
            start = None
    return out


def wordbeam_search_py(rows, width, dictionary, details=None):
    """ctc_wordbeam_search_host restated: groups from the rows' arg-max (numpy's: lowest index among equals), word_py per group, the words
    joined by one space class.  details: a list that receives word_py's info per group"""
    T, Cn = rows.shape
    space = space_of(Cn)
    words = set(dictionary)
    text = []
    for k, (a, n) in enumerate(segments_py(rows.argmax(axis=1), space) if T else []):
        w, info = word_py(rows[a:a + n], width, words)
        if details is not None:
            details.append(info)
        text += ([space] if k else []) + w
    return text


def beam_per_group_py(rows, width):
    """plain beam.beam_search_py on every group, joined: what an empty dictionary gives"""
    space = space_of(rows.shape[1])
    text = []
    for k, (a, n) in enumerate(segments_py(rows.argmax(axis=1), space)):
        text += ([space] if k else []) + beam.beam_search_py(rows[a:a + n], width)
    return text


# ------------------------------------------------------------------------------------------------ rows
def pattern_rows(pattern, Cn, seed, peak=0.9):
    """rows whose arg-max is pattern[t]: that class gets `peak`, the others share the rest at random"""
    rng = np.random.default_rng(seed)
    x = rng.random((len(pattern), Cn)) + 0.05
    x[np.arange(len(pattern)), pattern] = 0
    x = x / x.sum(axis=1, keepdims=True) * (1.0 - peak)
    x[np.arange(len(pattern)), pattern] = peak
    return x.astype(np.float32)


def group_rows(rng, T, Cn, power=1.0, blank_boost=1.0):
    """undecided rows of ONE word group: the space class stays far below every other class and below the candidate threshold"""
    x = rng.random((T, Cn)) ** power + 1e-3
    x[:, 0] *= blank_boost
    x[:, space_of(Cn)] = 1e-4
    out = beam._normalised(x)
    assert (out.argmax(axis=1) != space_of(Cn)).all()
    return out


# ------------------------------------------------------------------------------------------------ families: (rows, width, dictionary, claim)
def segmentation_cases():
    out = []
    sp = space_of(8)
    pats = {"no space": [1, 2, 2, 0, 3, 4], "all space": [sp] * 7, "leading": [sp, sp, 1, 2, 3], "trailing": [1, 0, 2, sp, sp],
            "doubled": [1, 2, sp, sp, 3, 0, 4, sp, sp, sp, 5], "one-row words": [1, sp, 2, sp, 3, sp, sp, 4], "single row": [2],
            "single space": [sp], "blank rows around": [0, 0, 1, sp, 0, 2, 0]}
    for i, (name, pat) in enumerate(pats.items()):
        rows = pattern_rows(pat, 8, 100 + i)
        words = ((1, 2), (3, 4), (2,), decoy(8))
        out.append((rows, 5, words, {"aim": name, "groups": len(segments_py(pat, sp))}))
    for end in (63, 64, 65):                                   # a word ENDING exactly at row 63 / 64 / 65 of 130 rows: the ballot's carry
        for start in (end - 3, 60, 0):
            pat = [sp] * 130
            for t in range(start, end):
                pat[t] = 1 + (t % 5)
            pat[100:104] = [2, 3, 0, 4]
            pat[129] = 5
            rows = pattern_rows(pat, 8, 200 + end + start)
            out.append((rows, 2, ((2, 3, 4), decoy(8)), {"aim": f"carry {start}-{end}", "groups": 3, "segment": (start, end - start)}))
    for Cn in (4, 8):                                          # arg-max ties between the space and another class: the lowest index decides
        sp2 = space_of(Cn)
        lo = np.full((6, Cn), 0.05, dtype=np.float32)
        lo[:, 1] = 0.9
        lo[2, 1] = lo[2, sp2] = 0.25                           # class 1 < space: the row stays in the group
        lo[4, :] = 0.125                                       # every class equal: the blank wins, not the space
        out.append((lo, 2, ((1,), decoy(Cn)), {"aim": "tie below the space", "groups": 1}))
    hi = np.full((6, 97), 0.001, dtype=np.float32)
    hi[:, 10] = 0.9
    hi[3, 10] = hi[3, 43] = hi[3, 90] = 0.25                   # class 10 < space 43 < class 90: class 10 wins -> one group
    hi2 = hi.copy()
    hi2[3, 10] = 0.001                                         # now the space ties with class 90 above it: the space wins -> two groups
    out.append((hi, 5, ((10,), decoy(97)), {"aim": "tie: lower class wins", "groups": 1}))
    out.append((hi2, 5, ((10,), decoy(97)), {"aim": "tie: space wins", "groups": 2}))
    return out


def _search(rng_seed, accept, tries=4000, Cns=(4, 8), widths=(2, 5), Ts=(2, 9), **kw):
    """draw single-group cases until accept(info, rows, width) returns a dictionary and a claim"""
    rng = np.random.default_rng(rng_seed)
    for _ in range(tries):
        Cn = int(rng.choice(Cns))
        T = int(rng.integers(Ts[0], Ts[1]))
        w = int(rng.choice(widths))
        rows = group_rows(rng, T, Cn, power=float(rng.choice([1.0, 2.0])), **kw)
        _, info = word_py(rows, w, set())
        got = accept(info, rows, w)
        if got is not None:
            return rows, w, got[0], got[1]
    raise AssertionError("the generator found no case for its claim")          # a bug in the generator, not a reason to lower the bar


def _hit_at(k, need_collapse=False, need_empty_first=False):
    def accept(info, rows, w):
        texts, sp = info["texts"], space_of(rows.shape[1])
        if len(texts) <= k or not texts[k] or texts[k] in texts[:k] or sp in texts[k] or texts[k] == texts[0]:
            return None
        if need_collapse and len(info["ranked"][k][0]) == len(texts[k]):
            return None
        if need_empty_first and texts[0] != ():
            return None
        return (texts[k], decoy(rows.shape[1])), {"hit": k}
    return accept


def rank_cases():
    """the hit is candidate 0, k (1 .. 18), 19, and candidate 20 -- just outside: the result must be candidate 0's text; no hit"""
    out = []
    for k in [0, 0] + list(range(1, 19)) * 2 + [19, 19, 19]:
        if k == 0:
            def first(info, rows, w):
                t = info["texts"][0]
                return ((t, decoy(rows.shape[1])), {"hit": 0}) if t and space_of(rows.shape[1]) not in t else None
            out.append(_search(3000 + len(out), first))
        else:
            out.append(_search(3000 + len(out), _hit_at(k), widths=(5, 32) if k > 8 else (2, 5), Cns=(8,) if k > 8 else (4, 8)))

    def outside(info, rows, w):
        ranked = info["ranked"]
        if len(ranked) <= WORD_CANDIDATES:
            return None
        t = tuple(beam.collapse(list(ranked[WORD_CANDIDATES][0])))
        if not t or t in info["texts"] or space_of(rows.shape[1]) in t:
            return None
        return (t, decoy(rows.shape[1])), {"hit": None, "outside": True}
    for i in range(3):
        out.append(_search(3100 + i, outside, widths=(5, 32), Cns=(8,)))
    for i in range(3):
        out.append(_search(3200 + i, lambda info, rows, w: ((decoy(rows.shape[1]),), {"hit": None})))
    return out


def collapse_cases():
    """a hit only after the collapse removes a blank or a repeat; an empty collapsed candidate ranked ahead of a hit"""
    out = [_search(3300 + i, _hit_at(k, need_collapse=True)) for i, k in enumerate((1, 2, 3, 5))]
    out += [_search(3400 + i, _hit_at(k, need_empty_first=True), blank_boost=6.0) for i, k in enumerate((1, 2, 4))]
    return out


def count_cases():
    """final tables of fewer than 20 entries (width 1, one candidate class: 2 entries), exactly 20, more; a merged entry among the final 20;
    equal totals among the final entries, so that only insertion order ranks them"""
    out = []
    one = np.zeros((5, 8), dtype=np.float32)
    one[:, 3] = 1.0
    out.append((one, 1, ((3,), decoy(8)), {"entries": 2, "hit": 0}))
    out.append((one[:1], 5, ((3,), decoy(8)), {"entries": 2, "hit": 0}))

    def entries(n_lo, n_hi, k):
        def accept(info, rows, w):
            if not (n_lo <= info["entries"] <= n_hi):
                return None
            got = _hit_at(min(k, info["entries"] - 1))(info, rows, w)
            return None if got is None else (got[0], dict(got[1], entries=info["entries"]))
        return accept
    out.append(_search(3500, entries(3, 19, 2)))
    out += [_search(3510 + i, entries(20, 20, k), widths=(5,)) for i, k in enumerate((1, 19))]
    out += [_search(3520 + i, entries(21, 999, k), widths=(5, 32)) for i, k in enumerate((3, 19))]

    def merged(info, rows, w):
        got = _hit_at(1)(info, rows, w)
        m = [r for r, e in enumerate(info["ranked"][:WORD_CANDIDATES]) if e[2] and e[3]]
        return None if got is None or not m else (got[0], dict(got[1], merged=m[0]))
    out += [_search(3530 + i, merged, Ts=(4, 9)) for i in range(3)]
    for Cn, row in ((4, [0.25, 0.25, 0.25, 0.25]), (8, [0.25, 0.25, 0.25, 0.125, 0.125, 0, 0, 0])):      # exact ties (powers of two)
        for T, w in ((2, 2), (3, 5), (3, 32)):
            rows = np.tile(np.array(row, dtype=np.float32), (T, 1))
            _, info = word_py(rows, w, set())
            tot = [e[1] for e in info["ranked"][:WORD_CANDIDATES]]
            k = next(r for r in range(1, len(tot)) if tot[r] == tot[r - 1] and _hit_at(r)(info, rows, w) is not None)
            words, claim = _hit_at(k)(info, rows, w)
            out.append((rows, w, words, dict(claim, tie=True)))
    return out


def join_cases():
    """empty words between non-empty ones; sequences whose text is exactly T symbols long"""
    sp = space_of(8)
    out = []
    for i, pat in enumerate(([1, 2, sp, 0, 0, sp, 3], [0, sp, 1, sp, 0, sp, 0, sp, 2], [0, 0, sp, 0])):
        rows = pattern_rows(pat, 8, 400 + i, peak=0.97)
        out.append((rows, 5, ((1, 2), (3,), decoy(8)), {"aim": "empty words", "groups": len(segments_py(pat, sp))}))
    for i, pat in enumerate(([1, sp, 2, sp, 3], [4], [1, sp, 2], [1, sp, 2, sp, 3, sp, 4, sp, 5, sp, 6, sp, 1])):
        rows = pattern_rows(pat, 8, 500 + i, peak=0.97)
        out.append((rows, 2, ((1,), (2,), decoy(8)), {"aim": "text of T symbols", "full": True}))
    wide = pattern_rows([20, 21, 43, 0, 22, 22, 43, 43, 0, 43, 23], 97, 600, peak=0.9)
    out.append((wide, 5, ((20, 21), (22,), decoy(97)), {"aim": "97 classes", "groups": 4}))
    return out


FAMILIES = {"segmentation": segmentation_cases, "rank": rank_cases, "collapse": collapse_cases, "count": count_cases, "join": join_cases}
RANK_FAMILIES = ("rank", "collapse")
_cache = {}


def family(name):
    """the family's cases, generated once per process (the rank families search for theirs)"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def check_claims(name):
    """every claim of family `name` holds for the Python restatement; -> the share of cases whose text differs from plain beam search per group"""
    differ = 0
    for rows, w, words, claim in family(name):
        details = []
        text = wordbeam_search_py(rows, w, words, details)
        plain = beam_per_group_py(rows, w)
        differ += text != plain
        assert len(text) <= rows.shape[0]
        assert rows.shape[1] in (4, 8, 97) and w in (1, 2, 5, 32) and (rows.shape[0] <= 48 or rows.shape[0] == 130), (name, rows.shape, w)
        if "groups" in claim:
            assert len(details) == claim["groups"], (name, claim, len(details))
        if "segment" in claim:
            assert claim["segment"] in segments_py(rows.argmax(axis=1), space_of(rows.shape[1])), (name, claim)
        if "hit" in claim:
            assert len(details) == 1 and details[0]["hit"] == claim["hit"], (name, claim, details[0]["hit"])
            assert (text != plain) == (claim["hit"] not in (None, 0)), (name, claim)
        if claim.get("outside"):
            t20 = tuple(beam.collapse(list(details[0]["ranked"][WORD_CANDIDATES][0])))
            assert t20 in words and text == list(details[0]["texts"][0])
        if "entries" in claim:
            assert details[0]["entries"] == claim["entries"], (name, claim, details[0]["entries"])
        if "merged" in claim:
            e = details[0]["ranked"][claim["merged"]]
            assert e[2] and e[3] and claim["merged"] < WORD_CANDIDATES
        if claim.get("tie"):
            tot = [e[1] for e in details[0]["ranked"]]
            assert tot[claim["hit"]] == tot[claim["hit"] - 1]
        if claim.get("full"):
            assert len(text) == rows.shape[0]
        if claim.get("aim") == "empty words":
            sp = space_of(rows.shape[1])
            assert any(a == sp and b == sp for a, b in zip(text, text[1:])) or text[:1] == [sp] or text[-1:] == [sp], text
        for info, (a, n) in zip(details, segments_py(rows.argmax(axis=1), space_of(rows.shape[1]))):
            assert list(info["texts"][0]) == beam.beam_search_py(rows[a:a + n], w)        # candidate 0 IS the beam search's answer
    if name == "count":
        n = [c[3]["entries"] for c in family(name) if "entries" in c[3]]
        assert 2 in n and 20 in n and any(2 < v < 20 for v in n) and any(v > 20 for v in n), n
    return differ / len(family(name))


# ------------------------------------------------------------------------------------------------ the table
def hash_py(word):
    h = HASH0
    for s in word:
        h = ((h ^ (s + 1)) * PRIME) & 0xFFFFFFFF
    return h


def table_py(words, nslots=0):
    """csrc/word_dict.h::wd_build restated -> (slots: list of word or None, longest probe run)"""
    words = list(dict.fromkeys(words))
    if nslots == 0:
        nslots = 1
        while nslots < 2 * len(words):
            nslots *= 2
    slots, longest = [None] * nslots, 0
    for w in words:
        k = 0
        while slots[(hash_py(w) + k) % nslots] is not None:
            k += 1
        slots[(hash_py(w) + k) % nslots] = w
        longest = max(longest, k + 1)
    return slots, longest


def colliding_words(length=10, alphabet=4):
    """two different words over classes 1 .. alphabet with the SAME 32-bit hash, found by enumerating all alphabet ** length of them"""
    n = alphabet ** length
    idx = np.arange(n, dtype=np.uint64)
    h = np.full(n, HASH0, dtype=np.uint64)
    for pos in range(length):
        sym = (idx // np.uint64(alphabet ** pos)) % np.uint64(alphabet) + np.uint64(1)
        h = ((h ^ (sym + np.uint64(1))) * np.uint64(PRIME)) & np.uint64(0xFFFFFFFF)
    order = np.argsort(h, kind="stable")
    same = np.nonzero(h[order][1:] == h[order][:-1])[0]
    assert len(same), "no collision in this space"
    word = lambda i: tuple(int((int(i) // alphabet ** pos) % alphabet + 1) for pos in range(length))
    a, b = word(order[same[0]]), word(order[same[0] + 1])
    assert a != b and hash_py(a) == hash_py(b)
    return a, b


def table_cases(seed=77):
    """-> [(words, nslots, queries, claim)]: words forced into one probe run longer than 8 (a deliberately small table), two different words
    of equal hash, the longest and the shortest admissible words, a word that is a prefix of another"""
    rng = np.random.default_rng(seed)
    out = []
    a, b = colliding_words()
    run = []
    while len(run) < 12:                                       # twelve words whose home is slot 5 of 32
        w = tuple(int(v) for v in rng.integers(1, 100, size=int(rng.integers(1, 9))))
        if hash_py(w) % 32 == 5 and w not in run:
            run.append(w)
    others = [tuple(int(v) for v in rng.integers(1, 100, size=4)) for _ in range(40)]
    out.append((run, 32, run + others + [w[:-1] for w in run if len(w) > 1] + [w + (1,) for w in run], {"probe": 12}))
    out.append(([a] + run, 32, [a, b] + run, {"collision": (a, b)}))
    out.append(([a, b], 0, [a, b, a[:-1], b + (1,)], {"collision": (a, b), "both": True}))
    long_w = tuple(int(v) for v in rng.integers(1, 128, size=WORD_MAX))
    out.append(([long_w, (7,), (7, 8), (7, 8, 9)], 0, [long_w, long_w[:-1], (7,), (8,), (7, 8), (7, 8, 9), (7, 8, 9, 9), (9,)], {"aim": "extremes"}))
    dense = [tuple(int(v) for v in rng.integers(1, 128, size=int(rng.integers(1, 7)))) for _ in range(60)]
    out.append((dense, 64, dense + others, {"aim": "dense", "probe_over": 8}))
    return out


def check_table_claims():
    for words, nslots, queries, claim in table_cases():
        _, longest = table_py(words, nslots)
        if "probe" in claim:
            assert longest == claim["probe"] > 8
        if "probe_over" in claim:
            assert longest > claim["probe_over"], longest
        if "collision" in claim:
            a, b = claim["collision"]
            assert hash_py(a) == hash_py(b) and a != b and len(a) == len(b) and (b in words) == bool(claim.get("both"))
        assert any(q in set(words) for q in queries) and any(q not in set(words) for q in queries)


def big_dictionary(n=50_000, seed=5):
    """a 50,000-word synthetic dictionary over classes 1 .. 96 without the space, and 10,000 probes, about half of them members"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 13, size=n)
    flat = rng.integers(1, 96, size=int(lens.sum()))
    flat[flat >= 43] += 1
    off = np.concatenate([[0], np.cumsum(lens)])
    words = [tuple(int(v) for v in flat[off[i]:off[i + 1]]) for i in range(n)]
    probes = [words[int(i)] for i in rng.integers(0, n, size=5000)]
    for i in rng.integers(0, n, size=5000):
        w = list(words[int(i)])
        w[int(rng.integers(0, len(w)))] = int(rng.integers(1, 43))
        probes.append(tuple(w))
    return words, probes


# ------------------------------------------------------------------------------------------------ ragged table
def ragged_table(nseq=300, seed=9):
    """300 sequences of T 0 .. 48 in shuffled order from one pool, trained-like rows with space rows between words -> (pool [rows, 97],
    seqs [nseq, 2], dictionary): the dictionary holds a lower-ranked candidate of every fifth group"""
    rng = np.random.default_rng(seed)
    Ts = np.concatenate([np.linspace(1, 48, nseq - 2).round().astype(int), [0, 0]])
    rng.shuffle(Ts)
    parts, words = [], [decoy(97)]
    for i, T in enumerate(Ts):
        if T == 0:
            continue
        rows = beam.peaked_rows(7000 + i, int(T), undecided=0.3)
        sp_rows = rng.random(int(T)) < 0.2
        rows[sp_rows] = pattern_rows([43] * int(sp_rows.sum()), 97, 8000 + i) if sp_rows.any() else rows[sp_rows]
        parts.append(rows)
        if i % 5 == 0:
            for a, n in segments_py(rows.argmax(axis=1), 43):
                texts = word_py(rows[a:a + n], 5, set())[1]["texts"]
                pick = [t for t in texts[1:] if t and 43 not in t and t != texts[0]]
                if pick:
                    words.append(pick[0])
    first = np.concatenate([[0], np.cumsum(Ts)[:-1]])
    return np.concatenate(parts), np.stack([first, Ts], axis=1).astype(np.int32), tuple(dict.fromkeys(words))


# ------------------------------------------------------------------------------------------------ the library's host functions
def flat_words(words):
    """-> (symbols uint16, word_off int32, n) as bbocr_set_dictionary / bbocr_host_ctc_wordbeam take them"""
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
    sym = np.array([v for w in words for v in w] or [0], dtype=np.uint16)
    return sym, off, len(words)


def host_text(lib, rows, w, words, cs=CS, space=None):
    """bbocr_host_ctc_wordbeam on one case: the yardstick"""
    T, Cn = rows.shape
    if T == 0:
        return []
    flat = np.ascontiguousarray(beam.embed(rows, cs))
    sym, woff, n = flat_words(words)
    off, idx = (C.c_int * 2)(), (C.c_int * T)()
    rc = lib.bbocr_host_ctc_wordbeam(flat.ctypes.data_as(C.POINTER(C.c_float)), 1, T, Cn, cs, w, space_of(Cn) if space is None else space,
                                     sym.ctypes.data_as(C.POINTER(C.c_uint16)), woff.ctypes.data_as(C.POINTER(C.c_int)), n, off, idx)
    assert rc == 0, rc
    return [idx[k] for k in range(off[1])]


def host_texts(lib, cases, cs=CS):
    import os
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(lambda c: host_text(lib, c[0], c[1], c[2], cs), cases))
