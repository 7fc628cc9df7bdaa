"""Inputs for the tests of the device beam search over MORE than 128 classes (test_ctc_beam_wide_cpu.py, test_gpu_ctc_beam_wide.py):
probability rows as ctc_rows_wide_kernel writes them (float32, C classes embedded at row stride cs = C rounded up to 16), grouped in
families that each aim at one way ctc_beam_wide.hip can differ from ctc_beam.cpp::ctc_beam_search_host -- and a Python restatement of the
search with the tempting WRONG variants, which shows that the inputs do aim there.

A case is ``(rows [T, C] float32, beam width)``.  Everything is seeded; nothing here needs a GPU or the library.
"""
import numpy as np

from ctc_beam_cases import BEAM_DEVICE_MAX, beam_search_py, collapse, host_texts  # noqa: F401  (re-exported for the two test files)

F = np.float32
CLASSES = (129, 1009, 6719, 8192)
K = 128                 # csrc/kernels.h kBeamWideCand: candidates of a row the device search keeps
LDS_LIMIT = 65536       # csrc/kernels.h kCtcBeamLdsLimit
SCATTER = (1, 2, 63, 64, 127, 128, 255, 256, 257)


def cs_of(Cn):
    return (Cn + 15) // 16 * 16


def max_T(width):
    """longest sequence ctc_beam_wide_kernel takes at this width: ctc_beam_wide.hip::beam_wide_lds_words, T rounded up to 2"""
    words = 2 * K + 4 + (2 * 7 + 4) * width + width * (1 + K)
    return (LDS_LIMIT // 4 - words) // width // 2 * 2


def threshold(Cn):
    return F(0.5 / Cn)


def n_candidates(rows):
    """candidates per row, in float32 as every search counts them"""
    return (rows >= threshold(rows.shape[1])).sum(axis=1)


def overflows(rows):
    return bool((n_candidates(rows) > K).any()) if rows.shape[0] else False


def search_py(rows, width, wrong=None):
    """ctc_beam_search_host in float32, statement by statement -> the best labelling, collapsed.  wrong: one of the restatements a device
    search over a wide class axis invites --
      "sym8"       labellings are compared as 8-bit symbols: classes c and c + 256 are one symbol, and class 256 is the blank's;
      "cand_only"  p[last] and p[0] of a beam's copy are taken from the candidate list: a value below 0.5/C reads as 0;
      "truncate"   a row's candidate list stops at K entries and nothing falls back."""
    T, Cn = rows.shape
    thr = threshold(Cn)
    key = (lambda lab: tuple(s & 0xFF for s in lab)) if wrong == "sym8" else (lambda lab: lab)
    last = {(): [(), F(1), F(0), F(1)]}                                     # key -> [labelling, total, nonblank, blank]
    for t in range(T):
        p = rows[t]
        cand = [int(c) for c in np.nonzero(p >= thr)[0]]
        if wrong == "truncate":
            cand = cand[:K]
        q = np.where(p >= thr, p, F(0)) if wrong == "cand_only" else p      # what a copy reads
        live = sorted(last.values(), key=lambda e: -e[1])[:width]          # sorted() is stable
        curr = {}
        for lab, total, nonblank, blank in live:
            pr_nb = nonblank * q[lab[-1]] if lab else F(0)
            pr_b = total * q[0]
            e = curr.setdefault(key(lab), [lab, F(0), F(0), F(0)])
            e[2] = e[2] + pr_nb
            e[3] = e[3] + pr_b
            e[1] = e[1] + (pr_b + pr_nb)
            for c in cand:
                same = bool(lab) and (lab[-1] & 0xFF if wrong == "sym8" else lab[-1]) == (c & 0xFF if wrong == "sym8" else c)
                ext = p[c] * blank if same else p[c] * total
                e = curr.setdefault(key(lab + (c,)), [lab + (c,), F(0), F(0), F(0)])
                e[2] = e[2] + ext
                e[1] = e[1] + ext
        last = curr
    best = sorted(last.values(), key=lambda e: -e[1])[0][0]
    return collapse(list(best))


def _normalised(x):
    x = x.astype(np.float64)
    return (x / x.sum(axis=1, keepdims=True)).astype(np.float32)


def _scatter(small, pos, Cn):
    """[T, n] over a small alphabet -> [T, Cn]: column 0 stays the blank, column k goes to class pos[k - 1], every other class holds 0"""
    out = np.zeros((small.shape[0], Cn), dtype=np.float32)
    out[:, 0] = small[:, 0]
    out[:, list(pos)] = small[:, 1:]
    return out


def _small(rng, n_active):
    """ctc_beam_cases.small_alphabet_cases' recipe: width 3, flat rows and long T preferred, so that labellings leave the beam and come back"""
    T = 13 - int(10 * rng.random() ** 2)
    w = int(rng.choice([1, 2, 3], p=[0.1, 0.15, 0.75]))
    power = int(rng.choice([1, 3, 6], p=[0.7, 0.2, 0.1]))
    return _normalised(rng.random((T, n_active)) ** power), w


def scattered_cases(Cn, n=200, seed=20241020):
    """3-5 active classes (the blank and 2-4 drawn from SCATTER and C - 1), T 4-13, widths 1-3"""
    rng = np.random.default_rng(seed + Cn)
    where = sorted({c for c in SCATTER if c < Cn} | {Cn - 1})
    out = []
    for _ in range(n):
        n_active = int(rng.integers(3, 6))
        small, w = _small(rng, n_active)
        pos = np.sort(rng.choice(where, size=n_active - 1, replace=False))
        out.append((_scatter(small, pos, Cn), w))
    return out


ALIAS_SETS = ((1, 257), (1, 256), (1, 257, 513), (2, 256, 258), (1, 256, 257), (255, 511, 767), (1, 2, 257, 258))


def alias_cases(Cn, n=105, seed=77):
    """small alphabets whose classes agree in the low byte (c and c + 256: two symbols, two dictionary entries) or are byte strings of one
    another under a shift (1 = 01 00, 256 = 00 01: [1, 256] against [256, 1]); class 256 has the blank's low byte.  C >= 1009"""
    assert Cn > 767
    rng = np.random.default_rng(seed + Cn)
    out = []
    for i in range(n):
        pos = ALIAS_SETS[i % len(ALIAS_SETS)]
        small, w = _small(rng, 1 + len(pos))
        out.append((_scatter(small, pos, Cn), w))
    return out


def _pow2_below(x):
    """the largest power of two strictly below x"""
    return F(2.0) ** F(np.ceil(np.log2(float(x))) - 1)


def _spare(Cn, used, n):
    return [c for c in (5, 6, 7, 9, 10, 11) if c not in used and c < Cn][:n]


SUB_PAIRS = lambda Cn: ((1, 2), (1, Cn - 1), (127, 128), (255, 256))      # noqa: E731  (B, A), B < A; the last needs C > 256
SUB_WIDTHS = (2, 3, 5, BEAM_DEVICE_MAX)


def subthreshold_cases(Cn):
    """ties that only a sub-threshold p[last] breaks.  s: the largest power of two below 0.5/C.
         row 0  p[B] = p[A] = 0.5                 -> beams [B], [A] (B < A: [B] first)
         row 1  p[A] = s, p[D] = 1 - s            -> [B,D] = [A,D] = 0.5 (1 - s); the copy of [A] keeps 0.5 s, NOT a candidate's value
         row 2  p[D] = p[E] = 0.5                 -> [A] + D joins [A,D]: 0.25 (1 - s) + 0.25 s = 0.25 > [B,D]'s 0.25 (1 - s)
    The text is [A, D]; a search that reads p[A] from row 1's candidate list returns [B, D].  At width 2 the copy of [A] has left the beam
    after row 1 and both return [B, D]: the control."""
    s = _pow2_below(threshold(Cn))
    assert s < threshold(Cn)
    out = []
    for B, A in SUB_PAIRS(Cn):
        if A >= Cn or B >= A:
            continue
        D, E = _spare(Cn, (A, B), 2)
        rows = np.zeros((3, Cn), dtype=np.float32)
        rows[0, [B, A]] = 0.5
        rows[1, A], rows[1, D] = s, F(1) - s
        rows[2, [D, E]] = 0.5
        out += [(rows, w) for w in SUB_WIDTHS]
    return out


def subthreshold_blank_cases(Cn):
    """the mirror: the sub-threshold term is the BLANK's.
         row 0  p[B] = p[A] = 0.5                 -> beams [B], [A]
         row 1  p[0] = s, p[A] = 1 - s            -> the copy of [A]: pr_b 0.5 s + pr_nb 0.5 (1 - s) = 0.5 > [B,A] = 0.5 (1 - s)
    The text is [A]; with p[0] read as 0 the copy of [A] ties with [B,A], which was inserted first: [B, A].  Width 1 keeps [B] alone after
    row 0 and returns [B, A] either way: the control."""
    s = _pow2_below(threshold(Cn))
    out = []
    for B, A in SUB_PAIRS(Cn):
        if A >= Cn or B >= A:
            continue
        rows = np.zeros((2, Cn), dtype=np.float32)
        rows[0, [B, A]] = 0.5
        rows[1, 0], rows[1, A] = s, F(1) - s
        out += [(rows, w) for w in (1,) + SUB_WIDTHS]
    return out


def k_row(Cn=129):
    """exactly K equal candidates, the widest row the device takes: at C = 129, 128 classes at 2^-7 and one (class 5) at 0"""
    row = np.full(Cn, F(2.0) ** -7, dtype=np.float32)
    row[5] = 0
    row[K + 1:] = 0
    return row


def tie_cases(Cn):
    """repeated rows of exactly equal probabilities (powers of two: totals tie bit for bit) on classes that straddle 127 / 128 and 255 / 256;
    at C = 129 also the row of exactly K equal candidates"""
    sets = [(0, 127, 128, 1)] if Cn <= 256 else [(0, 127, 128, 255), (0, 128, 255, 256), (127, 255, 256, Cn - 1), (0, 1, 256, 257)]
    out = []
    for cl in sets:
        row = np.zeros(Cn, dtype=np.float32)
        row[list(cl)] = 0.25
        for T in (3, 7, 12):
            for w in (1, 5, BEAM_DEVICE_MAX):
                out.append((np.tile(row, (T, 1)), w))
    if Cn == 129:
        out += [(np.tile(k_row(), (T, 1)), w) for T in (1, 4) for w in (1, 5, BEAM_DEVICE_MAX)]
    return out


def crowded_row(Cn, n):
    """a row of n candidates, n in (K - 1, K, K + 1), whose HIGHEST candidate class (C - 1) holds 0.5 and wins the step; the others hold
    2^-8 (>= 0.5/C for every C >= 129), one of them as much more as brings the sum to 1.  A list cut at K entries loses the winner."""
    low = np.arange(Cn - 1) if Cn == 129 else np.unique(np.linspace(0, Cn - 2, K).round().astype(int))
    assert len(low) == K and n - 1 <= K
    row = np.zeros(Cn, dtype=np.float32)
    row[low[:n - 1]] = F(2.0) ** -8
    row[low[0]] += F(2.0) ** -8 * F(K + 1 - n)
    row[Cn - 1] = 0.5
    assert float(row.astype(np.float64).sum()) == 1.0
    return row


def _plain_rows(Cn, T, seed):
    """decided steps on classes away from C - 1: 0.75 on one class, 0.25 on the blank"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((T, Cn), dtype=np.float32)
    rows[:, 0] = 0.25
    rows[np.arange(T), rng.integers(1, min(Cn - 1, 100), size=T)] = 0.75
    return rows


def overflow_cases(Cn):
    """-> [(rows, width, overflowed)]: T = 5; a row of K - 1, K or K + 1 candidates at the first, a middle or the last step (only K + 1
    overflows); at C = 129 also a flat table, every class a candidate.  One table of these holds sequences that overflow beside ones that
    do not."""
    out = []
    for i, (n, where) in enumerate([(n, where) for n in (K - 1, K, K + 1) for where in (0, 2, 4)]):
        rows = _plain_rows(Cn, 5, 900 + i)
        rows[where] = crowded_row(Cn, n)
        for w in (1, 5, BEAM_DEVICE_MAX):
            out.append((rows, w, n > K))
    if Cn == 129:
        flat = np.full((4, Cn), F(1) / F(Cn), dtype=np.float32)
        out += [(flat, w, True) for w in (1, 5)]
    return out


def peaked_rows_wide(seed, T, Cn, undecided=0.2, plausible=10):
    """trained-like rows over C classes (ctc_beam_cases.peaked_rows' recipe): per step `plausible` classes with logits N(0, 1.5) and every
    other class 16 below, one class far ahead at most steps, runs of repeats and blanks, a share of undecided steps"""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((T, Cn)) * 1.5 - 16.0
    for t in range(T):
        lg[t, rng.choice(Cn, size=min(plausible, Cn), replace=False)] += 16.0
    cls = np.repeat(rng.integers(0, Cn, size=T), rng.integers(1, 4, size=T))[:T]
    cls[rng.random(T) < 0.4] = 0
    lg[:, 0] = rng.standard_normal(T) * 1.5 + 1.0                             # the blank is plausible at every step
    lg[np.arange(T), cls] = rng.standard_normal(T) * 1.5 + np.where(rng.random(T) < 1.0 - undecided, 9.0, 2.0) + (cls == 0)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return _normalised(e)


TRAINED_T = (1, 2, 63, 64, 65, 160)
TRAINED_W = (1, 5, 10, BEAM_DEVICE_MAX)


def trained_cases(Cn):
    return [(peaked_rows_wide(7000 + Cn + 10 * i + j, T, Cn), w) for i, T in enumerate(TRAINED_T) for j, w in enumerate(TRAINED_W)]


def ragged_table(Cn, nseq=60, seed=3):
    """60 sequences with T from 1 to 160 in shuffled order, and two of T = 0: -> (pool [rows, C], seqs [nseq + 2, 2])"""
    rng = np.random.default_rng(seed + Cn)
    Ts = np.concatenate([np.linspace(1, 160, nseq).round().astype(int), [0, 0]])
    rng.shuffle(Ts)
    pool = np.concatenate([peaked_rows_wide(9000 + Cn + i, int(T), Cn, undecided=0.1) for i, T in enumerate(Ts) if T > 0])
    first = np.concatenate([[0], np.cumsum(Ts)[:-1]])
    return pool, np.stack([first, Ts], axis=1).astype(np.int32)


def too_long_rows(Cn=1009):
    """one sequence longer than the device search's LDS block allows at width 32 (it fits at width 5)"""
    return peaked_rows_wide(4242, max_T(BEAM_DEVICE_MAX) + 2, Cn, undecided=0.05)


def families(Cn):
    """name -> [(rows, width)] for one class count (the overflow family apart: it carries its expected fallbacks)"""
    f = {"scattered": scattered_cases(Cn), "subthreshold": subthreshold_cases(Cn), "subthreshold_blank": subthreshold_blank_cases(Cn),
         "ties": tie_cases(Cn), "trained": trained_cases(Cn)}
    if Cn > 767:
        f["aliases"] = alias_cases(Cn)
    return f
