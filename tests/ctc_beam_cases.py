"""Inputs for the beam-search tests (test_ctc_beam_cases_cpu.py, test_gpu_ctc_beam.py): probability rows as ctc_rows_kernel writes them
(float32, C classes embedded at row stride cs), grouped in families that each aim at one way a device search can differ from
ctc_beam.cpp::ctc_beam_search_host -- and a Python restatement of the search that shows the inputs do aim there.

A case is ``(rows [T, C] float32, beam width)``.  Everything is seeded; nothing here needs a GPU or the library.
"""
import ctypes as C

import numpy as np

CS = 112                # row stride of the recogniser's logits / probabilities
BEAM_DEVICE_MAX = 32    # include/bbocr.h BBOCR_BEAM_DEVICE_MAX (the tests check it against bb_ocr_amd._lib.BEAM_DEVICE_MAX)
F = np.float32


def embed(rows, cs=CS):
    """[T, C] -> [T, cs]: the columns behind C hold a value no search may read as a probability"""
    out = np.full((rows.shape[0], cs), 7.0, dtype=np.float32)
    out[:, :rows.shape[1]] = rows
    return out


def collapse(lab):
    return [s for i, s in enumerate(lab) if s != 0 and not (i > 0 and lab[i - 1] == s)]


def greedy_collapse(rows):
    return collapse([int(c) for c in rows.argmax(axis=1)])


def beam_search_py(rows, width, parent_pointer=False, trace=None):
    """ctc_beam_search_host in float32, statement by statement -> the best labelling, collapsed.

    parent_pointer=True is the tempting WRONG variant: labellings are nodes of a prefix tree, and the copy of beam b meets the extension
    (b', c) only when b's parent POINTER is b' -- a labelling that left the beam and is re-created from its grandparent gets a new node
    that its surviving child does not point to, so the two halves of one dictionary entry stay apart.
    trace: a list that receives, per step, the ranked totals of the step's entries (float32)."""
    T, Cn = rows.shape
    thr = F(0.5 / Cn)
    ids = iter(range(1, 1 << 30))
    # entry: [labelling, total, nonblank, blank, node, parent node]
    last = {(): [(), F(1), F(0), F(1), 0, -1]}
    for t in range(T):
        p = rows[t]
        cand = [int(c) for c in np.nonzero(p >= thr)[0]]
        live = sorted(last.values(), key=lambda e: -e[1])[:width]          # sorted() is stable
        curr = {}
        for src in live:
            lab = src[0]
            pr_nb = src[2] * p[lab[-1]] if lab else F(0)
            pr_b = src[1] * p[0]
            e = curr.setdefault(src[4] if parent_pointer else lab, [lab, F(0), F(0), F(0), src[4], src[5]])
            e[2] = e[2] + pr_nb
            e[3] = e[3] + pr_b
            e[1] = e[1] + (pr_b + pr_nb)
            for c in cand:
                ext = p[c] * src[3] if (lab and lab[-1] == c) else p[c] * src[1]
                if parent_pointer:
                    child = [b[4] for b in live if b[5] == src[4] and b[0][-1] == c]
                    key = child[0] if child else ("new", src[4], c)
                else:
                    key = lab + (c,)
                e = curr.get(key)
                if e is None:
                    e = curr[key] = [lab + (c,), F(0), F(0), F(0), next(ids), src[4]]
                e[2] = e[2] + ext
                e[1] = e[1] + ext
        last = curr
        if trace is not None:
            trace.append(np.array(sorted((e[1] for e in last.values()), reverse=True), dtype=np.float32))
    best = sorted(last.values(), key=lambda e: -e[1])[0][0]
    return collapse(list(best))


def _normalised(x):
    x = x.astype(np.float64)
    return (x / x.sum(axis=1, keepdims=True)).astype(np.float32)


def small_alphabet_cases(n=2000, seed=20240607):
    """C 3-5, T 4-13, width 1-3, rows of rng.random ** (1, 3 or 6): small enough that labellings fall out of the beam and come back.

    Every value of the four ranges occurs, but not equally often: a beam of width 1 never holds a labelling and its child together, so it
    cannot merge anything, and peaked rows (power 6) or few steps rarely push a labelling out and bring it back.  Drawn uniformly, 1.5 %
    of the cases tell parent-pointer merging from real equality; the weights below (width 3, power 1 and long T preferred) give 6.8 %."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        Cn = int(rng.integers(3, 6))
        T = 13 - int(10 * rng.random() ** 2)
        w = int(rng.choice([1, 2, 3], p=[0.1, 0.15, 0.75]))
        power = int(rng.choice([1, 3, 6], p=[0.7, 0.2, 0.1]))
        out.append((_normalised(rng.random((T, Cn)) ** power), w))
    return out


def tie_cases():
    """repeated rows with exactly equal probabilities (all powers of two, so sums and products are exact and totals tie bit for bit)"""
    out = []
    for Cn, row in ((4, [0.25, 0.25, 0.25, 0.25]), (3, [0.5, 0.25, 0.25]), (5, [0.25, 0.25, 0.25, 0.125, 0.125]), (3, [0.25, 0.5, 0.25])):
        for T in (3, 7, 12):
            for w in (1, 2, 3, 5, 10):
                out.append((np.tile(np.array(row, dtype=np.float32), (T, 1)), w))
    wide = np.zeros((9, 97), dtype=np.float32)                  # C = 97: four equal classes, the blank among them
    wide[:, [0, 11, 12, 40]] = 0.25
    wide2 = wide.copy()
    wide2[4:] = 0
    wide2[4:, [0, 12, 90, 96]] = 0.25
    for w in (1, 2, 5, 10, BEAM_DEVICE_MAX):
        out.append((wide, w))
        out.append((wide2, w))
    return out


def underflow_rows(seed=7, T=639):
    """T = 639, C = 97, near-flat: every class is a candidate at every step and each step costs a labelling a factor of ~1/97, so the
    totals run through the subnormal range to 0 within the first tens of steps and stay tied at 0 from there on"""
    rng = np.random.default_rng(seed)
    return _normalised(1.0 + 0.02 * rng.random((T, 97)))


def underflow_cases():
    rows = underflow_rows()
    return [(rows, 1), (rows, 5), (rows[:160], BEAM_DEVICE_MAX)]


def saturation_cases():
    """all 97 classes are candidates: p = float32(1/97) exactly (every total ties), and a ragged variant of it"""
    flat = np.full((6, 97), F(1) / F(97), dtype=np.float32)
    rng = np.random.default_rng(11)
    ragged = _normalised(1.0 + 0.6 * rng.random((9, 97)))       # min/max ratio 1.6: every class stays above 0.5/97
    assert (ragged >= F(0.5 / 97)).all()
    return [(r, w) for r in (flat, ragged) for w in (1, 5, BEAM_DEVICE_MAX)]


def peaked_rows(seed, T, undecided=0.2):
    """trained-like rows at C = 97: one class far ahead at most steps, runs of repeats and blanks, a share of undecided steps"""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((T, 97)) * 1.5
    cls = np.repeat(rng.integers(0, 97, size=T), rng.integers(1, 4, size=T))[:T]
    cls[rng.random(T) < 0.4] = 0
    lg[np.arange(T), cls] += np.where(rng.random(T) < 1.0 - undecided, 9.0, 2.0)
    lg[:, 0] += 1.0
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return _normalised(e)


def peaked_cases():
    return [(peaked_rows(100 + i, T), w) for i, (T, w) in enumerate(((1, 5), (2, 1), (31, 5), (63, 2), (64, 10), (65, 5), (159, BEAM_DEVICE_MAX)))]


def ragged_table(nseq=300, seed=3):
    """300 sequences with T from 1 to 639 in shuffled order (two more of T = 0 among them), rows of one pool: -> (pool [rows, C],
    seqs [nseq, 2]).  Few undecided steps: the host search is O(T^2) per sequence and pays for every candidate"""
    rng = np.random.default_rng(seed)
    Ts = np.concatenate([np.linspace(1, 639, nseq).round().astype(int), [0, 0]])
    rng.shuffle(Ts)
    pool = np.concatenate([peaked_rows(1000 + i, int(T), undecided=0.04) for i, T in enumerate(Ts) if T > 0])
    first = np.concatenate([[0], np.cumsum(Ts)[:-1]])
    return pool, np.stack([first, Ts], axis=1).astype(np.int32)


def host_texts(lib, cases, cs=CS):
    """bbocr_host_ctc_beam on each (rows, width): the yardstick.  One call per case on a few threads (ctypes drops the GIL)"""
    import os
    from concurrent.futures import ThreadPoolExecutor

    def one(case):
        rows, w = case
        T, Cn = rows.shape
        if T == 0:
            return []
        flat = np.ascontiguousarray(embed(rows, cs))
        off, idx = (C.c_int * 2)(), (C.c_int * T)()
        assert lib.bbocr_host_ctc_beam(flat.ctypes.data_as(C.POINTER(C.c_float)), 1, T, Cn, cs, w, off, idx) == 0
        return [idx[k] for k in range(off[1])]

    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(one, cases))
