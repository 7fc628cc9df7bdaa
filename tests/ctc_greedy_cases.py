"""The case table of the greedy CTC stage, shared by test_ctc_greedy_cpu.py and test_gpu_ctc_greedy.py: logits float32 [rows, cs] with C
classes per row, a ragged table of sequences {first row, T} and a class mask, grouped in families that each aim at one way ctc.hip
can go wrong (the family docstrings say which).  The shapes are the smallest at which that can happen.

The columns C .. cs-1 of every case hold NaN and +inf in turn: they must never influence a result.  NaN or +inf INSIDE the C columns is out
of scope (the logits are the output of the model's Linear layer over finite activations, hence finite); -inf inside is in scope, it is
what a hard mask upstream of the stage would produce, and the stage gives such a class probability 0.

Everything is seeded; nothing here needs a GPU or the library.  CASES is built once at import (well under a second).
"""
import functools

import numpy as np

import ctc_greedy_ref as R

WIDTHS = (1, 2, 37, 63, 64, 65, 97, 127, 128)
STRIDES = ("C", 112, 128, 131)                 # 131: rows are not even 8-byte aligned
RAGGED_T = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 639)
BITS = (31, 32, 63, 64, 95, 96, 127)           # word and half-wave boundaries of the 128-bit mask
MAX_UNDECIDABLE = 0.01                         # cap on the share of undecidable sequences over the random cases (0 for the designed ones)


class Case:
    def __init__(self, name, C, cs, logits, seqs, mask=None, random=False, tie=False, expect_idx=None, expect_text=None):
        rows = len(logits)
        full = np.empty((rows, cs), dtype=np.float32)
        full[:, :C] = logits
        full[:, C:] = np.where(np.arange(cs - C) % 2 == 0, np.nan, np.inf).astype(np.float32)      # the poison behind C
        self.name, self.C, self.cs, self.logits, self.mask = name, C, cs, full, mask
        self.seqs = np.asarray(seqs, dtype=np.int32).reshape(-1, 2)
        self.random, self.tie = random, tie
        self.expect_idx = None if expect_idx is None else np.asarray(expect_idx, dtype=np.int64)
        self.expect_text = expect_text
        assert not np.isnan(logits).any() and not (logits == np.inf).any(), name                   # finite or -inf inside C
        assert all(r0 >= 0 and T >= 0 and r0 + T <= rows for r0, T in self.seqs), name

    @functools.cached_property
    def p64(self):
        return R.probs64(self.logits, self.C, self.mask)

    @functools.cached_property
    def bound(self):
        return R.prob_bound(self.logits, self.C, self.mask)

    @functools.cached_property
    def decidable(self):
        return R.decidable_rows(self.logits, self.C, self.mask)

    def uniform(self):
        """(n, T) when the table is n sequences of one T laid end to end in order over all rows (what the oracle's [b, T, C] expresses)"""
        n, T = len(self.seqs), int(self.seqs[0, 1])
        ok = T > 0 and n * T == len(self.logits) and all(int(r0) == k * T and int(t) == T for k, (r0, t) in enumerate(self.seqs))
        return (n, T) if ok else None

    def __repr__(self):
        return self.name


def _rng(*key):
    return np.random.default_rng([20250611, *key])


def _stride(C, s):
    return C if s == "C" else s


def _peaked(rng, T, C, sigma=4.0):
    """random logits with runs of repeats and blanks, the winner far ahead at most steps (the rest is decided by the noise)"""
    lg = rng.standard_normal((T, C)) * sigma
    if T and C > 1:
        cls = np.repeat(rng.integers(0, C, size=T), rng.integers(1, 4, size=T))[:T]
        cls[rng.random(T) < 0.3] = 0
        lg[np.arange(T), cls] += np.where(rng.random(T) < 0.8, 12.0, 0.0)
    return lg.astype(np.float32)


def width_cases():
    """every C at which the rows kernel changes shape (second half-wave idle up to 64, one class in it at 65, full at 128, a single
    class) at every stride; 3 sequences of T = 29 end to end, so the oracle can express them"""
    out = []
    for C in WIDTHS:
        for cs in sorted({_stride(C, s) for s in STRIDES if _stride(C, s) >= C}):
            rng = _rng(1, C, cs)
            out.append(Case(f"width/C{C}-cs{cs}", C, cs, _peaked(rng, 87, C), [(0, 29), (29, 29), (58, 29)], random=True))
    return out


def ragged_cases():
    """ONE launch over every T around the 64-step chunks of the collapse kernel, T = 0 included; the table is shuffled and independent of
    row order, and rows lie between the sequences that belong to none"""
    out = []
    for C, cs in ((97, 112), (128, 128)):
        rng = _rng(2, C)
        order = rng.permutation(len(RAGGED_T))
        gaps = rng.integers(0, 4, size=len(RAGGED_T))
        first, r = {}, 2                                        # two rows before the first sequence
        for k, T in enumerate(RAGGED_T):
            first[k] = r
            r += T + int(gaps[k])
        rows = r + 3
        lg = _peaked(rng, rows, C)
        out.append(Case(f"ragged/C{C}", C, cs, lg, [(first[k], RAGGED_T[k]) for k in order], random=True))
    return out


def _pattern(name, classes, C=97, cs=112, seed=0):
    """the arg-max of step t is classes[t]: a large offset on small noise"""
    T = len(classes)
    lg = (_rng(3, seed, T).standard_normal((T + 2, C)) * 1.0).astype(np.float32)
    cl = np.asarray(classes)
    lg[1 + np.arange(T), cl] += 30.0
    exp = np.full(T + 2, -1)
    exp[1:T + 1] = cl
    return Case(f"collapse/{name}", C, cs, lg, [(1, T)], expect_idx=exp, expect_text=[R.collapse(cl)])


def collapse_cases():
    """the collapse kernel's seams: lane 0 of a chunk compares with the last step of the previous chunk (t = 63|64, 127|128), the prefix
    popcount at a full mask, cnt against len"""
    blank70 = [0] * 70
    rep1 = list(blank70)
    rep1[60:68] = [64] * 8
    rep2 = [0] * 140
    rep2[120:136] = [96] * 16
    at64 = [1] * 100
    at64[64] = 0
    return [_pattern("all_blank", blank70, seed=1),
            _pattern("one_char_129", [63] * 129, seed=2),
            _pattern("a_blank_a", [1, 0, 1], seed=3),
            _pattern("repeat_across_63_64", rep1, seed=4),
            _pattern("repeat_across_127_128", rep2, seed=5),
            _pattern("blank_at_64", at64, seed=6),
            _pattern("distinct_64", list(range(1, 65)), seed=7),
            _pattern("alternation", [63 if t % 2 == 0 else 64 for t in range(131)], seed=8),
            _pattern("alternation_C128", [127 if t % 2 == 0 else 64 for t in range(131)], C=128, cs=131, seed=9)]


def _tie(name, C, cs, tied, mask=None, winner=None, seed=0):
    """6 rows whose classes `tied` hold exactly 6.0 over a background of multiples of 1/8 in [-3, 3]: their probabilities tie bit for bit
    in any evaluation that treats classes alike.  winner: the first unmasked tied class."""
    rng = _rng(4, seed)
    lg = np.clip(np.round(rng.standard_normal((6, C)) * 8) / 8, -3, 3).astype(np.float32)
    lg[:, list(tied)] = 6.0
    if winner is None:
        winner = min(tied)
    return Case(f"tie/{name}", C, cs, lg, [(0, 6)], mask=mask, tie=True, expect_idx=[winner] * 6, expect_text=[[winner] if winner else []])


def tie_cases():
    """exact ties: between a lane's two classes (c and c + 64: `q1 > bp` must be strict), across the half-wave seam (63 | 64), between
    neighbouring lanes (the butterfly's `oi < bi`), all classes at once, and with the winner masked"""
    const = Case("tie/constant_row", 97, 112, np.zeros((6, 97), dtype=np.float32), [(0, 6)], tie=True, expect_idx=[0] * 6, expect_text=[[]])
    const_nb = Case("tie/constant_row_blank_masked", 97, 112, np.zeros((6, 97), dtype=np.float32), [(0, 6)], mask=R.mask_words([0]), tie=True,
                    expect_idx=[1] * 6, expect_text=[[1]])
    return [_tie("3_67", 97, 112, (3, 67), seed=1), _tie("63_64", 97, 112, (63, 64), seed=2), _tie("5_6", 97, 112, (5, 6), seed=3),
            _tie("63_127_C128", 128, 128, (63, 127), seed=4), _tie("0_64_C65", 65, 112, (0, 64), seed=5), const,
            _tie("3_67_masked_3", 97, 112, (3, 67), mask=R.mask_words([3]), winner=67, seed=6),
            _tie("63_64_masked_63", 97, 112, (63, 64), mask=R.mask_words([63]), winner=64, seed=7),
            _tie("5_6_masked_5", 97, 112, (5, 6), mask=R.mask_words([5]), winner=6, seed=8), const_nb]


def mask_cases():
    """the 128-bit mask at its word (31|32, 95|96) and half-wave (63|64: ignore.x/.y feed classes 0..63, .z/.w classes 64..127) boundaries
    and at bit 127, one bit at a time and as the complement of {blank, k}; class k is the unmasked arg-max of every other row, so the single
    bit also REMOVES an arg-max.  Then a mask that holds the blank, and the two real character lists of test_ctc_matches_oracle."""
    from oracle import recog

    out = []
    for k in BITS:
        rng = _rng(5, k)
        lg = (rng.standard_normal((40, 128)) * 2.0).astype(np.float32)
        lg[::2, k] += 9.0
        out.append(Case(f"mask/bit{k}", 128, 128, lg, [(0, 17), (17, 23)], mask=R.mask_words([k]), random=True))
        lg = (rng.standard_normal((40, 128)) * 1.5).astype(np.float32)
        lg[::2, k] += 4.0
        out.append(Case(f"mask/only_blank_and_{k}", 128, 131, lg, [(0, 17), (17, 23)], mask=R.mask_words(set(range(128)) - {0, k}), random=True))
    rng = _rng(5, 1000)
    lg = (rng.standard_normal((40, 97)) * 2.0).astype(np.float32)
    lg[:, 40] += 10.0
    out.append(Case("mask/removes_argmax", 97, 112, lg, [(0, 40)], mask=R.mask_words([40]), random=True))
    out.append(Case("mask/holds_blank", 97, 112, _peaked(rng, 40, 97), [(0, 40)], mask=R.mask_words([0, 10, 50]), random=True))
    lists = {"allow_digits": set(recog.CHARACTER[1:]) - set("0123456789"), "block_vowels": set("aeiouAEIOU -")}
    for name, gone in lists.items():
        words = R.mask_words([i for i, ch in enumerate(recog.CHARACTER) if i and ch in gone])
        out.append(Case(f"mask/{name}", 97, 112, _peaked(rng, 58, 97), [(0, 29), (29, 29)], mask=words, random=True))
    return out


def range_cases():
    """the exponent range: tails that underflow to +0, a maximum next to FLT_MAX (x - max must not overflow into NaN), -inf entries"""
    out = []
    for name, spread in (("spread_80", 80.0), ("spread_1e4", 1e4)):
        rng = _rng(6, int(spread))
        out.append(Case(f"range/{name}", 97, 112, ((rng.random((30, 97)) * 2 - 1) * spread).astype(np.float32), [(0, 30)]))
    rng = _rng(6, 3)
    lg = (rng.standard_normal((30, 97)) * 4).astype(np.float32)
    lg[rng.random((30, 97)) < 0.2] = -3e38
    lg[np.arange(30), rng.integers(0, 97, size=30)] = 3e38
    out.append(Case("range/max_3e38", 97, 112, lg, [(0, 30)]))
    lg = (rng.standard_normal((30, 97)) * 4).astype(np.float32)
    lg[rng.random((30, 97)) < 0.3] = -np.inf
    lg[np.arange(30), rng.integers(0, 97, size=30)] = 5.0
    out.append(Case("range/minus_inf", 97, 112, lg, [(0, 30)]))
    return out


def product_cases():
    """pmax about 0.25 at every step (C = 5: one class ln(4/3) above four equal ones), all steps non-blank: the float32 product passes
    2^-126 after 63 steps, is subnormal at step 70 and +0 from step 75 on"""
    out = []
    for name, T in (("underflow_639", 639), ("subnormal_70", 70)):
        rng = _rng(7, T)
        lg = np.zeros((T, 5), dtype=np.float32)
        lg[:, 1] = (np.log(4 / 3) + 0.01 * (rng.random(T) - 0.5)).astype(np.float32)
        out.append(Case(f"prod/{name}", 5, 5, lg, [(0, T)], expect_idx=[1] * T, expect_text=[[1]]))
    return out


def sweep_case():
    """more rows than 8192 blocks x 4 waves: the rows kernel's grid-stride loop runs a second sweep"""
    rng = _rng(8)
    return [Case("sweep/33100_rows", 5, 5, _peaked(rng, 33100, 5), [(33050, 40), (0, 33000), (33010, 7)], random=True)]


CASES = width_cases() + ragged_cases() + collapse_cases() + tie_cases() + mask_cases() + range_cases() + product_cases() + sweep_case()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def undecidable_sequences(case):
    """(sequences with an undecidable step, sequences)"""
    return sum(not case.decidable[r0:r0 + T].all() for r0, T in case.seqs), len(case.seqs)


def assert_caps():
    """The decidability caps, a condition on the table and the reference alone (asserted by the CPU test, and again by the GPU test so that
    the exemption of undecidable rows cannot hide a failure): sequences with an undecidable step are at most 1 % of those of the random
    cases and none in a designed case -- other than the ties, whose rows are undecidable by construction (or, with the winner masked,
    all decidable) and are checked against their designed winner instead."""
    bad = tot = 0
    for case in CASES:
        b, n = undecidable_sequences(case)
        if case.random:
            bad, tot = bad + b, tot + n
        elif case.tie:
            assert not case.decidable.any() or (case.mask is not None and case.decidable.all()), case.name
        else:
            assert b == 0 and case.decidable.all(), case.name
    assert tot >= 100 and bad <= MAX_UNDECIDABLE * tot, (bad, tot)
    return bad, tot
