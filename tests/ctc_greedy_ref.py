"""Plain references of the greedy CTC stage (ctc.hip: ctc_rows_kernel + ctc_collapse_kernel, and ctc_decode's host pow), and the check
functions that test_gpu_ctc_greedy.py applies to the device's outputs and test_ctc_greedy_cpu.py to stand-ins with planted defects.

The stage is checked in two halves.  The probabilities are compared with a float64 softmax under a DERIVED allowance (prob_bound).
Everything behind them -- arg-max, pmax, collapse, cnt, the float32 product, the confidence -- is an exact function of the device's own
probabilities / idx / pmax and is compared bit for bit with a restatement that takes those as its input.

Masks are the 4 x 32-bit words of launch_ctc (bit c of word c >> 5 removes class c), or None.  Nothing here needs a GPU or the library.
"""
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of float32
TINY = 2.0 ** -126                # smallest normal float32
K = 19.0
F = np.float32

# sentinels the caller puts into the stage's output tensors before a launch
S_IDX, S_OUT, S_CTC, S_PROB = -7, -9, 0x5A5A5A5A, -5.0


def mask_bits(mask, C):
    """-> bool [C], True where the class is removed"""
    if mask is None:
        return np.zeros(C, dtype=bool)
    return np.array([(int(mask[c >> 5]) >> (c & 31)) & 1 for c in range(C)], dtype=bool)


def mask_words(classes):
    w = [0, 0, 0, 0]
    for c in classes:
        w[c >> 5] |= 1 << (c & 31)
    return tuple(w)


def _soft64(logits, C, mask):
    x = np.asarray(logits)[:, :C].astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        d = m - x                                              # >= 0; inf for a -inf entry
    e = np.exp(-d)
    e[:, mask_bits(mask, C)] = 0.0
    return x, m, d, e


def probs64(logits, C, mask=None):
    """softmax over the first C columns in float64, masked classes zeroed, the rest renormalised (recognizer_predict's
    F.softmax / preds_prob[:, :, ignore_idx] = 0 / division by the remaining sum, as ONE division: the two are equal in exact arithmetic)"""
    _, _, _, e = _soft64(logits, C, mask)
    return e / e.sum(axis=1, keepdims=True)


def prob_bound(logits, C, mask=None):
    """Per-element allowance for a float32 evaluation of probs64:  (|x - max| + K) * 2^-24 * p  +  2^-126,  K = 19.

    Derivation (first order in u = 2^-24; the kernel's order of operations, but every step is what ANY float32 softmax + mask +
    renormalisation has to do).  Write d_j = max - x_j, E_j = exp(-d_j), p_j = E_j / sum of E over the unmasked classes.
      1. fl(x_j - max) is one rounding: the exponent is off by at most d_j * u, which is a RELATIVE error of d_j * u in E_j.  This is
         the |x - max| term; it is the only one that grows with the input.
      2. expf: HIP documents a maximum error of 1 ulp for expf; 1 ulp is at most 2^-23 = 2u relative.            e_j = E_j (1 + eta_j), |eta_j| <= (d_j + 2) u
      3. S = butterfly sum of the e_j (e0 + e1, then six xor steps: 7 roundings of positive terms), the same float in every lane.
      4. q_j = fl(e_j / S), one correctly rounded division: q_j = e_j / S * (1 + delta), |delta| <= u.
      5. norm = butterfly sum of the unmasked q_j: 7 roundings of positive terms.  A sum of positive terms inherits the p-weighted mean of
         its terms' relative errors, sum_k p_k (d_k + 2 + 1) u, and  sum_k p_k d_k = H(p) - ln(sum_k exp(-d_k)) <= ln C <= ln 128 < 4.86:
         the entropy H(p) is at most ln C and the sum holds the term exp(0) = 1.
      6. q'_j = fl(q_j / norm), one correctly rounded division.  S is the SAME float in numerator and denominator and cancels exactly, so
         the 7 roundings of step 3 do not reach the result.
    Sum for element j:  (d_j + 2) + 1   [e_j, first division]
                      + (4.86 + 3) + 7   [norm: inherited mean, its own roundings]
                      + 1   [second division]              = d_j + 18.86,   K = 19 (the 0.14 u left over exceeds every second-order
    term: (d u)^2 < 1e-10 for d <= 150, beyond which E underflows).
    Absolute floor 2^-126, the smallest normal float32: below it e_j and q_j are rounded to a multiple of 2^-149 (float32 subnormals are
    kept in this build), and have no relative precision to speak of.

    Where this is a theorem and where it is only the rule: step 5 takes `max` to be an unmasked class, and the floor takes the
    renormalisation to magnify nothing.  With the row's arg-max masked, d_k = D + d'_k with D = max - (largest unmasked logit): the
    roundings of fl(x_j - max) and fl(x_top' - max) are independent and both reach q'_j, so a bound that holds for EVERY float32 evaluation
    is (d_j + D + K) u p, and its floor 2^-148 / (unmasked share of the row) once that share is below 2^-22.  The rule is asserted as
    stated, without D, on those rows too (mask/bit*, mask/removes_argmax, mask/allow_digits with shares down to 1e-7): an evaluation
    reaches the worst case of two independent roundings only by coincidence, and on the table's rows torch's float32 softmax stays at
    0.63 of the stated allowance and the device at the figure in test_gpu_ctc_greedy.py.  A failure confined to rows whose arg-max is
    masked, by less than a factor (d + D + K) / (d + K), would be this and not a defect.
    """
    _, _, d, e = _soft64(logits, C, mask)
    p = e / e.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, (d + K) * U * p, 0.0) + TINY


def decidable_rows(logits, C, mask=None):
    """bool [rows]: the float64 top-1 / top-2 gap exceeds the sum of the two allowances, so every float32 evaluation inside prob_bound
    has the same arg-max (a row with a single unmasked class is decidable)"""
    p, b = probs64(logits, C, mask), prob_bound(logits, C, mask)
    if C == 1:
        return np.ones(len(p), dtype=bool)
    order = np.argsort(-p, axis=1, kind="stable")[:, :2]
    r = np.arange(len(p))
    return (p[r, order[:, 0]] - p[r, order[:, 1]]) > (b[r, order[:, 0]] + b[r, order[:, 1]])


# ------------------------------------------------------------------------------------------------ exact restatements
def collapse(idx_seq):
    """CTCLabelConverter.decode_greedy: drop repeats, drop blank 0"""
    s = [int(v) for v in idx_seq]
    return [v for t, v in enumerate(s) if v != 0 and not (t > 0 and s[t - 1] == v)]


def cnt(idx_seq):
    """len(values[indices != 0]): the non-blank steps, repeats included"""
    return int(np.count_nonzero(np.asarray(idx_seq)))


def prod32(idx_seq, pmax_seq):
    """numpy's multiply.reduce over values[indices != 0] in float32: strictly sequential in time order, subnormals kept"""
    p = F(1.0)
    for i, v in zip(np.asarray(idx_seq), np.asarray(pmax_seq, dtype=np.float32)):
        if i != 0:
            p = F(p * v)
    return p


def conf(prod, n):
    """custom_mean: prod ** (2 / sqrt(n)); an all-blank sequence scores 0"""
    return float(prod) ** (2.0 / math.sqrt(n)) if n > 0 else 0.0


# ------------------------------------------------------------------------------------------------ checks (device outputs or a stand-in's)
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_probs(case, probs):
    """probs float32 [rows, cs] against float64 -> the worst |error| / allowance.  No element is exempt; masked classes are exactly +0;
    the columns behind C keep the caller's sentinel."""
    C = case.C
    want, bound = case.p64, case.bound
    got = probs[:, :C].astype(np.float64)
    ratio = np.abs(got - want) / bound
    bad = ~(ratio <= 1.0)                                       # a NaN is a failure
    if bad.any():
        r, c = np.unravel_index(np.argmax(np.nan_to_num(ratio, nan=np.inf)), ratio.shape)
        raise AssertionError(f"{case.name}: {int(bad.sum())} probabilities outside prob_bound; worst at row {r} class {c}: "
                             f"got {got[r, c]!r} want {want[r, c]!r} allowance {bound[r, c]!r}")
    gone = mask_bits(case.mask, C)
    assert (_bits(probs[:, :C][:, gone]) == 0).all(), f"{case.name}: a masked class is not exactly +0"
    assert (_bits(probs[:, C:]) == _bits(F(S_PROB))).all(), f"{case.name}: a column behind C was written"
    return float(ratio.max()) if ratio.size else 0.0


def check_exact(case, probs, idx, pmax, out_idx, ctc_out, decode=None):
    """everything behind the probabilities, from the device's own probs / idx / pmax: bit for bit.
    ctc_out: int32 [n, 4] rows {len, cnt, prod bits, pad}; decode(len, cnt, prod) -> production's confidence, if given."""
    C = case.C
    rows = len(case.logits)
    first = probs[:, :C].argmax(axis=1)                         # numpy: the first index among equals
    assert np.array_equal(idx, first), f"{case.name}: idx differs from the first-index arg-max of the device row at rows {np.nonzero(idx != first)[0][:8]}"
    own = probs[np.arange(rows), idx]
    assert np.array_equal(_bits(pmax), _bits(own)), f"{case.name}: pmax is not probs[row, idx[row]] at rows {np.nonzero(_bits(pmax) != _bits(own))[0][:8]}"
    written = np.zeros(rows, dtype=bool)
    for k, (r0, T) in enumerate(case.seqs):
        seq, pm = idx[r0:r0 + T], pmax[r0:r0 + T]
        text = collapse(seq)
        ln, cn, pb, pad = (int(v) for v in ctc_out[k])
        assert ln == len(text) and cn == cnt(seq) and pad == 0, f"{case.name} seq {k}: len / cnt / pad {ln} / {cn} / {pad}, want {len(text)} / {cnt(seq)} / 0"
        assert list(out_idx[r0:r0 + ln]) == text, f"{case.name} seq {k}: text {list(out_idx[r0:r0 + ln])} want {text}"
        want = prod32(seq, pm)
        assert pb == int(np.float32(want).view(np.int32)), f"{case.name} seq {k}: prod {np.array([pb], dtype=np.int32).view(np.float32)[0]!r} want {want!r} (sequential float32 product in time order)"
        if decode is not None:
            got, ref = decode(ln, cn, want), conf(want, cn)
            assert abs(got - ref) <= math.ulp(ref), f"{case.name} seq {k}: confidence {got!r} want {ref!r}"
        written[r0:r0 + ln] = True
    assert (out_idx[~written] == S_OUT).all(), f"{case.name}: out_idx written outside the first len entries of a sequence at rows {np.nonzero((out_idx != S_OUT) & ~written)[0][:8]}"
    assert (ctc_out[len(case.seqs):] == np.int32(S_CTC)).all(), f"{case.name}: ctc_out written behind the last sequence"
    if case.expect_idx is not None:
        sel = case.expect_idx >= 0
        assert np.array_equal(idx[sel], case.expect_idx[sel]), f"{case.name}: idx differs from the designed arg-max at rows {np.nonzero(sel & (idx != case.expect_idx))[0][:8]}"
    if case.expect_text is not None:
        for k, (r0, T) in enumerate(case.seqs):
            assert list(out_idx[r0:r0 + int(ctc_out[k][0])]) == case.expect_text[k], f"{case.name} seq {k}: text differs from the designed one"


def check_fp64(case, idx):
    """idx against the float64 arg-max on every decidable row -> the share of undecidable rows (the caller holds it under the cap)"""
    ok = case.decidable
    want = case.p64.argmax(axis=1)
    assert np.array_equal(idx[ok], want[ok]), f"{case.name}: idx differs from the float64 arg-max on decidable rows {np.nonzero(ok & (idx != want))[0][:8]}"
    return 1.0 - float(ok.mean())
