"""Plain numpy references of the CTC stage over MORE than 128 classes (ctc.hip::ctc_rows_wide_kernel, pred_ctc.hip::pred_ctc_kernel) and the
checks that test_gpu_wide_classes.py applies to the device's outputs and test_wide_classes_cpu.py to stand-ins with planted defects.

As in ctc_greedy_ref.py the stage is checked in two halves: the probabilities against a float64 softmax under a DERIVED allowance
(prob_bound, re-derived below for the wide kernel's summation order), and everything behind them -- arg-max, pmax, collapse, cnt, product,
confidence -- bit for bit as a function of the device's own probabilities (ctc_greedy_ref.check_exact, which is generic in C).

Masks are ceil(C / 32) 32-bit words (at least four), bit c & 31 of word c >> 5 removing class c, or None.  Nothing here needs a GPU.
"""
import math

import numpy as np

import ctc_greedy_ref as G
from ctc_greedy_ref import F, S_CTC, S_IDX, S_OUT, S_PROB, TINY, U, check_exact, collapse, cnt, conf, mask_bits, prod32, probs64  # noqa: F401

S_PMAX = -3.0                     # sentinel of a pmax tensor


def n_words(C):
    return max(4, (C + 31) // 32)


def mask_words(classes, C):
    w = [0] * n_words(C)
    for c in classes:
        assert 0 < c < C
        w[c >> 5] |= 1 << (c & 31)
    return tuple(w)


def k_wide(C):
    """The constant of prob_bound for a row of C classes.

    C <= 128 is ctc_rows_kernel's two-registers-per-lane reduction: ctc_greedy_ref.K = 19, derived there.  Beyond, ctc_rows_wide_kernel walks
    the row 64 classes at a time: each lane adds its n = ceil(C / 64) terms in ascending class order (n - 1 roundings), then the 6-step
    butterfly (6 roundings): n + 5 roundings of positive terms per sum, where the narrow kernel has 1 + 6 = 7.  Following that file's steps
    with u = 2^-24, d_j = max - x_j:
      1.-2. e_j = E_j (1 + eta_j), |eta_j| <= (d_j + 2) u                     [fl(x_j - max), expf to 1 ulp = 2u]: unchanged
      3.    S, the sum of the e_j: the same float in every lane; it cancels in step 6 exactly as there -- its n + 5 roundings reach nothing
      4.    q_j = fl(e_j / S): u
      5.    norm, the sum of the unmasked q_j: inherits the p-weighted mean of its terms' errors, sum_k p_k (d_k + 3) u, and
            sum_k p_k d_k <= ln C (entropy bound, as there -- but ln C is no longer below ln 128); plus its own n + 5 roundings
      6.    q'_j = fl(q_j / norm): u
    Sum for element j:  (d_j + 2) + 1  +  (ln C + 3) + (n + 5)  +  1   =   d_j + ceil(C / 64) + ln C + 12.
    K(C) = ceil(C / 64) + ln C + 12.14: the 0.14 is the slack that file leaves for second-order terms (at C = 128: 2 + 4.86 + 12.14 = 19,
    its constant).  352 classes: 24.0; 1,009: 35.1; 6,719: 125.9 -- the walk's 105 sequential additions per lane dominate there.
    """
    if C <= 128:
        return G.K
    return -(-C // 64) + math.log(C) + 12.14


def prob_bound(logits, C, mask=None):
    """per-element allowance of a float32 evaluation of probs64 in the wide kernel's order: (|x - max| + K(C)) 2^-24 p + 2^-126.
    The remarks of ctc_greedy_ref.prob_bound on rows whose arg-max is masked apply unchanged."""
    _, _, d, e = G._soft64(logits, C, mask)
    p = e / e.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, (d + k_wide(C)) * U * p, 0.0) + TINY


# ------------------------------------------------------------------------------------------------ logits (the unfused Prediction launch)
def logit_bound(ref64):
    """tests/stage_ref.py's rule for an fp32-output GEMM with K = 256 against the float64 product of the ROUNDED operands:
    |got - ref| <= 2 acc + 2^-24, acc = 2e-5 max(1, max |ref|)"""
    return 2.0 * 2e-5 * max(1.0, float(np.abs(ref64).max())) + 2.0 ** -24


def logits64(x, w, b):
    """float64 logits of rounded operands: x [rows, 256], w [C, 256], b [C] (float arrays holding element-type values)"""
    return x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the fused kernel
def fused_ref(l64, C, mask=None):
    """what pred_ctc_kernel states, in float64 from float64 logits -> (idx, pmax, margin): idx = the unmasked class of the largest logit
    (lowest index among equals), pmax = its probability renormalised over the unmasked classes, margin = top-1 minus top-2 logit among the
    unmasked classes (inf with a single one)"""
    x = np.asarray(l64, dtype=np.float64)[:, :C]
    gone = mask_bits(mask, C)
    xm = np.where(gone[None, :], -np.inf, x)
    idx = xm.argmax(axis=1)
    top = xm.max(axis=1)
    if C - int(gone.sum()) > 1:
        second = np.partition(xm, C - 2, axis=1)[:, C - 2]
        margin = top - second
    else:
        margin = np.full(len(x), np.inf)
    e = np.exp(xm - x.max(axis=1, keepdims=True))
    pmax = e[np.arange(len(x)), idx] / e.sum(axis=1)
    return idx, pmax, margin


def check_fused(name, l64, C, mask, idx, pmax, L, expect_idx=None):
    """idx / pmax of the fused kernel against fused_ref of the float64 logits l64 whose device counterparts lie within L (logit_bound).

    expect_idx: per row the class a DESIGNED row must give (tie rows, whose margin of 0 exempts them below), or -1.
    idx: on every row whose margin exceeds 2 L the two candidates cannot swap (each logit moves by at most L), so idx must be the float64
    arg-max; the other rows are left out and their share is returned for the caller to hold under its cap.
    pmax: propagation of the logit bound through the softmax -- p_j = exp(x_j) / sum_k exp(x_k); with every x moved by at most L the
    numerator changes by a factor within exp(+-L) and the denominator, a sum of positive terms each within exp(+-L), by a factor within
    exp(-+L): relative change exp(2 L) - 1 = 2 L to first order (L is 1e-4: the next term is 1e-8 relative, inside prob_bound's slack),
    taken as 2 L.  On top comes the float32 evaluation of
    the softmax itself, prob_bound at the winning class.  For pred_ctc_kernel this second term is EMPIRICAL, not derived: K(C) counts
    the roundings of ctc_rows_wide_kernel, whereas the fused kernel adds up to 4 ceil(C / 64) terms per lane, multiplies both running sums
    by expf(old - new) whenever a lane's maximum grows (at most once per four-class group) and merges partial sums on three levels (two xor
    steps, the four waves); a worst-case count of those roundings is about four times K(C) and is not what is asserted.  The issue sets
    prob_bound as this check's allowance; the device's pmax has met it on every row of every case so far, and a miss by less than that
    factor of four on a row far from any margin would be this gap and not a defect."""
    want_idx, want_p, margin = fused_ref(l64, C, mask)
    if expect_idx is not None:          # designed rows (bitwise equal logits: the lowest class must win), -1 elsewhere
        sel = np.asarray(expect_idx) >= 0
        assert np.array_equal(np.asarray(idx)[sel], np.asarray(expect_idx)[sel]), f"{name}: idx differs from the designed class on rows {np.nonzero(sel & (np.asarray(idx) != expect_idx))[0][:8]}"
    ok = margin > 2.0 * L
    bad = ok & (np.asarray(idx) != want_idx)
    assert not bad.any(), f"{name}: idx differs from the float64 arg-max on rows {np.nonzero(bad)[0][:8]} (got {np.asarray(idx)[bad][:8]}, want {want_idx[bad][:8]})"
    pb = prob_bound(l64, C, mask)[np.arange(len(want_p)), want_idx]
    tol = 2.0 * L * want_p + pb
    err = np.abs(np.asarray(pmax, dtype=np.float64) - want_p)
    worst = ok & ~(err <= tol)
    assert not worst.any(), (f"{name}: pmax outside the propagated bound on rows {np.nonzero(worst)[0][:8]}: got {np.asarray(pmax)[worst][:4]} "
                             f"want {want_p[worst][:4]} allowance {tol[worst][:4]}")
    return 1.0 - float(ok.mean())


def check_probs(name, logits, C, mask, probs, sentinel=S_PROB):
    """probs float32 [rows, cs] of the wide rows kernel against float64 -> worst |error| / allowance.  No element is exempt; masked classes
    are exactly +0; the columns behind C keep the caller's sentinel (they are neither read nor written)."""
    want, bound = probs64(logits, C, mask), prob_bound(logits, C, mask)
    got = probs[:, :C].astype(np.float64)
    ratio = np.abs(got - want) / bound
    bad = ~(ratio <= 1.0)
    if bad.any():
        r, c = np.unravel_index(np.argmax(np.nan_to_num(ratio, nan=np.inf)), ratio.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} probabilities outside prob_bound; worst at row {r} class {c}: got {got[r, c]!r} "
                             f"want {want[r, c]!r} allowance {bound[r, c]!r}")
    gone = mask_bits(mask, C)
    assert (G._bits(probs[:, :C][:, gone]) == 0).all(), f"{name}: a masked class is not exactly +0"
    assert (G._bits(probs[:, C:]) == G._bits(F(sentinel))).all(), f"{name}: a column behind C was written"
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------ stand-ins (float32 numpy; planted defects)
def rows_standin(logits, C, mask=None, defect=None, sentinel=S_PROB):
    """ctc_rows_wide_kernel restated in float32 numpy -> (probs [rows, cs], idx, pmax).  defect: None, or one of
    'tie_high' (the highest index wins a tie), 'padded' (columns >= C take part), ('drop_bit', c) (mask bit c is ignored),
    'sum_masked' (the second sum runs over the masked classes too), 'last_tile' (the maximum misses the last 64-class step)."""
    x = np.asarray(logits, dtype=np.float32)
    rows, cs = x.shape
    n = cs if defect == "padded" else C
    gone = np.zeros(n, dtype=bool)
    gone[:C] = mask_bits(mask, C)
    if isinstance(defect, tuple) and defect[0] == "drop_bit":
        gone[defect[1]] = False
    v = x[:, :n]
    mcols = (n - 1) // 64 * 64 if defect == "last_tile" and n > 64 else n
    m = v[:, :mcols].max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):            # (a planted defect may overflow: that is how it shows)
        e = np.exp((v - m).astype(np.float32)).astype(np.float32)
        q = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
        qm = np.where(gone[None, :], F(0), q)
        norm = (q if defect == "sum_masked" else qm).sum(axis=1, keepdims=True, dtype=np.float32)
        p = (qm / norm).astype(np.float32)
    probs = np.full((rows, cs), sentinel, dtype=np.float32)
    probs[:, :n] = p
    if defect == "tie_high":
        idx = n - 1 - p[:, ::-1].argmax(axis=1)
    else:
        idx = p.argmax(axis=1)
    return probs, idx.astype(np.int32), p[np.arange(rows), idx]


def fused_standin(l32, C, mask=None, defect=None):
    """pred_ctc_kernel's result restated in numpy from float32 logits [rows, cs] -> (idx, pmax); defects as in rows_standin"""
    x = np.asarray(l32, dtype=np.float32).astype(np.float64)
    n = x.shape[1] if defect == "padded" else C
    gone = np.zeros(n, dtype=bool)
    gone[:C] = mask_bits(mask, C)
    if isinstance(defect, tuple) and defect[0] == "drop_bit":
        gone[defect[1]] = False
    v = x[:, :n]
    vm = np.where(gone[None, :], -np.inf, v)
    if defect == "last_tile" and n > 16:
        vm = vm.copy()
        vm[:, (n - 1) // 16 * 16:] = -np.inf          # the arg-max never sees the last 16-class fragment
    idx = n - 1 - vm[:, ::-1].argmax(axis=1) if defect == "tie_high" else vm.argmax(axis=1)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    s_un = e.sum(axis=1) if defect == "sum_masked" else np.where(gone[None, :], 0.0, e).sum(axis=1)
    pmax = e[np.arange(len(v)), idx] / s_un
    return idx.astype(np.int32), pmax.astype(np.float32)
