"""CPU: the references, the case table and the check functions of the greedy CTC stage, before any of them judges a kernel
(test_gpu_ctc_greedy.py).

* the float64 restatement decodes what oracle.recog.predict_from_logits decodes, on every case the oracle can express;
* the decidability caps hold for the reference alone;
* torch's float32 softmax, a correct float32 implementation with another summation order and another exp, stays inside prob_bound;
* each planted defect is rejected, on a named case, by the check functions the GPU test applies to the device's outputs;
* the reference's invariants hold over random C / cs / T / masks.
"""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as hs

import ctc_greedy_cases as K
import ctc_greedy_ref as R

F = np.float32


def embed(case, probs_c):
    out = np.full((len(case.logits), case.cs), R.S_PROB, dtype=np.float32)
    out[:, :case.C] = probs_c
    return out


# ------------------------------------------------------------------------------------------------ the restatement is the oracle's decode
def test_restatement_decodes_what_the_oracle_decodes():
    """probs64 + first-index arg-max + collapse against recognizer_predict's tail as the oracle restates it (float32 torch softmax, numpy
    mask / renormalisation / arg-max, decode_greedy), on every uniform case of at most 97 classes (the oracle's character table): the
    text is identical on every decidable sequence -- and on the tie cases too, where both take the first index."""
    from oracle import recog

    seen = 0
    for case in K.CASES:
        u = case.uniform()
        if u is None or case.C > recog.NUM_CLASS:
            continue
        n, T = u
        gone = [int(c) for c in np.nonzero(R.mask_bits(case.mask, case.C))[0]]
        ref = recog.predict_from_logits(case.logits[:, :case.C].reshape(n, T, case.C), ignore_idx=gone)
        idx = case.p64.argmax(axis=1)
        for k, (r0, t) in enumerate(case.seqs):
            if not (case.decidable[r0:r0 + t].all() or case.tie):
                continue
            text = "".join(recog.CHARACTER[v] for v in R.collapse(idx[r0:r0 + t]))
            assert text == ref[k][0], (case.name, k)
            pm = case.p64[np.arange(r0, r0 + t), idx[r0:r0 + t]].astype(np.float32)
            want = float(ref[k][1])
            assert R.conf(R.prod32(idx[r0:r0 + t], pm), R.cnt(idx[r0:r0 + t])) == pytest.approx(want, rel=1e-4, abs=1e-30), (case.name, k)
            seen += 1
    assert seen >= 60


def test_decidability_caps_hold_for_the_reference_alone():
    """at most 1 % of the random cases' sequences hold an undecidable step (with these seeds: none), no designed case does"""
    bad, tot = K.assert_caps()
    print(f"undecidable sequences over the random cases: {bad} of {tot}")


def test_case_table_covers_what_it_claims():
    names = set(K.BY_NAME)
    for C in K.WIDTHS:
        for s in K.STRIDES:
            cs = C if s == "C" else s
            assert cs < C or f"width/C{C}-cs{cs}" in names
    for case in (K.BY_NAME["ragged/C97"], K.BY_NAME["ragged/C128"]):
        assert sorted(int(T) for _, T in case.seqs) == sorted(K.RAGGED_T)
        assert [int(r0) for r0, _ in case.seqs] != sorted(int(r0) for r0, _ in case.seqs)             # table order is not row order
        used = np.zeros(len(case.logits), dtype=bool)
        for r0, T in case.seqs:
            assert not used[r0:r0 + T].any()
            used[r0:r0 + T] = True
        assert not used.all()                                                                        # rows that belong to no sequence
    for case in K.CASES:
        assert np.isnan(case.logits[:, case.C::2]).all() and (case.logits[:, case.C + 1::2] == np.inf).all(), case.name
    # the product cases do what their docstring says, in the reference's own float32 product
    for name, end in (("prod/underflow_639", "zero"), ("prod/subnormal_70", "subnormal")):
        case = K.BY_NAME[name]
        pm = case.p64[:, 1].astype(np.float32)
        assert (abs(pm - 0.25) < 0.002).all()
        run = np.array([R.prod32([1] * t, pm[:t]) for t in range(1, len(pm) + 1)])
        assert ((run > 0) & (run < R.TINY)).any()
        assert run[-1] == 0 if end == "zero" else 0 < run[-1] < R.TINY
    assert len(K.BY_NAME["sweep/33100_rows"].logits) > 8192 * 4 and max(int(T) for _, T in K.BY_NAME["sweep/33100_rows"].seqs) > 8192 * 4
    # the real character lists are the reader's own masks
    from bb_ocr_amd.reader import ignore_mask
    from oracle import recog

    assert tuple(ignore_mask(recog.CHARACTER, list(recog.CHARSET), allowlist="0123456789")) == K.BY_NAME["mask/allow_digits"].mask
    assert tuple(ignore_mask(recog.CHARACTER, list(recog.CHARSET), blocklist="aeiouAEIOU -")) == K.BY_NAME["mask/block_vowels"].mask


# ------------------------------------------------------------------------------------------------ the allowance is not too tight
def torch_probs32(case):
    """recognizer_predict in float32: F.softmax, masked classes zeroed, division by the remaining sum"""
    p = torch.softmax(torch.from_numpy(np.ascontiguousarray(case.logits[:, :case.C])), dim=-1).numpy()
    p[:, R.mask_bits(case.mask, case.C)] = 0.0
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def test_torch_float32_softmax_stays_inside_prob_bound():
    """torch's float32 softmax (vectorised exp, its own summation order) + numpy's float32 renormalisation against probs64 on every case:
    inside prob_bound everywhere, so the derived allowance is not too tight for a correct float32 implementation.  Worst observed
    |error| / allowance: 0.779 (range/spread_80, an element 65.3 below its row's maximum; 0.66 on the sigma-4 cases at 32.2 below).  It
    is that close because the |x - max| term is sharp: just above a power of two the rounding of x - max alone is worth (|x - max|) u."""
    worst, where = 0.0, None
    for case in K.CASES:
        r = R.check_probs(case, embed(case, torch_probs32(case)))
        if r > worst:
            worst, where = r, case.name
    print(f"torch float32 softmax: worst |error| / prob_bound = {worst:.3f} on {where}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ planted defects
def _tree(v):
    if len(v) == 0:
        return F(1.0)
    if len(v) == 1:
        return F(v[0])
    return F(_tree(v[:len(v) // 2]) * _tree(v[len(v) // 2:]))


def standin(case, defect=None):
    """the stage in numpy as the restatement defines it (probabilities: float64 rounded once to float32) -> (probs, idx, pmax, out_idx,
    ctc_out) as the device leaves them, sentinels included; `defect` plants one mistake"""
    C, rows = case.C, len(case.logits)
    ncol = min(case.cs, 64) if defect == "reads_poison" and C < 64 else C
    mask = case.mask
    if defect == "swap_yz" and mask is not None:
        mask = (mask[0], mask[2], mask[1], mask[3])
    with np.errstate(all="ignore"):
        if defect == "no_renorm":
            p = R.probs64(case.logits, ncol, None)
            p[:, R.mask_bits(mask, ncol)] = 0.0
        else:
            p = R.probs64(case.logits, ncol, mask)
    probs = embed(case, p[:, :C].astype(np.float32))
    pc = probs[:, :C]
    idx = (C - 1 - pc[:, ::-1].argmax(axis=1)) if defect == "last_tie" else pc.argmax(axis=1)
    idx = idx.astype(np.int32)
    pmax = pc[np.arange(rows), idx]
    out_idx = np.full(rows, R.S_OUT, dtype=np.int32)
    ctc_out = np.full((len(case.seqs) + 2, 4), R.S_CTC, dtype=np.int32)
    for k, (r0, T) in enumerate(case.seqs):
        s, pm = idx[r0:r0 + T], pmax[r0:r0 + T]
        keep = [t for t in range(T) if s[t] != 0 and (t == 0 or s[t] != s[t - 1] or (defect == "prev_reset_64" and t % 64 == 0))]
        nb = [t for t in range(T) if s[t] != 0]
        if defect == "prod_kept":
            prod = R.prod32(s[keep], pm[keep])
        elif defect == "tree_prod":
            prod = _tree(pm[nb])
        elif defect == "flush":
            prod = F(1.0)
            for t in nb:
                prod = F(prod * pm[t])
                if abs(prod) < R.TINY:
                    prod = F(0.0)
        else:
            prod = R.prod32(s, pm)
        out_idx[r0:r0 + len(keep)] = s[keep]
        ctc_out[k] = [len(keep), len(keep) if defect == "cnt_len" else len(nb), int(np.float32(prod).view(np.int32)), 0]
    return probs, idx, pmax, out_idx, ctc_out


def judge(case, outs):
    """what the GPU test does with the device's outputs"""
    probs, idx, pmax, out_idx, ctc_out = outs
    R.check_probs(case, probs)
    R.check_exact(case, probs, idx, pmax, out_idx, ctc_out)
    R.check_fp64(case, idx)


def test_checks_accept_the_restatement():
    for case in K.CASES:
        judge(case, standin(case))


DEFECTS = [("last_tie", "tie/3_67"), ("last_tie", "tie/5_6"), ("last_tie", "tie/63_64"), ("last_tie", "tie/constant_row"),
           ("prev_reset_64", "collapse/repeat_across_63_64"), ("prev_reset_64", "collapse/repeat_across_127_128"),
           ("prod_kept", "prod/subnormal_70"), ("tree_prod", "ragged/C97"), ("cnt_len", "collapse/one_char_129"),
           ("swap_yz", "mask/bit32"), ("swap_yz", "mask/bit64"), ("swap_yz", "mask/only_blank_and_63"), ("no_renorm", "mask/removes_argmax"),
           ("flush", "prod/subnormal_70"), ("reads_poison", "width/C37-cs112"), ("reads_poison", "width/C63-cs131"), ("reads_poison", "width/C1-cs112")]


@pytest.mark.parametrize("defect,name", DEFECTS, ids=[f"{d}-{n}" for d, n in DEFECTS])
def test_planted_defect_is_rejected(defect, name):
    """last index wins a tie; prev = -1 whenever t % 64 == 0; product over the kept characters only; pairwise product; cnt = len; mask
    words y and z swapped; mask without renormalisation; subnormals flushed in the product; columns >= C read when C < 64"""
    case = K.BY_NAME[name]
    with pytest.raises(AssertionError):
        judge(case, standin(case, defect))


# ------------------------------------------------------------------------------------------------ invariants of the reference
@settings(max_examples=60, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(C=hs.integers(1, 128), extra=hs.sampled_from([0, 1, 15, 31]), T=hs.integers(0, 140), seed=hs.integers(0, 2 ** 31), masked=hs.floats(0.0, 0.9),
       sigma=hs.sampled_from([0.5, 2.0, 4.0]))
def test_reference_invariants(C, extra, T, seed, masked, sigma):
    rng = np.random.default_rng(seed)
    lg = np.full((T, C + extra), np.nan, dtype=np.float32)
    lg[:, :C] = rng.standard_normal((T, C)) * sigma
    gone = [c for c in range(C) if rng.random() < masked][:C - 1]                  # at least one class stays
    mask = R.mask_words(gone) if gone else None
    p = R.probs64(lg, C, mask)
    assert p.shape == (T, C) and (p[:, R.mask_bits(mask, C)] == 0).all()
    assert np.allclose(p[:, ~R.mask_bits(mask, C)].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    idx = p.argmax(axis=1) if T else np.zeros(0, dtype=np.int64)
    assert not set(idx) & set(gone)
    text = R.collapse(idx)
    assert len(text) <= R.cnt(idx) <= T
    assert all(a != b for a, b in zip(text, text[1:])) or 0 in idx                # equal neighbours only across a blank
    pm = p[np.arange(T), idx].astype(np.float32)
    assert 0.0 <= R.conf(R.prod32(idx, pm), R.cnt(idx)) <= 1.0
