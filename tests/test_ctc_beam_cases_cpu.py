"""The inputs of test_gpu_ctc_beam.py can fail: each family of tests/ctc_beam_cases.py is run through bbocr_host_ctc_beam (the yardstick)
and through a float32 Python restatement of the search, and must show the property it was built for -- labellings that leave the beam and
come back, bit-equal totals at the cut, totals that underflow to 0, steps at which every class is a candidate.  No GPU."""
import numpy as np
import pytest

import ctc_beam_cases as cases


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def test_width_limit_is_the_headers():
    import os
    import re

    from bb_ocr_amd import _lib

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbocr.h")).read()
    assert int(re.search(r"#define BBOCR_BEAM_DEVICE_MAX (\d+)", hdr).group(1)) == _lib.BEAM_DEVICE_MAX == cases.BEAM_DEVICE_MAX
    assert "bbocr_op_ctc_beam" in _lib.PROTOTYPES and "bbocr_op_ctc_probs" in _lib.PROTOTYPES


def test_small_alphabet_family_tells_parent_pointers_from_equality(lib):
    cs = cases.small_alphabet_cases()
    assert 1900 <= len(cs) <= 2100
    assert {r.shape[1] for r, _ in cs} == {3, 4, 5} and {r.shape[0] for r, _ in cs} == set(range(4, 14)) and {w for _, w in cs} == {1, 2, 3}
    host = cases.host_texts(lib, cs)
    assert [cases.beam_search_py(r, w) for r, w in cs] == host                     # the restatement is the host's search
    wrong = sum(cases.beam_search_py(r, w, parent_pointer=True) != h for (r, w), h in zip(cs, host))
    print("parent-pointer merging differs on", wrong, "of", len(cs))
    assert wrong >= 0.05 * len(cs)
    assert any(cases.greedy_collapse(r) != h for (r, _), h in zip(cs, host))


def test_tie_family_has_bit_equal_totals_at_the_cut(lib):
    cs = cases.tie_cases()
    assert [cases.beam_search_py(r, w) for r, w in cs] == cases.host_texts(lib, cs)
    tied = 0
    for rows, w in cs:
        assert (rows[1:] == rows[:-1]).all() or rows.shape[1] == 97                # repeated rows
        trace = []
        cases.beam_search_py(rows, w, trace=trace)
        top = [x[:w + 1] for x in trace if len(x) > 1]
        tied += any((x[1:].view(np.uint32) == x[:-1].view(np.uint32)).any() for x in top)
    assert tied >= 0.9 * len(cs)


def test_underflow_family_reaches_subnormals_and_zero(lib):
    rows = cases.underflow_rows()
    assert rows.shape == (639, 97) and (rows >= np.float32(0.5 / 97)).all()
    trace = []
    assert cases.beam_search_py(rows, 5, trace=trace) == cases.host_texts(lib, [(rows, 5)])[0]
    tiny = np.finfo(np.float32).tiny
    sub = [t for t, x in enumerate(trace) if ((x[:6] > 0) & (x[:6] < tiny)).any()]
    zero = [t for t, x in enumerate(trace) if (x == 0).all()]
    assert sub and zero and sub[0] < zero[0] < 600                                  # through the subnormal range, then 0 long before the end
    assert all((x == 0).all() for x in trace[zero[0]:])
    assert {w for _, w in cases.underflow_cases()} == {1, 5, cases.BEAM_DEVICE_MAX}


def test_saturation_family_has_every_class_as_a_candidate(lib):
    cs = cases.saturation_cases()
    assert {w for _, w in cs} == {1, 5, cases.BEAM_DEVICE_MAX}
    for rows, _ in cs:
        assert rows.shape[1] == 97 and (rows >= np.float32(0.5 / 97)).all()
    assert any((r == np.float32(1) / np.float32(97)).all() for r, _ in cs)
    assert [cases.beam_search_py(r, w) for r, w in cs] == cases.host_texts(lib, cs)


def test_peaked_and_ragged_inputs(lib):
    cs = cases.peaked_cases()
    assert [cases.beam_search_py(r, w) for r, w in cs] == cases.host_texts(lib, cs)
    assert {r.shape[0] for r, _ in cs} >= {1, 63, 64, 65}
    pool, seqs = cases.ragged_table()
    T = seqs[:, 1]
    assert len(seqs) >= 300 and T.min() == 0 and T.max() == 639 and T[T > 0].min() == 1 and (np.diff(T) < 0).any() and (np.diff(T) > 0).any()
    assert seqs[0, 0] == 0 and (seqs[1:, 0] == np.cumsum(T)[:-1]).all() and T.sum() == len(pool)
