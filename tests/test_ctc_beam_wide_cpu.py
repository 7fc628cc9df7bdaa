"""No GPU: the inputs of the wide-class device beam search (tests/ctc_beam_wide_cases.py) aim where they claim to.  The Python restatement
equals bbocr_host_ctc_beam (the yardstick of test_gpu_ctc_beam_wide.py) on every case, each wrong restatement a device search over more
than 128 classes invites changes the text of cases of the family built against it, the crowded rows hold exactly the candidates they are
named for, and the routing rule and bbocr_create_v2's check of bbocr_config_v2::beam_wide answer without a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import ctc_beam_wide_cases as W

CLASSES = W.CLASSES


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


@functools.lru_cache(maxsize=None)
def families(Cn):
    return W.families(Cn)


@functools.lru_cache(maxsize=None)
def reference(Cn, name):
    """search_py on one family: computed once, shared by the tests below"""
    return [W.search_py(r, w) for r, w in families(Cn)[name]]


def changed(Cn, name, wrong):
    cs = families(Cn)[name]
    got = [W.beam_search_py(r, w, parent_pointer=True) if wrong == "parent_pointer" else W.search_py(r, w, wrong) for r, w in cs]
    return [i for i, (g, m) in enumerate(zip(got, reference(Cn, name))) if g != m]


@pytest.mark.parametrize("Cn", CLASSES)
def test_python_search_equals_the_host_search(lib, Cn):
    for name, cs in families(Cn).items():
        assert reference(Cn, name) == [W.beam_search_py(r, w) for r, w in cs], name        # two restatements, one answer
        assert W.host_texts(lib, cs, W.cs_of(Cn)) == reference(Cn, name), name
    ov = [(r, w) for r, w, _ in W.overflow_cases(Cn)]
    assert W.host_texts(lib, ov, W.cs_of(Cn)) == [W.search_py(r, w) for r, w in ov]
    pool, seqs = W.ragged_table(Cn)
    rg = [(pool[a:a + T], 5) for a, T in seqs]
    assert W.host_texts(lib, rg, W.cs_of(Cn)) == [W.search_py(r, w) if len(r) else [] for r, w in rg]


def test_too_long_sequence(lib):
    rows = W.too_long_rows()
    assert rows.shape[0] > W.max_T(W.BEAM_DEVICE_MAX) and rows.shape[0] <= W.max_T(5) and not W.overflows(rows)
    assert W.host_texts(lib, [(rows, 5)], W.cs_of(rows.shape[1])) == [W.search_py(rows, 5)]


@pytest.mark.parametrize("Cn", CLASSES)
def test_scattered_alphabets_defeat_parent_pointers(Cn):
    bad = changed(Cn, "scattered", "parent_pointer")
    print(f"C={Cn}: parent-pointer merging changes {len(bad)} of {len(families(Cn)['scattered'])} scattered cases")
    assert len(bad) >= 3


@pytest.mark.parametrize("Cn", [c for c in CLASSES if c > 767])
def test_aliases_defeat_8_bit_symbols(Cn):
    bad = changed(Cn, "aliases", "sym8")
    print(f"C={Cn}: 8-bit symbols change {len(bad)} of {len(families(Cn)['aliases'])} alias cases")
    assert len(bad) >= len(families(Cn)["aliases"]) // 2
    # and every alias set is among the changed cases: high-byte twins (1 / 257), the shifted pair (1 / 256), the blank's twin (256)
    assert {i % len(W.ALIAS_SETS) for i in bad} == set(range(len(W.ALIAS_SETS)))
    assert changed(Cn, "scattered", "sym8") and changed(Cn, "ties", "sym8") and changed(Cn, "trained", "sym8")


@pytest.mark.parametrize("Cn", CLASSES)
def test_subthreshold_cases_defeat_candidate_only_reads(Cn):
    """EVERY case of width >= 3 (blank mirror: >= 2) changes; the narrow control does not; the texts are the constructed ones"""
    pairs = [(B, A) for B, A in W.SUB_PAIRS(Cn) if A < Cn]
    assert len(pairs) == (4 if Cn > 256 else 3)
    cs, ref = families(Cn)["subthreshold"], reference(Cn, "subthreshold")
    bad = set(changed(Cn, "subthreshold", "cand_only"))
    assert bad == {i for i, (_, w) in enumerate(cs) if w >= 3} and len(bad) == 3 * len(pairs)
    for i, (rows, w) in enumerate(cs):
        B, A = pairs[i // len(W.SUB_WIDTHS)]
        D = int(rows[1].argmax())
        assert ref[i] == ([A, D] if w >= 3 else [B, D]), (i, w, ref[i])
        assert W.search_py(rows, w, "cand_only") == [B, D]
        assert 0 < rows[1, A] < W.threshold(Cn) and W.n_candidates(rows).tolist() == [2, 1, 2]
    cs, ref = families(Cn)["subthreshold_blank"], reference(Cn, "subthreshold_blank")
    bad = set(changed(Cn, "subthreshold_blank", "cand_only"))
    assert bad == {i for i, (_, w) in enumerate(cs) if w >= 2} and len(bad) == 4 * len(pairs)
    for i, (rows, w) in enumerate(cs):
        B, A = pairs[i // (1 + len(W.SUB_WIDTHS))]
        assert ref[i] == ([A] if w >= 2 else [B, A]) and 0 < rows[1, 0] < W.threshold(Cn)


@pytest.mark.parametrize("Cn", CLASSES)
def test_crowded_rows_hold_the_candidates_they_are_named_for(Cn):
    for n in (W.K - 1, W.K, W.K + 1):
        row = W.crowded_row(Cn, n)
        assert row.dtype == np.float32 and int(W.n_candidates(row[None])[0]) == n
        assert int(np.nonzero(row >= W.threshold(Cn))[0][-1]) == Cn - 1 == int(row.argmax())       # the winner is the LAST candidate
    assert int(W.n_candidates(W.k_row()[None])[0]) == W.K and W.k_row().shape == (129,)
    ov = W.overflow_cases(Cn)
    assert [W.overflows(r) for r, _, _ in ov] == [o for _, _, o in ov]
    assert 0 < sum(o for _, _, o in ov) < len(ov)                                      # one table: sequences that overflow beside ones that do not
    assert {int(np.argmax(W.n_candidates(r) > W.K)) for r, _, o in ov if o} >= {0, 2, 4}        # first, middle and last step


@pytest.mark.parametrize("Cn", CLASSES)
def test_overflow_cases_defeat_a_truncated_list(Cn):
    ov = W.overflow_cases(Cn)
    for rows, w, over in ov:
        cut, full = W.search_py(rows, w, "truncate"), W.search_py(rows, w)
        crowded = int(np.argmax(W.n_candidates(rows) > W.K)) if over else -1
        if over and rows[crowded].max() == 0.5:
            assert cut != full and Cn - 1 in full and Cn - 1 not in cut                # the cut list lost the step's winner
        elif not over:
            assert cut == full


@pytest.mark.parametrize("Cn", CLASSES)
def test_trained_like_rows_stay_within_the_candidate_list(Cn):
    cs = families(Cn)["trained"]
    assert sorted({r.shape[0] for r, _ in cs}) == list(W.TRAINED_T) and sorted({w for _, w in cs}) == list(W.TRAINED_W)
    most = max(int(W.n_candidates(r).max()) for r, _ in cs)
    pool, seqs = W.ragged_table(Cn)
    print(f"C={Cn}: at most {most} candidates per trained-like row, {int(W.n_candidates(pool).max())} in the ragged table")
    assert most <= W.K and int(W.n_candidates(pool).max()) <= W.K and 1 < most
    assert len(seqs) >= 60 and (seqs[:, 1] == 0).sum() == 2 and (seqs[:, 1] == 1).any() and int(seqs[:, 1].sum()) == len(pool)
    assert any(W.search_py(r, w) != W.search_py(r, 1) for r, w in cs if w > 1)          # the width matters on these rows


def _route(lib, beam_wide, w, Cn, Ts):
    tab = (C.c_int * (2 * len(Ts)))(*[v for i, T in enumerate(Ts) for v in (sum(Ts[:i]), T)])
    return lib.bbocr_host_ctc_route(beam_wide, w, Cn, tab, len(Ts))


def test_routing_rule(lib):
    """ctc_route without a device: 4 (CTC_BEAM_DEVICE_WIDE) for 129 .. 8192 classes with the option on, widths 1 .. 32 and sequences that fit
    the LDS block; everything else is what it was"""
    from bb_ocr_amd import _lib

    assert W.BEAM_DEVICE_MAX == _lib.BEAM_DEVICE_MAX and _lib.REC_CLASSES_MAX == 8192
    for Cn in (129, 130, 352, 1009, 6719, 8192):
        for w in (1, 5, W.BEAM_DEVICE_MAX):
            assert _route(lib, 1, w, Cn, [3, 0, 160]) == 4, (Cn, w)
            assert _route(lib, 0, w, Cn, [3, 0, 160]) == 1, (Cn, w)                   # option off: the host, as before
            assert _route(lib, 1, w, Cn, [3, W.max_T(w)]) == 4 and _route(lib, 1, w, Cn, [W.max_T(w) + 1, 3]) == 1
        assert _route(lib, 1, W.BEAM_DEVICE_MAX + 1, Cn, [3, 160]) == 1               # width 33
        assert _route(lib, 1, 0, Cn, [3, 160]) == 0 and _route(lib, 0, 0, Cn, [3, 160]) == 0          # greedy stays greedy (no fused weights here)
    assert W.max_T(W.BEAM_DEVICE_MAX) == 356 and W.max_T(5) == 3076                   # the bounds include/bbocr.h states
    for Cn in (2, 97, 128):                                                            # at most 128 classes: the option changes nothing
        for flag in (0, 1):
            assert _route(lib, flag, 5, Cn, [3, 160]) == 2 and _route(lib, flag, W.BEAM_DEVICE_MAX + 1, Cn, [3, 160]) == 1
    assert _route(lib, 1, 5, 8193, [3]) == 1                                           # (no context is that wide; the rule does not reach past the maximum)
    assert lib.bbocr_host_ctc_route(1, 5, 1009, None, 2) == -1


def test_create_checks_beam_wide(lib):
    """refused before anything touches a device, like a bad class count (test_wide_classes_cpu.py); 0 and 1 pass that check and fail, on a
    machine without a device, with the device's error"""
    from bb_ocr_amd import _lib

    # the field is appended behind rec_classes in bbocr_config_v2; bbocr_config and bbocr_create keep their 32 bytes
    assert [f[0] for f in _lib.bbocr_config_v2._fields_][-2:] == ["rec_classes", "beam_wide"] and C.sizeof(_lib.bbocr_config_v2) == 36
    assert _lib.bbocr_config_v2._fields_[:-1] == _lib.bbocr_config._fields_ and C.sizeof(_lib.bbocr_config) == 32
    assert _lib.bbocr_config_v2.beam_wide.offset == 32 and _lib.bbocr_config_v2.rec_classes.offset == _lib.bbocr_config.rec_classes.offset
    for kw in ({"beam_wide": 2}, {"beam_wide": -1}, {"beam_wide": 7, "rec_classes": 6719}, {"beam_wide": 256, "rec_classes": 97}):
        h = C.c_void_p()
        assert lib.bbocr_create_v2(C.byref(_lib.bbocr_config_v2(device=0, **kw)), C.byref(h)) == -1 and not h.value, kw
    for kw in ({"beam_wide": 1}, {"beam_wide": 1, "rec_classes": 6719}, {"beam_wide": 0, "rec_classes": 6719}):
        h = C.c_void_p()
        rc = lib.bbocr_create_v2(C.byref(_lib.bbocr_config_v2(device=10 ** 6, **kw)), C.byref(h))          # no such device anywhere
        assert rc not in (0, -1) and not h.value, (kw, rc)
    assert lib.bbocr_create_v2(None, None) == -1 and lib.bbocr_op_ctc_beam_wide(None, None, 0, None, 0, 0, 0, 0, None, None, None) == -1


def test_reader_has_the_option():
    """Reader(beam_wide=None): None means the environment variable BBOCR_BEAM_WIDE (the constructor itself needs a device)"""
    import inspect

    import bb_ocr_amd

    assert inspect.signature(bb_ocr_amd.Reader.__init__).parameters["beam_wide"].default is None
    assert hasattr(bb_ocr_amd.Reader, "ctc_beam_wide_device")
