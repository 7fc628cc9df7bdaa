"""CPU: decoder='wordbeamsearch' on the host.  bbocr_host_ctc_wordbeam (csrc/ctc_wordbeam.cpp, the definition) against the Python
restatement of tests/ctc_wordbeam_cases.py on every family, exactly; the families' own claims; the route rule at its edges; the Reader-side
loading of a word list; and tools/wordbeam_hostcheck under a sanitizer."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ctc_beam_cases as beam
import ctc_wordbeam_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


def test_constants_are_the_headers():
    import re

    from bb_ocr_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "bbocr.h")).read()
    assert int(re.search(r"#define BBOCR_WORD_CANDIDATES (\d+)", hdr).group(1)) == cases.WORD_CANDIDATES
    assert re.search(r"BBOCR_DECODER_WORDBEAMSEARCH = 2", hdr)
    wd = open(os.path.join(ROOT, "bb-ocr_amd", "csrc", "word_dict.h")).read()
    assert int(re.search(r"WD_WORD_MAX = (\d+)", wd).group(1)) == cases.WORD_MAX
    for name in ("bbocr_host_ctc_wordbeam", "bbocr_host_wordbeam_route", "bbocr_set_dictionary", "bbocr_dictionary_stats", "bbocr_op_word_segments",
                 "bbocr_op_dict_lookup", "bbocr_op_ctc_wordbeam"):
        assert name in _lib.PROTOTYPES


@pytest.mark.parametrize("name", list(cases.FAMILIES))
def test_family_aims_where_it_claims(name):
    share = cases.check_claims(name)
    if name in cases.RANK_FAMILIES:
        assert share >= 0.5, share          # at least half of the dictionary-rank cases differ from plain beam search per group


def test_table_families_aim_where_they_claim():
    cases.check_table_claims()
    words, probes = cases.big_dictionary()
    member = set(words)
    n = sum(p in member for p in probes)
    assert len(words) == 50_000 and len(probes) == 10_000 and 4000 < n < 6500


@pytest.mark.parametrize("name", list(cases.FAMILIES))
def test_host_search_equals_the_restatement(lib, name):
    fam = cases.family(name)
    got = cases.host_texts(lib, fam)
    want = [cases.wordbeam_search_py(rows, w, words) for rows, w, words, _ in fam]
    bad = [i for i in range(len(fam)) if got[i] != want[i]]
    assert not bad, (name, bad[:5], [(got[i], want[i], fam[i][3]) for i in bad[:3]])


def test_ragged_table_on_the_host(lib):
    pool, seqs, words = cases.ragged_table()
    fam = [(pool[a:a + T], 5, words) for a, T in seqs]
    got = cases.host_texts(lib, fam)
    want = [cases.wordbeam_search_py(r, w, d) if len(r) else [] for r, w, d in fam]
    assert got == want
    plain = [cases.beam_per_group_py(r, w) if len(r) else [] for r, w, _ in fam]
    assert sum(g != p for g, p in zip(got, plain)) >= 20          # the dictionary changes texts here too


@pytest.mark.parametrize("name", list(cases.FAMILIES))
def test_empty_dictionary_is_beam_search_per_group(lib, name):
    """with no word, every group decodes as bbocr_host_ctc_beam decodes its rows, and the words are joined by the space"""
    for rows, w, _, _ in cases.family(name):
        sp = cases.space_of(rows.shape[1])
        want = []
        for k, (a, n) in enumerate(cases.segments_py(rows.argmax(axis=1), sp)):
            want += ([sp] if k else []) + beam.host_texts(lib, [(rows[a:a + n], w)])[0]
        assert cases.host_text(lib, rows, w, ()) == want


def test_host_argument_errors(lib):
    rows = np.ascontiguousarray(beam.embed(cases.pattern_rows([1, 7, 2], 8, 1)))
    p = rows.ctypes.data_as(C.POINTER(C.c_float))
    off, idx = (C.c_int * 2)(), (C.c_int * 3)()
    u16, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int)

    def call(words=((1, 2),), space=7, Cn=8, w=5, p=p, off=off, idx=idx):
        sym, woff, n = cases.flat_words(words)
        return lib.bbocr_host_ctc_wordbeam(p, 1, 3, Cn, beam.CS, w, space, sym.ctypes.data_as(u16), woff.ctypes.data_as(i32), n, off, idx)

    assert call() == 0
    assert call(words=((0, 1),)) == -1 and call(words=((1, 7),)) == -1 and call(words=((8,),)) == -1 and call(words=((),)) == -1
    assert call(words=(tuple([1, 2] * 513),)) == -1 and call(words=(tuple([1, 2] * 512),)) == 0           # 1026 / 1024 symbols
    assert call(w=0) == -1 and call(space=0) == -1 and call(space=8) == -1 and call(p=None) == -1 and call(off=None) == -1 and call(idx=None) == -1


def test_route_rule_at_its_edges(lib):
    from bb_ocr_amd import _lib

    def route(w, Cn, T):
        return lib.bbocr_host_wordbeam_route(w, Cn, (C.c_int * 4)(0, T, T, 1), 2)

    assert route(32, 97, 40) == 6 and route(33, 97, 40) == 5 and _lib.BEAM_DEVICE_MAX == 32
    assert route(5, 128, 40) == 6 and route(5, 129, 40) == 5

    def lds_bytes(w, Cn, T):            # csrc/ctc_beam_steps.h's LDS sum with sel[max(W, 20)], plus the collapsed text's line
        ts = (max(T, 1) + 3) & ~3
        return 4 * (3 * 128 + 15 * w + max(w, cases.WORD_CANDIDATES) + w * (1 + Cn) + 2 * w * (ts // 4) + ts // 4)

    for w, Cn in ((32, 97), (5, 97), (1, 4), (32, 128)):
        T = max(t for t in range(1, 30000) if lds_bytes(w, Cn, t) <= 65536)
        assert route(w, Cn, T) == 6 and route(w, Cn, T + 1) == 5, (w, Cn, T)
    assert route(0, 97, 4) == -1 and lib.bbocr_host_wordbeam_route(5, 97, None, 1) == -1
    # values 0 .. 4 keep their meaning
    assert lib.bbocr_host_ctc_route(0, 5, 97, (C.c_int * 2)(0, 40), 1) == 2 and lib.bbocr_host_ctc_route(0, 0, 97, (C.c_int * 2)(0, 40), 1) == 0


def test_reader_side_loading(tmp_path, monkeypatch):
    from bb_ocr_amd import CHARACTER
    from bb_ocr_amd.reader import load_dictionary

    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes("\ufeffcover\n\nbook\r\ncover\nnaïve中\nTitle\n".encode("utf-8"))          # BOM, blank line, duplicate, foreign character
    b.write_text("page\ntwo words\nhello\ncover\n", encoding="utf-8")
    d = load_dictionary(str(a), CHARACTER)
    assert d["words"] == ["cover", "book", "Title"] and d["dropped_empty"] == 1 and d["dropped_duplicates"] == 1 and d["dropped_foreign"] == 1
    assert d["unmatchable_repeats"] == 1 and d["space"] == CHARACTER.index(" ") == 43                  # "book"
    assert d["word_off"].tolist() == [0, 5, 9, 14] and d["symbols"].dtype == np.uint16
    assert [CHARACTER[i] for i in d["symbols"][:5]] == list("cover")
    d2 = load_dictionary([str(a), b], CHARACTER)
    assert d2["words"] == ["cover", "book", "Title", "page", "hello"] and d2["dropped_foreign"] == 2 and d2["dropped_duplicates"] == 2
    assert d2["unmatchable_repeats"] == 2
    d3 = load_dictionary(["cover", "cover", "", "bäd"], CHARACTER)                                  # an iterable of words
    assert d3["words"] == ["cover"] and (d3["dropped_duplicates"], d3["dropped_empty"], d3["dropped_foreign"]) == (1, 1, 1)
    assert load_dictionary(iter(["x" * 1025, "x" * 3]), CHARACTER)["words"] == ["xxx"]
    monkeypatch.delenv("BBOCR_DICTIONARY", raising=False)
    assert load_dictionary(None, CHARACTER) is None
    monkeypatch.setenv("BBOCR_DICTIONARY", os.pathsep.join([str(a), str(b)]))
    assert load_dictionary(None, CHARACTER)["words"] == d2["words"]
    with pytest.raises(ValueError):
        load_dictionary(["ab"], ["[blank]", "a", "b"])                                                   # a model without ' '


def test_hostcheck_runs_clean_under_a_sanitizer():
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no clang++ to build the host check with")
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("this compiler cannot link a sanitized host program")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wordbeam_hostcheck.py"), "--cxx", cxx], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 mismatches, 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
