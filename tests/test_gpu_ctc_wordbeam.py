"""-m gpu: decoder='wordbeamsearch' on the device (csrc/ctc_wordbeam.hip).  Stage by stage -- the word-group kernel against the host rule, the
dictionary lookup against set membership, the search against bbocr_host_ctc_wordbeam on the families of tests/ctc_wordbeam_cases.py
(test_ctc_wordbeam_cpu.py shows that each family aims where it claims) -- and end to end through readtext on the trained reader.  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_cases as beam
import ctc_wordbeam_cases as cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1
GUARD = -7
U16, I32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int)


def set_words(reader, words, space):
    """the context's dictionary as class-index strings (the cases' alphabets are not the model's characters); () clears it"""
    sym, off, n = cases.flat_words(words)
    return reader._lib.bbocr_set_dictionary(reader._h, sym.ctypes.data_as(U16), off.ctypes.data_as(I32), n, space)


@pytest.fixture()
def ctx(reader):
    """the shared Reader, left WITHOUT a dictionary: other modules pin what it does then"""
    yield reader
    assert set_words(reader, (), 0) == 0


def device(reader, fam):
    """bbocr_op_ctc_wordbeam over (rows, width, dictionary) cases: one ragged table per (C, width, dictionary), rows embedded at stride 112, the
    text buffer between guard values"""
    out = [None] * len(fam)
    groups = {}
    for i, c in enumerate(fam):
        groups.setdefault((c[0].shape[1], c[1], c[2]), []).append(i)
    for (Cn, w, words), members in groups.items():
        assert set_words(reader, words, cases.space_of(Cn)) == 0
        pool = torch.from_numpy(np.concatenate([beam.embed(fam[i][0]) for i in members])).cuda()
        first = np.concatenate([[0], np.cumsum([fam[i][0].shape[0] for i in members])]).astype(int)
        n, rows = len(members), int(first[-1])
        tab = (C.c_int * (2 * n))(*[int(v) for k, i in enumerate(members) for v in (first[k], fam[i][0].shape[0])])
        off = (C.c_int * (n + 1))(*([GUARD] * (n + 1)))
        idx = (C.c_int * (rows + 8))(*([GUARD] * (rows + 8)))
        reader._check(reader._lib.bbocr_op_ctc_wordbeam(reader._h, C.c_void_p(pool.data_ptr()), rows, tab, n, Cn, pool.shape[1], w, off, idx))
        assert off[0] == 0 and off[n] <= rows and all(v == GUARD for v in idx[off[n]:]) and all(v != GUARD for v in idx[:off[n]])
        for k, i in enumerate(members):
            out[i] = idx[off[k]:off[k + 1]]
    return out


@pytest.mark.parametrize("name", list(cases.FAMILIES))
def test_device_search_equals_the_host_search(ctx, name):
    fam = cases.family(name)
    want = cases.host_texts(ctx._lib, fam)
    got = device(ctx, fam)
    bad = [i for i in range(len(fam)) if got[i] != want[i]]
    assert not bad, (name, len(bad), bad[:5], [(got[i], want[i], fam[i][1], fam[i][0].shape, fam[i][3]) for i in bad[:3]])
    assert device(ctx, fam) == got                                                  # run twice: the same texts


def test_ragged_table_of_300_sequences(ctx):
    """T from 0 to 48 in shuffled order in ONE launch: segments of many sequences share the segment table and the grid-stride loop"""
    pool, seqs, words = cases.ragged_table()
    fam = [(pool[a:a + T], 5, words) for a, T in seqs]
    want = cases.host_texts(ctx._lib, fam)
    assert set_words(ctx, words, 43) == 0
    dev = torch.from_numpy(beam.embed(pool)).cuda()
    tab = [(int(a), int(T)) for a, T in seqs]
    got = ctx.ctc_wordbeam_device(dev, tab, 5)
    assert len(got) == len(seqs) >= 300
    assert [i for i in range(len(fam)) if got[i] != want[i]] == []
    assert all(got[i] == [] for i in np.nonzero(seqs[:, 1] == 0)[0]) and (seqs[:, 1] == 1).any() and any(43 in g for g in got)
    plain = ctx.ctc_beam_device(dev, tab, 5)
    assert sum(g != p for g, p in zip(got, plain)) >= 20                             # the dictionary (and the grouping) changes texts
    assert ctx.ctc_wordbeam_device(dev, tab, 5) == got
    for w in (1, 32):
        assert ctx.ctc_wordbeam_device(dev, tab[:60], w) == cases.host_texts(ctx._lib, [(r, w, d) for r, _, d in fam[:60]])


def test_word_segments_equal_the_host_rule(ctx):
    fam = cases.family("segmentation") + cases.family("join")
    for Cn in (4, 8, 97):
        members = [c for c in fam if c[0].shape[1] == Cn]
        a = np.concatenate([c[0].argmax(axis=1) for c in members]).astype(np.int32)
        first = np.concatenate([[0], np.cumsum([c[0].shape[0] for c in members])]).astype(int)
        tab = [(int(first[k]), c[0].shape[0]) for k, c in enumerate(members)]
        got = ctx.word_segments_device(torch.from_numpy(a).cuda(), tab, cases.space_of(Cn))
        want = [[(f + s, n) for s, n in cases.segments_py(a[f:f + T], cases.space_of(Cn))] for f, T in tab]
        assert got == want, Cn
        assert any(len(g) == 0 for g in got) or Cn != 8
    pool, seqs, _ = cases.ragged_table()
    a = pool.argmax(axis=1).astype(np.int32)
    tab = [(int(f), int(T)) for f, T in seqs]
    got = ctx.word_segments_device(torch.from_numpy(a).cuda(), tab, 43)
    assert got == [[(f + s, n) for s, n in cases.segments_py(a[f:f + T], 43)] for f, T in tab]
    assert sum(len(g) for g in got) > 600 and ctx.word_segments_device(torch.from_numpy(a).cuda(), tab, 43) == got
    # every chunk boundary: runs that start and end at each position around rows 64 and 128 of one long sequence
    rng = np.random.default_rng(5)
    long_rows = [(rng.random(200) < p).astype(np.int32) * 43 for p in (0.05, 0.5, 0.95)]
    long_rows += [np.array([43] * s + [1] * n + [43] * (200 - s - n), dtype=np.int32) for s in (0, 62, 63, 64, 65, 127, 128) for n in (1, 2, 64, 65, 72)]
    for a in long_rows:
        assert ctx.word_segments_device(torch.from_numpy(a).cuda(), [(0, 200), (3, 190)], 43) == \
            [cases.segments_py(a, 43), [(3 + s, n) for s, n in cases.segments_py(a[3:193], 43)]]


def test_dict_lookup_equals_set_membership(ctx):
    for words, nslots, queries, claim in cases.table_cases():
        found, probe = ctx.dict_lookup_device(queries, words, nslots)
        member = set(words)
        assert found == [int(q in member) for q in queries], claim
        assert probe == cases.table_py(words, nslots)[1]
    words, probes = cases.big_dictionary()
    member = set(words)
    found, probe = ctx.dict_lookup_device(probes, words)
    assert found == [int(p in member) for p in probes] and 0 < sum(found) < len(probes) and probe == cases.table_py(words)[1]
    # ... and through the context's own table
    assert set_words(ctx, words[:2000], 43) == 0
    found, probe2 = ctx.dict_lookup_device(probes[:500] + words[:50])
    assert found == [int(p in set(words[:2000])) for p in probes[:500] + words[:50]] and sum(found) >= 50
    w, sl, pr, un = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert ctx._lib.bbocr_dictionary_stats(ctx._h, C.byref(w), C.byref(sl), C.byref(pr), C.byref(un)) == 0
    kept = list(dict.fromkeys(words[:2000]))
    assert (w.value, sl.value, pr.value) == (len(kept), 4096, probe2) and pr.value == cases.table_py(kept)[1]
    assert un.value == sum(any(a == b for a, b in zip(x, x[1:])) for x in kept)


PAGE = dict(width=640, height=384, lines=5, margin=24)
# A word of page 326 whose LOWER-ranked final candidates at width 5 hold another text (found by searching the page's word groups against
# the one-edit variants of its words): with LOWER in the dictionary and WORD absent, the word search returns LOWER where 'beamsearch'
# returns WORD.
SEED, WORD, LOWER = 326, "harry", "hary"


def _vocabulary_legs(r, img, vocabulary):
    """the page under a dictionary of its own words: route 6 at widths 5 and 32, route 5 at width 33, the greedy call's boxes and confidences"""
    r.set_dictionary(vocabulary)
    stats = r.dictionary_stats()
    assert stats["words"] == len(vocabulary) and stats["dropped_foreign"] == 0 and stats["longest_probe"] >= 1 and stats["slots"] >= 2 * len(vocabulary)
    assert stats["unmatchable_repeats"] == sum(any(a == b for a, b in zip(w, w[1:])) for w in vocabulary)
    plain = r.readtext(img)
    assert len(plain) >= 5 and any(p[1] for p in plain)
    out = {}
    for w, route in ((5, 6), (beam.BEAM_DEVICE_MAX, 6), (beam.BEAM_DEVICE_MAX + 1, 5)):          # width 33: the host route
        out[w] = r.readtext(img, decoder="wordbeamsearch", beamWidth=w)
        assert r.last_ctc_route() == route, w
        assert [b[0] for b in out[w]] == [p[0] for p in plain] and [b[2] for b in out[w]] == [p[2] for p in plain], w
        assert sum(v in " ".join(b[1] for b in out[w]).split() for v in vocabulary) >= len(vocabulary) // 2, w
    return out


def test_readtext_wordbeamsearch(readers_trained):
    from bb_ocr_amd import synth

    r = readers_trained["fp16"]
    try:
        # page 321: the device route and the host route return the same strings (widths 32 and 33 hold the same final candidates on this
        # page; that route 6 is route 5's function of the same rows at ONE width is what the op tests pin, exactly)
        img, boxes = synth.page(321, **PAGE)
        out = _vocabulary_legs(r, img, sorted({b[4] for b in boxes}))
        assert [b[1] for b in out[beam.BEAM_DEVICE_MAX]] == [b[1] for b in out[beam.BEAM_DEVICE_MAX + 1]]
        # page SEED: the same legs, then a dictionary that holds a lower-ranked candidate of one word instead of the word
        img, boxes = synth.page(SEED, **PAGE)
        vocabulary = sorted({b[4] for b in boxes})
        _vocabulary_legs(r, img, vocabulary)
        beamed = r.readtext(img, decoder="beamsearch", beamWidth=5)
        assert WORD in " ".join(b[1] for b in beamed).split()
        r.set_dictionary([w for w in vocabulary if w != WORD] + [LOWER])
        lower = r.readtext(img, decoder="wordbeamsearch", beamWidth=5)
        assert r.last_ctc_route() == 6
        assert [b[1] for b in lower] != [b[1] for b in beamed] and LOWER in " ".join(b[1] for b in lower).split()
        assert lower == r.readtext(img, decoder="wordbeamsearch", beamWidth=5)
        # the other callers take the decoder too
        t = torch.from_numpy(img[None]).cuda()
        assert [b[1] for b in r.readtext_device(t, decoder="wordbeamsearch")[0]] == [b[1] for b in lower]
    finally:
        r.set_dictionary([])
    with pytest.raises(NotImplementedError):
        r.readtext(img, decoder="wordbeamsearch")


def test_argument_errors(ctx):
    lib, h = ctx._lib, ctx._h
    rows, Cn, cs = 8, 97, 112
    probs = torch.from_numpy(beam.embed(beam.peaked_rows(1, rows))).cuda()
    pp = C.c_void_p(probs.data_ptr())
    off, idx = (C.c_int * 3)(-5, -5, -5), (C.c_int * 16)(*([-5] * 16))
    ok = (C.c_int * 4)(0, 4, 4, 4)

    def search(p=pp, rows=rows, seqs=ok, nseq=2, Cn=Cn, cs=cs, w=5, off=off, idx=idx):
        return lib.bbocr_op_ctc_wordbeam(h, p, rows, seqs, nseq, Cn, cs, w, off, idx)

    assert set_words(ctx, (), 0) == 0
    assert search() == ERR_ARG                                                       # no dictionary on the context
    for bad in (((0, 5),), ((5, 43),), ((97,),), ((5, 6), ()), ((1,) * 1025,)):      # symbol 0, the space class, a symbol >= C, an empty word, 1025 symbols
        assert set_words(ctx, bad, 43) == ERR_ARG
    assert set_words(ctx, ((5, 6),), 0) == ERR_ARG and set_words(ctx, ((5, 6),), 97) == ERR_ARG
    assert lib.bbocr_set_dictionary(h, None, None, 1, 43) == ERR_ARG
    assert search() == ERR_ARG                                                       # a refused table has changed nothing: still none
    assert set_words(ctx, ((5, 6), (7,)), 43) == 0
    assert set_words(ctx, ((0, 5),), 43) == ERR_ARG                                  # ... and a refused table keeps the one before it
    assert ctx.dict_lookup_device([(5, 6), (7,), (5,)]) == ([1, 1, 0], 1)
    assert search(p=None) == ERR_ARG and search(seqs=None) == ERR_ARG and search(off=None) == ERR_ARG and search(idx=None) == ERR_ARG
    assert search(cs=96) == ERR_ARG and search(Cn=129, cs=136) == ERR_ARG and search(Cn=40, cs=112) == ERR_ARG       # the space class 43 lies outside 40 classes
    assert search(w=0) == ERR_ARG and search(w=-1) == ERR_ARG and search(w=beam.BEAM_DEVICE_MAX + 1) == ERR_ARG
    assert search(seqs=(C.c_int * 4)(0, 4, 5, 4)) == ERR_ARG and search(seqs=(C.c_int * 4)(-1, 4, 4, 4)) == ERR_ARG and search(seqs=(C.c_int * 4)(0, 4, 4, -1)) == ERR_ARG
    assert list(off) == [-5] * 3 and list(idx) == [-5] * 16                          # a refused call has written nothing
    assert search() == 0 and off[0] == 0 and off[2] <= 8
    seg_off, segs = (C.c_int * 3)(-5, -5, -5), (C.c_int * 16)(*([-5] * 16))
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    pa = C.c_void_p(a.data_ptr())
    assert lib.bbocr_op_word_segments(h, None, 8, ok, 2, 43, seg_off, segs) == ERR_ARG and lib.bbocr_op_word_segments(h, pa, 8, None, 2, 43, seg_off, segs) == ERR_ARG
    assert lib.bbocr_op_word_segments(h, pa, 8, ok, 2, 43, None, segs) == ERR_ARG and lib.bbocr_op_word_segments(h, pa, 8, ok, 2, 43, seg_off, None) == ERR_ARG
    assert lib.bbocr_op_word_segments(h, pa, 8, (C.c_int * 4)(0, 4, 5, 4), 2, 43, seg_off, segs) == ERR_ARG
    assert list(seg_off) == [-5] * 3 and list(segs) == [-5] * 16
    assert lib.bbocr_op_word_segments(h, pa, 8, ok, 2, 43, seg_off, segs) == 0 and list(seg_off) == [0, 1, 2] and list(segs[:4]) == [0, 4, 4, 4]
    q, qo, found = (C.c_uint16 * 2)(5, 6), (C.c_int * 2)(0, 2), (C.c_int * 1)(-5)
    assert lib.bbocr_op_dict_lookup(h, None, None, 0, 0, None, qo, 1, found, None) == ERR_ARG
    assert lib.bbocr_op_dict_lookup(h, None, None, 0, 0, q, None, 1, found, None) == ERR_ARG
    assert lib.bbocr_op_dict_lookup(h, None, None, 0, 0, q, qo, 1, None, None) == ERR_ARG
    assert lib.bbocr_op_dict_lookup(h, q, qo, 1, 3, q, qo, 1, found, None) == ERR_ARG and found[0] == -5         # 3 slots: no power of two
    assert lib.bbocr_op_dict_lookup(h, (C.c_uint16 * 2)(5, 200), qo, 1, 0, q, qo, 1, found, None) == ERR_ARG  # the device table holds bytes below 128
    assert lib.bbocr_op_dict_lookup(h, q, qo, 1, 0, q, qo, 1, found, None) == 0 and found[0] == 1


def test_a_reader_without_a_dictionary_still_refuses(reader):
    with pytest.raises(NotImplementedError):
        reader.readtext(np.zeros((64, 64, 3), dtype=np.uint8), decoder="wordbeamsearch")
    assert reader.dictionary_stats() == {"words": 0, "dropped_foreign": 0, "unmatchable_repeats": 0, "slots": 0, "longest_probe": 0}
    from bb_ocr_amd import _lib, synth

    p = reader._params({})
    p.decoder, p.beam_width = 2, 5                                                  # past the Reader: the library refuses as well
    t = torch.from_numpy(synth.page(321, **PAGE)[0][None]).cuda()
    res = C.POINTER(_lib.bbocr_result)()
    assert reader._lib.bbocr_readtext_batch(reader._h, C.c_void_p(t.data_ptr()), None, 1, PAGE["height"], PAGE["width"], C.byref(p), C.byref(res)) == ERR_ARG
    assert b"dictionary" in reader._lib.bbocr_last_error(reader._h)
