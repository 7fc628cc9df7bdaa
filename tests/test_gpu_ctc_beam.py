"""-m gpu: decoder='beamsearch' on the device.  bbocr_op_ctc_beam (ctc_beam.hip, one wave per sequence) must give bbocr_host_ctc_beam's text
on the same float32 rows EXACTLY, sequence by sequence, on the families of tests/ctc_beam_cases.py (test_ctc_beam_cases_cpu.py shows that
each family can fail), and bbocr_op_ctc / readtext must reach that kernel and keep the greedy path's boxes and confidences."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_cases as cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FAMILIES = {"small_alphabet": cases.small_alphabet_cases, "ties": cases.tie_cases, "underflow": cases.underflow_cases,
            "saturation": cases.saturation_cases, "peaked": cases.peaked_cases}
_host = {}


def host(reader, name, cs):
    """the yardstick's answers, computed once per family"""
    if name not in _host:
        _host[name] = cases.host_texts(reader._lib, cs)
    return _host[name]


def device(reader, cs):
    """bbocr_op_ctc_beam over (rows, width) cases: one ragged table per (C, width), rows embedded at stride 112"""
    out = [None] * len(cs)
    groups = {}
    for i, (rows, w) in enumerate(cs):
        groups.setdefault((rows.shape[1], w), []).append(i)
    for (Cn, w), members in groups.items():
        pool = torch.from_numpy(np.concatenate([cases.embed(cs[i][0]) for i in members])).cuda()
        first = np.concatenate([[0], np.cumsum([cs[i][0].shape[0] for i in members])])
        texts = reader.ctc_beam_device(pool, [(int(first[k]), cs[i][0].shape[0]) for k, i in enumerate(members)], w, C=Cn)
        for i, t in zip(members, texts):
            out[i] = t
    return out


@pytest.mark.parametrize("name", list(FAMILIES))
def test_device_search_equals_the_host_search(reader, name):
    cs = FAMILIES[name]()
    want = host(reader, name, cs)
    got = device(reader, cs)
    bad = [i for i in range(len(cs)) if got[i] != want[i]]
    assert not bad, (name, len(bad), bad[:5], [(got[i], want[i], cs[i][1], cs[i][0].shape) for i in bad[:3]])
    assert device(reader, cs) == got                                               # run twice: the same texts


def test_ragged_table_of_300_sequences(reader):
    """T from 0 to 639 in shuffled order in ONE launch; T = 0 gives the empty text, T = 1 is in the table"""
    pool, seqs = cases.ragged_table()
    cs = [(pool[a:a + T], 5) for a, T in seqs]
    want = host(reader, "ragged", cs)
    dev = torch.from_numpy(cases.embed(pool)).cuda()
    got = reader.ctc_beam_device(dev, [(int(a), int(T)) for a, T in seqs], 5)
    assert len(got) == len(seqs) >= 300
    assert [i for i in range(len(cs)) if got[i] != want[i]] == []
    assert all(got[i] == [] for i in np.nonzero(seqs[:, 1] == 0)[0]) and (seqs[:, 1] == 1).any()
    assert any(g for g in got)
    assert reader.ctc_beam_device(dev, [(int(a), int(T)) for a, T in seqs], 5) == got


@pytest.mark.parametrize("width", [1, 2, 5, 10, cases.BEAM_DEVICE_MAX])
def test_every_width_on_trained_like_rows(reader, width):
    cs = [(cases.peaked_rows(500 + i, T), width) for i, T in enumerate((1, 7, 40, 64, 129))]
    cs += [(cases.peaked_rows(600 + i, 48, undecided=0.7), width) for i in range(4)]          # many undecided steps: wide beams stay full
    want = host(reader, f"widths{width}", cs)
    assert device(reader, cs) == want
    assert width == 1 or any(w != cases.greedy_collapse(r) for (r, _), w in zip(cs, want))


def _op_ctc(reader, d, n, T, Cn, cs, mask, bw):
    off, idx, conf = (C.c_int * (n + 1))(), (C.c_int * (n * T))(), (C.c_double * n)()
    reader._check(reader._lib.bbocr_op_ctc(reader._h, C.c_void_p(d.data_ptr()), n, T, Cn, cs, off, idx, conf, mask, bw))
    return [[idx[k] for k in range(off[i], off[i + 1])] for i in range(n)], list(conf)


def test_op_ctc_reaches_the_device_search(reader):
    """bbocr_op_ctc(beam_width) == bbocr_host_ctc_beam on bbocr_op_ctc_probs' rows; the confidences are the greedy call's"""
    import bb_ocr_amd
    from bb_ocr_amd.reader import ignore_mask

    rng = np.random.default_rng(17)
    n, T, Cn, cs = 9, 83, 97, 112
    logits = (rng.standard_normal((n, T, cs)) * 1.5).astype(np.float32)
    logits[:, :, 0] += 2.0
    d = torch.from_numpy(logits).cuda()
    words = ignore_mask(bb_ocr_amd.CHARACTER, list(bb_ocr_amd.CHARSET), blocklist="aeiouAEIOU -")
    for bw, mask in ((5, None), (3, (C.c_uint * 4)(*words))):
        probs = torch.full((n * T, cs), 7.0, dtype=torch.float32, device="cuda")
        reader._check(reader._lib.bbocr_op_ctc_probs(reader._h, C.c_void_p(d.data_ptr()), n * T, Cn, cs, mask, C.c_void_p(probs.data_ptr())))
        ph = probs.cpu().numpy().reshape(n, T, cs)
        assert np.allclose(ph[:, :, :Cn].sum(axis=2), 1.0, atol=1e-5) and (ph[:, :, Cn:] == 7.0).all()
        want = cases.host_texts(reader._lib, [(ph[i, :, :Cn], bw) for i in range(n)])
        got, conf = _op_ctc(reader, d, n, T, Cn, cs, mask, bw)
        greedy, gconf = _op_ctc(reader, d, n, T, Cn, cs, mask, 0)
        assert got == want and conf == gconf
        assert got != greedy                                                        # the search changes some strings
        assert reader.ctc_beam_device(probs, [(i * T, T) for i in range(n)], bw) == want


def test_readtext_beamsearch_keeps_boxes_and_confidences(readers_trained):
    """decoder='beamsearch' on the trained page: width 5 runs on the device, width BBOCR_BEAM_DEVICE_MAX + 1 on the host; both return the
    greedy call's boxes and confidences, and two calls in flight return what serial calls return"""
    from bb_ocr_amd import synth

    r = readers_trained["fp16"]
    img = synth.page(321, width=640, height=384, lines=5, margin=24)[0]
    plain = r.readtext(img)
    assert len(plain) >= 5 and any(p[1] for p in plain)
    for w in (5, cases.BEAM_DEVICE_MAX + 1):
        beam = r.readtext(img, decoder="beamsearch", beamWidth=w)
        assert [b[0] for b in beam] == [p[0] for p in plain] and [b[2] for b in beam] == [p[2] for p in plain], w
    batches = [torch.from_numpy(np.stack([synth.page(81_000 + 10 * k + i, width=640, height=384, lines=3 + i, margin=24)[0] for i in range(3)])).cuda()
               for k in range(3)]
    serial = [r.readtext_device(b, decoder="beamsearch", beamWidth=5) for b in batches]
    assert all(any(p) for p in serial)
    assert list(r.readtext_stream(iter(batches * 2), decoder="beamsearch", beamWidth=5)) == serial * 2


def test_argument_errors(reader):
    lib, h = reader._lib, reader._h
    rows, Cn, cs = 8, 97, 112
    probs = torch.from_numpy(cases.embed(cases.peaked_rows(1, rows))).cuda()
    pp = C.c_void_p(probs.data_ptr())
    off, idx = (C.c_int * 3)(-5, -5, -5), (C.c_int * 16)(*([-5] * 16))
    ok = (C.c_int * 4)(0, 4, 4, 4)

    def beam(p=pp, rows=rows, seqs=ok, nseq=2, Cn=Cn, cs=cs, w=5, off=off, idx=idx):
        return lib.bbocr_op_ctc_beam(h, p, rows, seqs, nseq, Cn, cs, w, off, idx)

    assert beam(p=None) == ERR_ARG and beam(seqs=None) == ERR_ARG and beam(off=None) == ERR_ARG and beam(idx=None) == ERR_ARG
    assert beam(cs=96) == ERR_ARG and beam(Cn=129, cs=136) == ERR_ARG
    assert beam(w=0) == ERR_ARG and beam(w=-1) == ERR_ARG and beam(w=cases.BEAM_DEVICE_MAX + 1) == ERR_ARG
    assert beam(seqs=(C.c_int * 4)(0, 4, 5, 4)) == ERR_ARG and beam(seqs=(C.c_int * 4)(-1, 4, 4, 4)) == ERR_ARG      # outside [0, rows)
    assert beam(seqs=(C.c_int * 4)(0, 4, 4, -1)) == ERR_ARG
    assert list(off) == [-5] * 3 and list(idx) == [-5] * 16                          # a refused call has written nothing
    assert beam() == 0 and off[0] == 0 and off[2] <= 8
    out = torch.full((rows, cs), 3.0, dtype=torch.float32, device="cuda")
    po = C.c_void_p(out.data_ptr())
    assert lib.bbocr_op_ctc_probs(h, None, rows, Cn, cs, None, po) == ERR_ARG
    assert lib.bbocr_op_ctc_probs(h, pp, rows, Cn, cs, None, None) == ERR_ARG
    assert lib.bbocr_op_ctc_probs(h, pp, rows, Cn, 96, None, po) == ERR_ARG
    assert lib.bbocr_op_ctc_probs(h, pp, rows, 129, 136, None, po) == ERR_ARG
    assert lib.bbocr_op_ctc_probs(h, pp, 0, Cn, cs, None, po) == ERR_ARG
    assert (out == 3.0).all().item()
