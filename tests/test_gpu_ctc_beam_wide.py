"""-m gpu: decoder='beamsearch' on the device for recognisers of more than 128 classes (bbocr_config_v2::beam_wide).  bbocr_op_ctc_beam_wide
(ctc_beam_wide.hip: a candidate list per row, then one wave per sequence) must give bbocr_host_ctc_beam's text on the same float32 rows
EXACTLY, sequence by sequence, on the families of tests/ctc_beam_wide_cases.py (test_ctc_beam_wide_cpu.py shows that each family can fail)
-- WITHOUT the host fallback, except for the sequences built to overflow the candidate list, and for exactly those -- and bbocr_op_ctc /
readtext of a context with the option must reach those kernels (route 4) and return what the host route returns."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_wide_cases as W

pytestmark = pytest.mark.gpu

ERR_ARG = -1
_R = {}
_host = {}


def stage_reader(beam_wide=True):
    """a recogniser-only Reader of 1,009 classes: the stage entry points of a wide context take every C up to 8,192"""
    import bb_ocr_amd
    from bb_ocr_amd import weights

    if beam_wide not in _R:
        chars = [chr(0x4E00 + k) for k in range(1008)]
        _R[beam_wide] = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=(None, weights.synthetic_crnn_state(0, num_class=1009)),
                                          detector=False, precision="fp16", beam_wide=beam_wide)
    return _R[beam_wide]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for r in _R.values():
        r.close()
    _R.clear()
    _host.clear()


def host(key, cs, Cn):
    """the yardstick's answers, computed once per family"""
    if key not in _host:
        _host[key] = W.host_texts(stage_reader()._lib, cs, W.cs_of(Cn))
    return _host[key]


def embed(rows, Cn):
    out = np.full((rows.shape[0], W.cs_of(Cn)), 7.0, dtype=np.float32)      # behind C: a value no search may read as a probability
    out[:, :Cn] = rows
    return out


def device(cs, Cn):
    """bbocr_op_ctc_beam_wide over (rows, width) cases: one ragged table per width -> (texts, sequences searched on the host)"""
    r = stage_reader()
    out, n_host = [None] * len(cs), 0
    groups = {}
    for i, (_, w) in enumerate(cs):
        groups.setdefault(w, []).append(i)
    for w, members in groups.items():
        pool = torch.from_numpy(np.concatenate([embed(cs[i][0], Cn) for i in members])).cuda()
        first = np.concatenate([[0], np.cumsum([cs[i][0].shape[0] for i in members])])
        texts, nh = r.ctc_beam_wide_device(pool, [(int(first[k]), cs[i][0].shape[0]) for k, i in enumerate(members)], w, Cn)
        n_host += nh
        for i, t in zip(members, texts):
            out[i] = t
    return out, n_host


FAMILIES = ("scattered", "aliases", "subthreshold", "subthreshold_blank", "ties", "trained")


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("Cn", W.CLASSES)
def test_device_search_equals_the_host_search(Cn, name):
    fam = W.families(Cn)
    if name not in fam:
        assert name == "aliases" and Cn == 129                  # no two classes below 129 share a low byte: the family starts at 1,009
        return
    cs = fam[name]
    want = host((Cn, name), cs, Cn)
    got, n_host = device(cs, Cn)
    bad = [i for i in range(len(cs)) if got[i] != want[i]]
    print(f"C={Cn} {name}: {len(cs)} cases, {len(bad)} differ, {n_host} searched on the host")
    assert not bad, (name, len(bad), bad[:5], [(got[i], want[i], cs[i][1], cs[i][0].shape) for i in bad[:3]])
    assert n_host == 0, "the host fallback must not stand in for the kernel"
    assert device(cs, Cn) == (got, 0)                           # run twice: the same texts


@pytest.mark.parametrize("Cn", W.CLASSES)
def test_overflowed_sequences_alone_fall_back(Cn):
    """rows of K - 1, K and K + 1 candidates in ONE table per width: the K + 1 rows send exactly their own sequences to the host"""
    ov = W.overflow_cases(Cn)
    cs = [(r, w) for r, w, _ in ov]
    want = host((Cn, "overflow"), cs, Cn)
    got, n_host = device(cs, Cn)
    built = sum(o for _, _, o in ov)
    print(f"C={Cn} overflow: {len(cs)} cases, {built} built to overflow, {n_host} searched on the host")
    assert got == want
    assert n_host == built and 0 < built < len(cs)
    assert device(cs, Cn) == (got, built)
    mine = [(r, w) for r, w, o in ov if not o]                  # the same rows without their overflowing neighbours: the kernel alone
    assert device(mine, Cn) == ([t for t, (_, _, o) in zip(want, ov) if not o], 0)


@pytest.mark.parametrize("Cn", [1009, 6719])
def test_ragged_table(Cn):
    """62 sequences, T from 0 to 160 in shuffled order, in ONE launch; T = 0 gives the empty text, T = 1 is in the table"""
    pool, seqs = W.ragged_table(Cn)
    cs = [(pool[a:a + T], 5) for a, T in seqs]
    want = host((Cn, "ragged"), cs, Cn)
    dev = torch.from_numpy(embed(pool, Cn)).cuda()
    tab = [(int(a), int(T)) for a, T in seqs]
    got, n_host = stage_reader().ctc_beam_wide_device(dev, tab, 5, Cn)
    assert got == want and n_host == 0 and len(got) == len(seqs) >= 60
    assert all(got[i] == [] for i in np.nonzero(seqs[:, 1] == 0)[0]) and (seqs[:, 1] == 1).any() and any(got)
    assert stage_reader().ctc_beam_wide_device(dev, tab, 5, Cn) == (got, 0)


def test_sequence_at_and_beyond_the_lds_block():
    """width 32 takes T = 356 and refuses T = 358, which width 5 takes"""
    long = W.too_long_rows()
    Cn, T = long.shape[1], W.max_T(W.BEAM_DEVICE_MAX)
    assert long.shape[0] == T + 2
    dev = torch.from_numpy(embed(long, Cn)).cuda()
    r = stage_reader()
    want = host("long", [(long[:T], W.BEAM_DEVICE_MAX), (long, 5)], Cn)
    assert r.ctc_beam_wide_device(dev, [(0, T)], W.BEAM_DEVICE_MAX, Cn) == ([want[0]], 0)
    assert r.ctc_beam_wide_device(dev, [(0, T + 2)], 5, Cn) == ([want[1]], 0)
    with pytest.raises(Exception):
        r.ctc_beam_wide_device(dev, [(0, T + 2)], W.BEAM_DEVICE_MAX, Cn)


def test_argument_errors(reader):
    r = stage_reader()
    lib, h = r._lib, r._h
    rows, Cn, cs = 8, 1009, 1024
    probs = torch.from_numpy(embed(W.peaked_rows_wide(1, rows, Cn), Cn)).cuda()
    pp = C.c_void_p(probs.data_ptr())
    off, idx, nh = (C.c_int * 3)(-5, -5, -5), (C.c_int * 16)(*([-5] * 16)), C.c_int(-5)
    ok = (C.c_int * 4)(0, 4, 4, 4)

    def beam(h=h, p=pp, rows=rows, seqs=ok, nseq=2, Cn=Cn, cs=cs, w=5, off=off, idx=idx, nh=C.byref(nh)):
        return lib.bbocr_op_ctc_beam_wide(h, p, rows, seqs, nseq, Cn, cs, w, off, idx, nh)

    assert beam(p=None) == ERR_ARG and beam(seqs=None) == ERR_ARG and beam(off=None) == ERR_ARG and beam(idx=None) == ERR_ARG
    assert beam(cs=1008) == ERR_ARG and beam(Cn=128, cs=128) == ERR_ARG and beam(Cn=97, cs=112) == ERR_ARG and beam(Cn=8193, cs=8208) == ERR_ARG
    assert beam(w=0) == ERR_ARG and beam(w=-1) == ERR_ARG and beam(w=W.BEAM_DEVICE_MAX + 1) == ERR_ARG
    assert beam(seqs=(C.c_int * 4)(0, 4, 5, 4)) == ERR_ARG and beam(seqs=(C.c_int * 4)(-1, 4, 4, 4)) == ERR_ARG      # outside [0, rows)
    assert beam(seqs=(C.c_int * 4)(0, 4, 4, -1)) == ERR_ARG
    assert beam(nseq=0) == ERR_ARG
    # a T too long for the LDS block at this width (the table lies inside `rows` as the call states them; it is refused before anything runs)
    big = W.max_T(W.BEAM_DEVICE_MAX) + 1
    assert beam(rows=big, seqs=(C.c_int * 2)(0, big), nseq=1, w=W.BEAM_DEVICE_MAX) == ERR_ARG
    assert beam(h=reader._h) == ERR_ARG                                              # a context of 97 classes
    assert list(off) == [-5] * 3 and list(idx) == [-5] * 16 and nh.value == -5      # a refused call has written nothing
    assert beam() == 0 and off[0] == 0 and off[2] <= 8 and nh.value == 0
    assert beam(nh=None) == 0                                                        # n_host may be NULL
    # and the narrow entry point is what it was: 129 classes stay an argument error, on either context
    assert lib.bbocr_op_ctc_beam(h, pp, rows, ok, 2, 129, cs, 5, off, idx) == ERR_ARG
    assert lib.bbocr_op_ctc_beam(reader._h, pp, rows, ok, 2, 129, cs, 5, off, idx) == ERR_ARG


def _op_ctc(reader, d, n, T, Cn, cs, mask, bw):
    off, idx, conf = (C.c_int * (n + 1))(), (C.c_int * (n * T))(), (C.c_double * n)()
    reader._check(reader._lib.bbocr_op_ctc(reader._h, C.c_void_p(d.data_ptr()), n, T, Cn, cs, off, idx, conf, mask, bw))
    return [[idx[k] for k in range(off[i], off[i + 1])] for i in range(n)], list(conf)


@pytest.mark.parametrize("Cn,T,bw", [(1009, 83, 5), (6719, 40, W.BEAM_DEVICE_MAX), (1009, W.max_T(W.BEAM_DEVICE_MAX) + 4, W.BEAM_DEVICE_MAX)])
def test_op_ctc_follows_the_route(Cn, T, bw):
    """bbocr_op_ctc(beam_width) on a context with the option == bbocr_host_ctc_beam on bbocr_op_ctc_probs' rows, with and without a class
    mask; the confidences are the greedy call's; a context without the option gives the same.  The last case is too long for the device at
    width 32 and takes the host route, as ctc_route says (test_ctc_beam_wide_cpu.py::test_routing_rule)."""
    rng = np.random.default_rng(17 + Cn)
    n, cs = 6, W.cs_of(Cn)
    active = np.sort(rng.choice(np.arange(1, Cn), size=40, replace=False))          # a trained model's rows: few classes carry the mass
    logits = np.full((n, T, cs), -20.0, dtype=np.float32)
    logits[:, :, active] = (rng.standard_normal((n, T, 40)) * 1.5).astype(np.float32)
    logits[:, :, 0] = (rng.standard_normal((n, T)) * 1.5 + 2.0).astype(np.float32)
    d = torch.from_numpy(logits).cuda()
    on, plain = stage_reader(True), stage_reader(False)
    words = np.zeros((Cn + 31) // 32, dtype=np.uint32)
    for c in active[::3]:
        words[c >> 5] |= np.uint32(1 << (c & 31))
    for mask in (None, (C.c_uint * len(words))(*words.tolist())):
        probs = torch.full((n * T, cs), 7.0, dtype=torch.float32, device="cuda")
        on._check(on._lib.bbocr_op_ctc_probs(on._h, C.c_void_p(d.data_ptr()), n * T, Cn, cs, mask, C.c_void_p(probs.data_ptr())))
        ph = probs.cpu().numpy().reshape(n, T, cs)
        assert int(W.n_candidates(ph.reshape(n * T, cs)[:, :Cn]).max()) <= W.K
        want = W.host_texts(on._lib, [(ph[i, :, :Cn], bw) for i in range(n)], cs)
        got, conf = _op_ctc(on, d, n, T, Cn, cs, mask, bw)
        greedy, gconf = _op_ctc(on, d, n, T, Cn, cs, mask, 0)
        assert got == want and conf == gconf
        assert got != greedy                                                        # the search changes some strings
        assert _op_ctc(plain, d, n, T, Cn, cs, mask, bw) == (got, conf)
        if T <= W.max_T(bw):
            assert on.ctc_beam_wide_device(probs, [(i * T, T) for i in range(n)], bw, Cn) == (want, 0)
        if mask is not None:
            assert not {int(c) for c in active[::3]} & {s for t in got for s in t}


# ------------------------------------------------------------------------------------------------ end to end
def _wide_model(states_trained, Cn, seed=5):
    """test_gpu_wide_classes.py's model: the trained 97-class recogniser scattered into Cn classes by an injective map (blank stays 0); every
    other class has zero weights and bias -30; the character table has the English characters at the mapped positions"""
    from bb_ocr_amd.reader import CHARSET

    cs, rs = states_trained
    pos = np.sort(np.random.default_rng(seed).choice(np.arange(1, Cn), size=96, replace=False))
    state = dict(rs)
    w = np.zeros((Cn, 256), np.float32)
    b = np.full(Cn, -30.0, np.float32)
    w[0], b[0] = rs["Prediction.weight"][0], rs["Prediction.bias"][0]
    w[pos], b[pos] = rs["Prediction.weight"][1:], rs["Prediction.bias"][1:]
    state["Prediction.weight"], state["Prediction.bias"] = w, b
    chars = [chr(0x4E00 + k) for k in range(Cn - 1)]
    for p, ch in zip(pos, CHARSET):
        chars[p - 1] = ch
    return (cs, state), chars


@pytest.mark.parametrize("Cn", [1009, 6719])
def test_readtext_takes_route_4_and_equals_the_host_route(Cn, states_trained):
    import bb_ocr_amd
    from bb_ocr_amd import synth

    states, chars = _wide_model(states_trained, Cn)
    dev = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states, precision="fp16", beam_wide=True)
    hst = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states, precision="fp16")
    try:
        assert dev.beam_wide and not hst.beam_wide
        img = synth.page(321, width=640, height=384, lines=5, margin=24)[0]
        plain = dev.readtext(img)
        assert dev.last_ctc_route() == 3 and len(plain) >= 5 and any(p[1] for p in plain)      # greedy: the fused kernel, as without the option
        for w in (5, W.BEAM_DEVICE_MAX):
            got = dev.readtext(img, decoder="beamsearch", beamWidth=w)
            assert dev.last_ctc_route() == 4 and dev.last_ctc_host_sequences() == 0, w       # the kernels' text, no sequence left to the host
            want = hst.readtext(img, decoder="beamsearch", beamWidth=w)
            assert hst.last_ctc_route() == 1, w
            assert got == want, w                                                    # boxes, strings and confidences exactly
            assert [g[0] for g in got] == [p[0] for p in plain]                      # (the greedy pass's confidences come from the fused kernel:
            #                                                                          equal to 1e-6, test_gpu_wide_classes.py, not bit for bit)
        got = dev.readtext(img, decoder="beamsearch", beamWidth=W.BEAM_DEVICE_MAX + 1)
        assert dev.last_ctc_route() == 1                                             # width 33: the host
        assert got == hst.readtext(img, decoder="beamsearch", beamWidth=W.BEAM_DEVICE_MAX + 1)
        digits = dev.readtext(img, decoder="beamsearch", beamWidth=5, allowlist="0123456789")
        assert dev.last_ctc_route() == 4
        assert digits == hst.readtext(img, decoder="beamsearch", beamWidth=5, allowlist="0123456789")
        assert all(set(t) <= set("0123456789") for _, t, _ in digits)
        # two calls in flight return what serial calls return
        batches = [torch.from_numpy(np.stack([synth.page(81_000 + 10 * k + i, width=640, height=384, lines=3 + i, margin=24)[0] for i in range(3)])).cuda()
                   for k in range(3)]
        serial = [dev.readtext_device(b, decoder="beamsearch", beamWidth=5) for b in batches]
        assert dev.last_ctc_route() == 4 and all(any(p) for p in serial)
        assert list(dev.readtext_stream(iter(batches * 2), decoder="beamsearch", beamWidth=5)) == serial * 2
        assert serial == [hst.readtext_device(b, decoder="beamsearch", beamWidth=5) for b in batches]
    finally:
        dev.close()
        hst.close()


def test_the_option_changes_nothing_at_97_classes(states_trained, readers_trained):
    import bb_ocr_amd
    from bb_ocr_amd import synth

    r = bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, precision="fp16", beam_wide=True)
    try:
        img = synth.page(321, width=640, height=384, lines=5, margin=24)[0]
        en = readers_trained["fp16"]
        got = r.readtext(img, decoder="beamsearch", beamWidth=5)
        assert r.last_ctc_route() == 2                          # (the record of the thread's LAST call: read before the next one)
        assert got == en.readtext(img, decoder="beamsearch", beamWidth=5) and en.last_ctc_route() == 2
    finally:
        r.close()
