"""-m gpu: the recogniser's ``rec_quant`` mode -- the sequence half in torch's dynamic int8 arithmetic (csrc/quant.hip).

Stage level: bbocr_op_qlinear / bbocr_op_qlstm equal tests/quant_ref.py (which tests/test_quant_ref_cpu.py pins to torch bit for bit) EXACTLY in
everything that is integer or a single fused multiply-add -- parameters, codes, the products' fp32 outputs -- and to 2e-6 through a step's
exp / tanh.  The recurrence is checked step by step from the device's OWN previous state, so nothing drifts.  Whole crops are compared with
torch's dynamically quantised ``oracle.nets.CRNN`` on the CPU under a margin rule whose tolerance (quant_cases.ARGMAX_TOL) comes from the
CPU-side distance between the restatement and torch."""
import ctypes as C

import numpy as np
import pytest
import torch

import quant_cases as QC
import quant_ref as Q
from conftest import LogitTap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rq(states_trained):
    import bb_ocr_amd

    r = bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, rec_quant=True)       # precision None -> exact_rec
    assert r.precision == "exact_rec" and r.rec_quant
    yield r
    r.close()


@pytest.fixture(scope="module")
def qseq(states_trained):
    return Q.QSequence(states_trained[1])


@pytest.fixture(scope="module")
def oracle_quant(states_trained):
    """The CPU reference: the oracle whose recogniser went through torch.quantization.quantize_dynamic, as easyocr's does on a CPU device."""
    from oracle import pipeline

    if not QC.quant_engine_ok():
        pytest.skip("torch reports no fbgemm / x86 quantised engine")
    cs, rs = states_trained
    o = pipeline.OracleReader({k: torch.from_numpy(v) for k, v in cs.items()}, {k: torch.from_numpy(v) for k, v in rs.items()})
    o.recognizer = QC.quantize_dynamic(o.recognizer)
    return o


# ------------------------------------------------------------------------------------------------ one quantised product
def _segments(rows):
    """Crops of 1, 15, 16 and 33 rows in turn until `rows` are used up: boundaries fall anywhere inside the 16-row fragments."""
    out, at, k = [], 0, 0
    while at < rows:
        T = min((1, 15, 16, 33)[k % 4], rows - at)
        out.append((at, T))
        at, k = at + T, k + 1
    return out


def _layer_ref(qseq, layer, x):
    """Reference of one segment for bbocr_op_qlinear's `layer`: (out [T, N], codes, scale, zp)."""
    if layer < 2:
        fwd, bwd = qseq.layers[layer][:2]
        a, cd, s, zp = Q.qlinear(x, fwd.q_ih, fwd.s_ih, fwd.b_ih)
        b = Q.qlinear(x, bwd.q_ih, bwd.s_ih, bwd.b_ih)[0]
        return np.concatenate([a, b], axis=1), cd, s, zp
    if layer < 4:
        _, _, ql, sl, bl = qseq.layers[layer - 2]
        return Q.qlinear(x, ql, sl, bl)
    out, cd, s, zp = Q.qlinear(x, qseq.q_pred, qseq.s_pred, qseq.b_pred)
    return np.concatenate([out, np.zeros((x.shape[0], 15), np.float32)], axis=1), cd, s, zp


@pytest.mark.parametrize("layer", [0, 2, 4], ids=["256to2048", "512to256", "256to97"])
def test_qlinear_op_equals_the_restatement_exactly(rq, qseq, layer):
    """The three layer shapes x 1, 15, 16, 17 and 300 rows (300: past the 256-row padding) cut into crops of 1 / 15 / 16 / 33 rows whose
    inputs cycle through the kinds of the CPU matrix -- all-zero, one-signed, tie and saturated inputs included."""
    K = 512 if layer == 2 else 256
    rng = np.random.default_rng(100 + layer)
    kinds = [k for k in QC.case_kinds() if k != "single_row"]
    n = 0
    for rows in (1, 15, 16, 17, 300):
        segs = _segments(rows)
        xs = [QC.make_case(rng, kinds[(n + i) % len(kinds)], K, T) for i, (_, T) in enumerate(segs)]
        n += len(segs)
        out, codes, params = rq.qlinear_device(torch.from_numpy(np.concatenate(xs)).cuda(), segs, layer)
        out, codes = out.cpu().numpy(), codes.cpu().numpy()
        for (r0, T), x, p in zip(segs, xs, params):
            want, cd, s, zp = _layer_ref(qseq, layer, x)
            assert (np.float32(p[0]), int(p[1])) == (s, zp), (rows, r0, T, p, s, zp)
            assert np.array_equal(codes[r0:r0 + T], cd), (rows, r0, T)
            assert np.array_equal(out[r0:r0 + T], want), (rows, r0, T, float(np.abs(out[r0:r0 + T] - want).max()))


def test_qlinear_op_refuses_bad_tables_and_other_contexts(rq, readers_trained):
    x = torch.zeros((16, 256), dtype=torch.float32, device="cuda")
    for segs in ([(0, 8)], [(0, 8), (9, 7)], [(0, 17)], [(0, 0), (0, 16)]):
        with pytest.raises(RuntimeError):
            rq.qlinear_device(x, segs, 0)
    with pytest.raises(ValueError):
        rq.qlinear_device(x, [(0, 16)], 5)
    with pytest.raises(ValueError):
        rq.qlinear_device(x.to(torch.float64), [(0, 16)], 0)
    with pytest.raises(RuntimeError):
        readers_trained["exact_rec"].qlinear_device(x, [(0, 16)], 0)           # not a rec_quant context: a status, not a fall-back


# ------------------------------------------------------------------------------------------------ the recurrence
@pytest.mark.parametrize("layer", [0, 1])
def test_qlstm_op_step_by_step_from_the_devices_own_state(rq, qseq, layer):
    """T = 1, 2, 15, 16, 47 mixed in one 16-sequence tile and a 17th sequence in a second tile, both directions.  For every step: the
    parameters and codes of the h that entered it -- read back from the device's previous row, zeros (scale 0.1) at a direction's first step
    -- equal the restatement's exactly, and the restatement's step from the device's (h, c) gives the device's h and c within 2e-6."""
    Ts = [1, 2, 15, 16, 47] * 3 + [47, 15]
    assert len(Ts) == 17
    segs, at = [], 0
    for T in Ts:
        segs.append((at, T))
        at += T
    rng = np.random.default_rng(7 + layer)
    G = (rng.standard_normal((at, 2048)) * 1.5).astype(np.float32)
    h, c, hcodes, hparams = (t.cpu().numpy() for t in rq.qlstm_device(torch.from_numpy(G).cuda(), segs, layer))
    worst = 0.0
    for r0, T in segs:
        for d, p in enumerate(qseq.layers[layer][:2]):
            sl = slice(d * 256, (d + 1) * 256)
            for step in range(T):
                t = T - 1 - step if d else step
                prev = t + 1 if d else t - 1
                hp = h[r0 + prev, sl] if step else np.zeros(256, np.float32)
                cp = c[r0 + prev, sl] if step else np.zeros(256, np.float32)
                h2, c2, _, cd, s, zp = Q.lstm_step(G[r0 + t, d * 1024:(d + 1) * 1024], hp, cp, p.q_hh, p.s_hh, p.b_hh)
                got = hparams[r0 + t, d]
                assert (np.float32(got[0]), int(got[1])) == (s, zp), (r0, T, d, step, got, s, zp)
                if step == 0:
                    assert s == np.float32(0.1) and zp == 0
                assert np.array_equal(hcodes[r0 + t, sl], cd), (r0, T, d, step)
                e = max(float(np.abs(h[r0 + t, sl] - h2).max()), float((np.abs(c[r0 + t, sl] - c2) / np.maximum(1.0, np.abs(c2))).max()))
                worst = max(worst, e)
                assert e <= 2e-6, (r0, T, d, step, e)
    print(f"layer {layer}: {2 * at} steps, largest one-step distance of h / c from the restatement {worst:.2e}")


# ------------------------------------------------------------------------------------------------ the sequence half on real crops
def _device_logits(r, xs, W):
    """bbocr_crnn_logits of an exact-mode reader on crops x [64, W] in [-1, 1] that came from uint8 levels: the codes 1 + level."""
    g = np.rint((np.stack(xs) * 0.5 + 0.5) * 255.0).astype(np.int16) + 1
    dev = torch.from_numpy(g).contiguous().cuda()
    T = W // 4 - 1
    out = torch.zeros((len(xs), T, 112), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r._check(r._lib.bbocr_crnn_logits(r._h, C.c_void_p(dev.data_ptr()), len(xs), W, C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()[:, :, :97]


@pytest.fixture(scope="module")
def crop_refs(oracle_trained, oracle_quant):
    """Per padded width: the crops of the two pages, the quantised CPU model's logits and the fp32 model's (computed once)."""
    by_w = {}
    for img in QC.pages():
        for W, x in QC.page_crops(oracle_trained, img):
            by_w.setdefault(W, []).append(x)
    return {W: (xs, np.stack([QC.logits(oracle_quant.recognizer, x) for x in xs]), np.stack([QC.logits(oracle_trained.recognizer, x) for x in xs]))
            for W, xs in by_w.items()}


def _sequence_half_figures(r, crop_refs):
    sq_q = sq_f = n = steps = excluded = bad = 0
    for W, (xs, want_q, want_f) in sorted(crop_refs.items()):
        got = _device_logits(r, xs, W)
        sq_q += float(((got - want_q) ** 2).sum())
        sq_f += float(((got - want_f) ** 2).sum())
        n += got.size
        decidable = QC.margins(want_q) > QC.ARGMAX_TOL
        steps += decidable.size
        excluded += int((~decidable).sum())
        bad += int(((got.argmax(-1) != want_q.argmax(-1)) & decidable).sum())
    return np.sqrt(sq_q / n), np.sqrt(sq_f / n), steps, excluded, bad


def test_sequence_half_follows_the_quantised_model_not_the_fp32_one(rq, readers_trained, crop_refs):
    """Over all logits of the two pages' crops: rms(device - quantised CPU model) < rms(device - fp32 CPU model), and the arg-max equals the
    quantised model's at every time step whose top-2 margin there exceeds ARGMAX_TOL; the rule excludes at most 1 % of the steps.  The
    exact_rec reader without the switch (the parent's arithmetic) is on the fp32 side of the same comparison."""
    rms_q, rms_f, steps, excluded, bad = _sequence_half_figures(rq, crop_refs)
    print(f"rec_quant: rms(device - quantised) {rms_q:.3e}, rms(device - fp32) {rms_f:.3e}; {steps} steps, {excluded} below the margin "
          f"{QC.ARGMAX_TOL}, {bad} decidable arg-max differences")
    assert rms_q < rms_f
    assert bad == 0
    assert excluded <= QC.MAX_EXCLUDED * steps
    p_q, p_f = _sequence_half_figures(readers_trained["exact_rec"], crop_refs)[:2]
    print(f"exact_rec without the switch: rms(device - quantised) {p_q:.3e}, rms(device - fp32) {p_f:.3e}")
    assert p_f < p_q


# ------------------------------------------------------------------------------------------------ readtext
def _same_box(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def _oracle_boxes(o, img, decoder="greedy", **kw):
    """readtext of the quantised oracle box by box (its own order: horizontal boxes, then free ones): [(result, decidable)] -- decidable: every
    recogniser call made for the box (the contrast retry included) had all its top-2 margins above ARGMAX_TOL."""
    from oracle import imgproc, recog

    _, grey = imgproc.reformat_input(img)
    hori, free = o.detect(img)
    out, calls = [], 0
    for hb, fb in [([b], []) for b in hori] + [([], [b]) for b in free]:
        with LogitTap(o) as tap:
            res = o.recognize(grey, hb, fb, **kw)
        calls += len(tap.calls)
        ok = all(float(QC.margins(lg).min()) > QC.ARGMAX_TOL for lg in tap.calls)
        for box, text, conf in res:
            if decoder == "beamsearch":          # the search over the probabilities of the call that won (the last one whose greedy text is `text`)
                lg = [l for l in tap.calls if recog.predict_from_logits(l)[0][0] == text][-1]
                text = recog.predict_from_logits(lg, decoder="beamsearch", beam_width=5)[0][0]
            out.append(((box, text, conf), ok))
    return out, calls


def _check_texts(got, want, what):
    assert len(got) == len(want), what
    skipped = 0
    for g, ((box, text, _), ok) in zip(got, want):
        assert _same_box(g[0], box), (what, g[0], box)
        if ok:
            assert g[1] == text, (what, g[1], text)
        skipped += not ok
    return skipped


def test_readtext_follows_the_quantised_cpu_reference(rq, readers_trained, oracle_quant):
    """Both pages: the boxes are the exact_rec call's, the texts those of the quantised CPU reference wherever the margin rule holds;
    decoder='beamsearch' on the first page keeps the greedy call's boxes and confidences and finds the reference search's text."""
    skipped = boxes = 0
    for k, img in enumerate(QC.pages()):
        got = rq.readtext(img)
        plain = readers_trained["exact_rec"].readtext(img)
        assert len(got) == len(plain) >= 4 and all(_same_box(g[0], p[0]) for g, p in zip(got, plain))
        want, _ = _oracle_boxes(oracle_quant, img)
        skipped += _check_texts(got, want, f"page {k}")
        boxes += len(got)
        if k == 0:
            beam = rq.readtext(img, decoder="beamsearch", beamWidth=5)
            assert [(b, c) for b, _, c in beam] == [(b, c) for b, _, c in got]
            _check_texts(beam, _oracle_boxes(oracle_quant, img, decoder="beamsearch")[0], "beamsearch")
    print(f"{boxes} boxes, {skipped} left to the margin rule")
    assert skipped <= boxes // 2


def test_readtext_contrast_retry_and_pages_of_two_shapes(rq, oracle_quant):
    """A faint page read with contrast_ths raised so that boxes take the retry: texts as the quantised CPU reference's under the margin rule.
    And readtext_pages over two shapes equals the page-by-page calls bit for bit."""
    from bb_ocr_amd import synth

    faint = synth.page(94_011, width=500, height=250, lines=4, margin=20, line_pitch=38, faint=1.0)[0]
    kw = dict(contrast_ths=0.9)
    got = rq.readtext(faint, **kw)
    want, calls = _oracle_boxes(oracle_quant, faint, **kw)
    assert calls > len(want) > 0, "no box took the contrast retry"
    print("first-pass confidences", [round(c, 3) for _, _, c in rq.readtext(faint, contrast_ths=0.0)], "with the retry", [round(c, 3) for _, _, c in got])
    _check_texts(got, want, "faint page")
    pages = [torch.from_numpy(p).cuda() for p in (QC.pages()[0], faint, QC.pages()[1])]
    single = [rq.readtext_device(p[None])[0] for p in pages]
    assert all(single) and rq.readtext_pages(pages) == single


# ------------------------------------------------------------------------------------------------ the switch and the weight blob
def test_switch_is_refused_outside_the_exact_precisions(states_trained):
    import bb_ocr_amd
    from bb_ocr_amd import _lib

    for prec in ("fp16", "bf16", "mixed"):
        with pytest.raises(ValueError):
            bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, precision=prec, rec_quant=True)
    lib = _lib.load()
    for prec, flag, ok in ((1, 1, False), (0, 1, False), (3, 1, False), (4, 2, False), (4, -1, False), (2, 1, True), (4, 1, True), (1, 0, True)):
        h = C.c_void_p()
        rc = lib.bbocr_create(C.byref(_lib.bbocr_config(device=torch.cuda.current_device(), precision=prec, rec_quant=flag)), C.byref(h))
        assert (rc == 0) == ok and (ok or rc == -1), (prec, flag, rc)         # BBOCR_ERR_ARG
        if h:
            lib.bbocr_destroy(h)


def test_blob_of_the_other_kind_is_refused(rq, readers_trained):
    plain = readers_trained["exact_rec"]
    for src, dst in ((plain, rq), (rq, plain)):
        blob = src.export_weights_blob()
        rc = dst._lib.bbocr_weights_import(dst._h, C.c_void_p(blob.data_ptr()), blob.numel())
        assert rc == -3, rc                                                    # BBOCR_ERR_WEIGHTS
    blob = rq.export_weights_blob()                                            # and its own kind round-trips
    rq.import_weights_blob(blob)


def test_switch_off_is_the_exact_rec_path_bit_for_bit(states_trained, readers_trained):
    import bb_ocr_amd

    img = QC.pages()[0]
    off = bb_ocr_amd.Reader(["en"], gpu=True, weights=states_trained, precision="exact_rec", rec_quant=False)
    try:
        assert off.readtext(img) == readers_trained["exact_rec"].readtext(img)
    finally:
        off.close()
