"""GPU: recognisers of more than 128 classes (bbocr_config::rec_classes) -- the unfused Prediction launch, ctc_rows_wide_kernel, the fused
pred_ctc_kernel, and readtext of wide Readers against the English one.  References and allowances: tests/wide_ctc_ref.py (checked on
stand-ins by test_wide_classes_cpu.py).  Every figure is printed before it is asserted.

Inputs (the same for every test of one width and element type, computed once): Prediction weights uniform(+-1/16) * 4 and inputs
uniform(+-1), rounded to the element type, seed 7; 2,048 rows, of which the launches take the first 1, 255, 256 or all.  Two weight rows are
copies of one another in different 16-class fragments (classes 3 and C - 2, bias -3 so that they rarely lead an ordinary row) and four input
rows are 0.375 sign(w[3]): there the two logits are bitwise equal and the largest of the row, and the lower class must win.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import wide_ctc_ref as W

pytestmark = pytest.mark.gpu

WIDTHS = (129, 352, 1009, 6719)
ROWS = (1, 255, 256, 2048)
ELS = ("fp16", "bf16")
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
TIE_A, TIE_ROWS = 3, (5, 250, 300, 2040)
ERR_ARG, ERR_WEIGHTS = -1, -3


def _round(a, el):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[el]).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def operands(el, Cn):
    """-> (x [2048, 256], w [C, 256], b [C]) float32 arrays of element-type values, and their float64 logits"""
    rng = np.random.default_rng(7)
    w = _round(rng.uniform(-1 / 16, 1 / 16, (Cn, 256)) * 4, el)
    b = rng.uniform(-0.5, 0.5, Cn).astype(np.float32)
    x = _round(rng.uniform(-1, 1, (2048, 256)), el)
    w[Cn - 2] = w[TIE_A]
    b[TIE_A] = b[Cn - 2] = -3.0
    for r in TIE_ROWS:
        x[r] = np.where(w[TIE_A] >= 0, 0.375, -0.375)          # logit 0.375 * sum |w| - 3 = 9: above every ordinary logit, and max |ref| stays its size
    l64 = W.logits64(x, w, b)
    return x, w, b, l64


_CTX = {}


def wide_reader(el, Cn, state=None, **kw):
    """a recogniser-only Reader of C classes (any character table: the stage tests read class indices), kept for the module"""
    import bb_ocr_amd
    from bb_ocr_amd import weights

    key = (el, Cn)
    if state is None and key in _CTX:
        return _CTX[key]
    chars = [chr(0x4E00 + k) for k in range(Cn - 1)]
    if state is None:
        _, w, b, _ = operands(el, Cn)
        state = dict(weights.synthetic_crnn_state(0, num_class=Cn))
        state["Prediction.weight"], state["Prediction.bias"] = w, b
    r = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=(None, state), detector=False, precision=el, **kw)
    if not kw:
        _CTX[key] = r
    return r


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for r in _CTX.values():
        r.close()
    _CTX.clear()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _masks(Cn, l64):
    """None; bits in words 0, 4, 127 (where the width has them) and the last; a mask that removes row 0's arg-max and the lower tie class"""
    spread = sorted({5, 128, Cn - 1} | ({4095} if Cn > 4095 else set()))
    top0 = int(l64[0].argmax())
    return [("none", None), ("spread", W.mask_words(spread, Cn)), ("argmax", W.mask_words(sorted({top0 if top0 else 1, TIE_A}), Cn))]


# ------------------------------------------------------------------------------------------------ logits, unfused route
@pytest.mark.parametrize("el", ELS)
@pytest.mark.parametrize("Cn", WIDTHS)
def test_unfused_logits(el, Cn):
    x, w, b, l64 = operands(el, Cn)
    r = wide_reader(el, Cn)
    cs = (Cn + 15) // 16 * 16
    L = W.logit_bound(l64)
    xd = _dev(x, DT[el])
    for rows in ROWS:                                          # one row, a padded last tile, one full tile, eight
        out = torch.full((rows * cs + 1,), -7.0, dtype=torch.float32, device="cuda")
        r._check(r._lib.bbocr_op_pred(r._h, C.c_void_p(xd.data_ptr()), rows, C.c_void_p(out.data_ptr())))
        got = out.cpu().numpy()
        assert got[-1] == -7.0, "the element behind the logits was written"
        got = got[:-1].reshape(rows, cs)
        err = float(np.abs(got[:, :Cn].astype(np.float64) - l64[:rows]).max())
        print(f"unfused logits {el} C={Cn} rows={rows}: max |err| {err:.3e}, allowance {L:.3e}")
        assert err <= L
        assert (got[:, Cn:] == 0).all(), "the columns behind the classes belong to no class: the plan's zero weights and bias leave 0 there"


# ------------------------------------------------------------------------------------------------ probabilities, wide rows kernel
def _rows_case(Cn, seed):
    """logits [301, cs] with cs two 16-column groups past C (so that every width has padded columns), ragged sequences tiling the rows"""
    rng = np.random.default_rng(seed)
    rows, cs = 301, (Cn + 15) // 16 * 16 + 16
    x = rng.normal(0.0, 1.3, (rows, cs)).astype(np.float32)
    x[:, Cn:] = rng.normal(0.0, 1.3, (rows, cs - Cn)).astype(np.float32)
    x[1, 7] = -np.inf                                          # a -inf logit: probability exactly 0, nothing else disturbed
    x[2, Cn - 1] = 11.0                                        # the maximum in the last class
    x[3, Cn] = 300.0                                           # the row's largest VALUE sits behind C: it must not take part (expf would overflow)
    x[4, 9] = x[4, Cn - 2] = 8.0                               # equal maxima 64-class steps apart: the lower class
    seqs, at = [], 0
    for T in (1, 64, 65, 100, 71):
        seqs.append((at, T))
        at += T
    assert at == rows
    return x, cs, seqs


@pytest.mark.parametrize("Cn", WIDTHS)
def test_wide_rows_kernel(Cn):
    r = wide_reader("fp16", Cn)
    x, cs, seqs = _rows_case(Cn, 11 + Cn)
    rows, n = len(x), len(seqs)
    top2 = int(x[2, :Cn].argmax())
    masks = [("none", None), ("spread", W.mask_words(sorted({5, 128, Cn - 1} | ({4095} if Cn > 4095 else set())), Cn)),
             ("argmax", W.mask_words([top2], Cn))]
    xd = _dev(x)
    tab = (C.c_int * (2 * n))(*[v for s in seqs for v in s])
    for name, mask in masks:
        probs = torch.full((rows * cs + 1,), W.S_PROB, dtype=torch.float32, device="cuda")
        idx = torch.full((rows + 1,), W.S_IDX, dtype=torch.int32, device="cuda")
        pmax = torch.full((rows + 1,), W.S_PMAX, dtype=torch.float32, device="cuda")
        oidx = torch.full((rows + 1,), W.S_OUT, dtype=torch.int32, device="cuda")
        cout = torch.full((n + 1, 4), W.S_CTC, dtype=torch.int32, device="cuda")
        mw = None if mask is None else (C.c_uint * len(mask))(*mask)
        r._check(r._lib.bbocr_op_ctc_rows(r._h, C.c_void_p(xd.data_ptr()), rows, Cn, cs, mw, tab, n, C.c_void_p(probs.data_ptr()),
                                          C.c_void_p(idx.data_ptr()), C.c_void_p(pmax.data_ptr()), C.c_void_p(oidx.data_ptr()), C.c_void_p(cout.data_ptr())))
        p = probs.cpu().numpy()
        assert p[-1] == np.float32(W.S_PROB) and idx[-1].item() == W.S_IDX and pmax[-1].item() == W.S_PMAX and oidx[-1].item() == W.S_OUT
        p = p[:-1].reshape(rows, cs)
        worst = W.check_probs(f"C={Cn}/{name}", x, Cn, mask, p)
        print(f"wide rows kernel C={Cn} mask={name}: worst |err| / allowance {worst:.3f} (K = {W.k_wide(Cn):.1f})")
        case = types.SimpleNamespace(name=f"C={Cn}/{name}", C=Cn, logits=x, seqs=seqs, expect_idx=None, expect_text=None)
        W.check_exact(case, p, idx.cpu().numpy()[:-1], pmax.cpu().numpy()[:-1], oidx.cpu().numpy()[:-1], cout.cpu().numpy())
        got = idx.cpu().numpy()
        if name == "none":
            assert got[2] == Cn - 1 and got[4] == 9 and p[1, 7] == 0.0
        if name == "argmax":
            assert got[2] != top2
    # the probabilities may be left out (the greedy route): idx and pmax are the same bits
    idx2 = torch.full((rows,), W.S_IDX, dtype=torch.int32, device="cuda")
    pmax2 = torch.full((rows,), W.S_PMAX, dtype=torch.float32, device="cuda")
    r._check(r._lib.bbocr_op_ctc_rows(r._h, C.c_void_p(xd.data_ptr()), rows, Cn, cs, mw, tab, n, None, C.c_void_p(idx2.data_ptr()),
                                      C.c_void_p(pmax2.data_ptr()), C.c_void_p(oidx.data_ptr()), C.c_void_p(cout.data_ptr())))
    assert torch.equal(idx2, idx[:-1]) and torch.equal(pmax2.view(torch.int32), pmax[:-1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ the fused kernel
@pytest.mark.parametrize("el", ELS)
@pytest.mark.parametrize("Cn", WIDTHS)
def test_fused_kernel(el, Cn):
    x, w, b, l64 = operands(el, Cn)
    r = wide_reader(el, Cn)
    L = W.logit_bound(l64)
    xd = _dev(x, DT[el])
    expect = np.full(2048, -1)
    expect[list(TIE_ROWS)] = TIE_A
    for name, mask in _masks(Cn, l64):
        want_tie = expect.copy()
        if mask is not None and W.mask_bits(mask, Cn)[TIE_A]:
            want_tie[list(TIE_ROWS)] = Cn - 2                  # the lower tie class is gone: its copy leads
        md = None if mask is None else _dev(np.array(mask, dtype=np.uint32).view(np.int32))
        for rows in ROWS:
            idx = torch.full((rows + 1,), W.S_IDX, dtype=torch.int32, device="cuda")
            pmax = torch.full((rows + 1,), W.S_PMAX, dtype=torch.float32, device="cuda")
            r._check(r._lib.bbocr_op_pred_ctc(r._h, C.c_void_p(xd.data_ptr()), rows, None if md is None else C.c_void_p(md.data_ptr()),
                                              0 if mask is None else (Cn + 31) // 32, C.c_void_p(idx.data_ptr()), C.c_void_p(pmax.data_ptr())))
            gi, gp = idx.cpu().numpy(), pmax.cpu().numpy()
            assert gi[-1] == W.S_IDX and gp[-1] == np.float32(W.S_PMAX), "an element behind the outputs was written"
            share = W.check_fused(f"{el}/C={Cn}/{name}/rows={rows}", l64[:rows], Cn, mask, gi[:-1], gp[:-1], L, want_tie[:rows])
            print(f"fused {el} C={Cn} mask={name} rows={rows}: {share * 100:.3f} % of the rows below the margin 2 L = {2 * L:.2e}")
            if rows == 2048:
                assert share <= 0.01                           # the reference alone leaves out 0 .. 0.25 % (test_wide_classes_cpu.py) + the 4 tie rows


# ------------------------------------------------------------------------------------------------ end to end
def _wide_model(states_trained, Cn, seed=5):
    """the trained 97-class recogniser scattered into Cn classes by an injective map (blank stays 0): every other class has zero weights and
    bias -30; the character table has the English characters at the mapped positions"""
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


@pytest.fixture(scope="module")
def pages():
    from bb_ocr_amd import synth

    return [synth.page(4100 + i, width=640, height=384, lines=4 + i, margin=24)[0] for i in range(2)]


def _same(name, got, want, rel):
    assert [g[0] for g in got] == [w[0] for w in want], f"{name}: boxes differ"
    assert [g[1] for g in got] == [w[1] for w in want], f"{name}: strings differ: {[g[1] for g in got]} / {[w[1] for w in want]}"
    d = max([abs(g[2] - w[2]) / max(abs(w[2]), 1e-30) for g, w in zip(got, want)] + [0.0])
    print(f"{name}: {len(got)} boxes, largest relative confidence difference {d:.3e} (bound {rel:.1e})")
    assert d <= rel, name
    return d


@pytest.mark.parametrize("Cn", [1009, 6719])
def test_readtext_equals_the_english_reader(Cn, states_trained, readers_trained, pages):
    import bb_ocr_amd

    states, chars = _wide_model(states_trained, Cn)
    wide = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states, precision="fp16")
    try:
        en = readers_trained["fp16"]
        assert en._lib.bbocr_set_class_mask(en._h, None, 0) == ERR_ARG               # at most 128 classes: bbocr_params::ignore_mask rules
        for k, img in enumerate(pages):
            want = en.readtext(img)
            assert len(want) >= 4 and any(t for _, t, _ in want)
            assert en.last_ctc_route() == 0                    # CTC_GREEDY
            _same(f"C={Cn} page {k} greedy (fused route)", wide.readtext(img), want, 1e-6)
            assert wide.last_ctc_route() == 3, "a greedy fp16 pass over more than 128 classes must run pred_ctc_kernel (CTC_GREEDY_FUSED)"
            # (the route is the record of the thread's LAST call, like the stage times: read it before the next call)
            beam_en = en.readtext(img, decoder="beamsearch", beamWidth=5)
            assert en.last_ctc_route() == 2                    # device search at 97 classes
            beam_wide = wide.readtext(img, decoder="beamsearch", beamWidth=5)
            assert wide.last_ctc_route() == 1                  # host search beyond 128
            _same(f"C={Cn} page {k} beamsearch (host)", beam_wide, beam_en, 1e-6)
            digits = wide.readtext(img, allowlist="0123456789")
            assert wide.last_ctc_route() == 3
            _same(f"C={Cn} page {k} allowlist", digits, en.readtext(img, allowlist="0123456789"), 1e-6)
            assert all(set(t) <= set("0123456789") for _, t, _ in digits)
        # blob: export -> import between two wide contexts reproduces the results; a 97-class blob is refused
        blob = wide.export_weights_blob()
        twin = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights="empty", precision="fp16")
        try:
            twin.import_weights_blob(blob)
            assert twin.readtext(pages[0]) == wide.readtext(pages[0])
            small = en.export_weights_blob()
            rc = twin._lib.bbocr_weights_import(twin._h, C.c_void_p(small.data_ptr()), small.numel())
            assert rc == ERR_WEIGHTS, rc
            assert b"97" in twin._lib.bbocr_last_error(twin._h) and str(Cn).encode() in twin._lib.bbocr_last_error(twin._h)
        finally:
            twin.close()
    finally:
        wide.close()


@pytest.mark.parametrize("Cn", [1009, 6719])
def test_readtext_exact_rec_unfused_route(Cn, states_trained, readers_trained, pages):
    import bb_ocr_amd

    states, chars = _wide_model(states_trained, Cn)
    wide = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states, precision="exact_rec")
    try:
        en = readers_trained["exact_rec"]
        for k, img in enumerate(pages):
            want = en.readtext(img)
            got = wide.readtext(img)
            assert wide.last_ctc_route() == 0                  # CTC_GREEDY: Prediction through the split plan, ctc_rows_wide_kernel
            _same(f"C={Cn} page {k} exact_rec (unfused route)", got, want, 1e-6)
    finally:
        wide.close()


def test_class_count_of_the_state_dict_and_the_mask_entry_point(states_trained):
    import bb_ocr_amd

    states, chars = _wide_model(states_trained, 1009)
    with pytest.raises(RuntimeError, match="1009.*97|97.*1009"):        # english_g2's Prediction into a 1,009-class context: both numbers named
        bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states_trained, detector=False, precision="fp16")
    with pytest.raises(ValueError, match="rec_quant"):
        bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=states, detector=False, rec_quant=True)
    r = wide_reader("fp16", 129)
    lib, h = r._lib, r._h
    words = (C.c_uint32 * 5)(0, 0, 0, 0, 0)
    assert lib.bbocr_set_class_mask(h, words, 5) == 0 and lib.bbocr_set_class_mask(h, words, 6) == ERR_ARG
    words[0] = 1
    assert lib.bbocr_set_class_mask(h, words, 5) == ERR_ARG                          # the blank
    words[0], words[4] = 0, 2
    assert lib.bbocr_set_class_mask(h, words, 5) == ERR_ARG                          # class 129 of 129
    words[4] = 1
    assert lib.bbocr_set_class_mask(h, words, 5) == 0 and lib.bbocr_set_class_mask(h, None, 0) == 0
