"""CPU: recognisers of more than 128 classes -- the numpy references and checks of tests/wide_ctc_ref.py before they judge a kernel
(test_gpu_wide_classes.py), the Reader's handling of a custom model's yaml / character list / mask / text table, and the context's
validation of the class count.  Nothing here creates a context."""
import ctypes as C
import os

import numpy as np
import pytest

import ctc_greedy_cases as K
import ctc_greedy_ref as G
import wide_ctc_ref as W

F = np.float32


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_the_narrow_one_up_to_128_classes():
    seen = 0
    for case in K.CASES:
        if case.C > 128:
            continue
        mask = case.mask
        assert np.array_equal(W.probs64(case.logits, case.C, mask), G.probs64(case.logits, case.C, mask))
        assert np.array_equal(W.prob_bound(case.logits, case.C, mask), G.prob_bound(case.logits, case.C, mask)), case.name
        seen += 1
    assert seen >= 10
    assert W.k_wide(128) == G.K and W.k_wide(97) == G.K
    assert W.mask_words([1, 33, 127], 128) == G.mask_words([1, 33, 127])
    # beyond: the constant follows the walk -- ceil(C / 64) + ln C + 12.14, continuous with 19 at the old limit
    assert abs(W.k_wide(129) - (3 + np.log(129) + 12.14)) < 1e-12 and 19.9 < W.k_wide(129) < 20.1
    assert 125.5 < W.k_wide(6719) < 126.5
    assert len(W.mask_words([6718], 6719)) == 210 and W.mask_words([6718], 6719)[209] == 1 << (6718 & 31)


def _rows(C, cs, rows=48, seed=3):
    rng = np.random.default_rng(seed)
    x = np.full((rows, cs), 55.0, dtype=np.float32)           # a value no class ever reaches: a kernel that reads the padding shows it
    x[:, :C] = rng.normal(0.0, 1.3, (rows, C)).astype(np.float32)
    return x


def test_a_float32_evaluation_in_another_order_stays_inside_the_bound():
    import torch

    for C in (129, 352, 1009, 6719):
        x = _rows(C, (C + 15) // 16 * 16)
        for mask in (None, W.mask_words([1, 130 if C > 130 else 5, C - 1], C)):
            p = torch.softmax(torch.from_numpy(x[:, :C]), dim=1).numpy()
            p[:, W.mask_bits(mask, C)] = 0
            p = (p / p.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
            probs = np.full(x.shape, W.S_PROB, np.float32)
            probs[:, :C] = p
            assert W.check_probs(f"torch/{C}", x, C, mask, probs) < 1.0
            sp, si, spm = W.rows_standin(x, C, mask)
            assert W.check_probs(f"standin/{C}", x, C, mask, sp) < 1.0


@pytest.mark.parametrize("C", [129, 1009, 6719])
def test_planted_defects_are_caught_rows_kernel(C):
    """each defect, on an input where it matters, is rejected by check_probs or by ctc_greedy_ref.check_exact's arg-max statement"""
    cs = (C + 15) // 16 * 16
    x = _rows(C, cs)
    x[0, C - 1] = 9.0                                         # the maximum sits in the last class (the last 64-class step)
    mask = W.mask_words([128, min(4095, C - 2), C - 1], C)

    def rejected(defect, m=mask, xx=x):
        probs, idx, pmax = W.rows_standin(xx, C, m, defect)
        try:
            W.check_probs("planted", xx, C, m, probs)
            assert np.array_equal(idx, probs[:, :C].argmax(axis=1)), "idx is not the first-index arg-max of the row"
        except AssertionError:
            return True
        return False

    assert not rejected(None)
    assert rejected("padded")                                 # the 55.0 behind C enters the softmax (and is written)
    for bit in (128, min(4095, C - 2), C - 1):
        assert rejected(("drop_bit", bit)), bit
    assert rejected("sum_masked")
    big = x.copy()
    big[0, C - 1] = 120.0                                     # a softmax is shift-invariant: a missed maximum shows once expf(120 - 4) overflows
    assert not rejected(None, m=None, xx=big) and rejected("last_tile", m=None, xx=big)
    tie = x.copy()
    tie[:, 7] = tie[:, C - 3] = 8.0                           # two equal maxima in different 64-class steps
    assert not rejected(None, m=None, xx=tie) and rejected("tie_high", m=None, xx=tie)


@pytest.mark.parametrize("C", [129, 1009, 6719])
def test_planted_defects_are_caught_fused_kernel(C):
    cs = (C + 15) // 16 * 16
    x = _rows(C, cs)
    x[0, C - 1] = 9.0
    bits = [128, min(4095, C - 2), C - 1]
    L = W.logit_bound(x[:, :C].astype(np.float64))

    def rejected(defect, m, xx, expect=None):
        idx, pmax = W.fused_standin(xx, C, m, defect)
        try:
            W.check_fused("planted", xx[:, :C].astype(np.float64), C, m, idx, pmax, L, expect)
        except AssertionError:
            return True
        return False

    mask = W.mask_words(bits, C)
    assert not rejected(None, mask, x) and not rejected(None, None, x)
    assert rejected("padded", None, x)
    for bit in bits:                                          # the dropped bit must matter: make that class the row's maximum
        xb = x.copy()
        xb[1, bit] = 9.0
        assert not rejected(None, mask, xb) and rejected(("drop_bit", bit), mask, xb), bit
    heavy = x.copy()
    heavy[:, 128] = 6.0                                       # a masked class that carries most of the mass: summing it shows in pmax
    assert not rejected(None, mask, heavy) and rejected("sum_masked", mask, heavy)
    assert rejected("last_tile", None, x)
    tie = x.copy()
    tie[:, 7] = tie[:, C - 3] = 8.0
    lower = np.full(len(tie), 7)
    lower[0] = -1                                             # (row 0 keeps its 9.0 in the last class)
    assert not rejected(None, None, tie, lower) and rejected("tie_high", None, tie, lower)
    # the share of rows left out is a figure of the INPUTS: the reference alone, on the GPU test's distribution
    rng = np.random.default_rng(7)
    w = (rng.uniform(-1 / 16, 1 / 16, (C, 256)) * 4).astype(np.float16)
    xin = rng.uniform(-1, 1, (2048, 256)).astype(np.float16)
    l64 = W.logits64(xin, w, np.zeros(C))
    _, _, margin = W.fused_ref(l64, C)
    assert float((margin <= 2 * W.logit_bound(l64)).mean()) <= 0.0025


# ------------------------------------------------------------------------------------------------ Reader plumbing without a context
def _yaml(tmp_path, name, **over):
    import yaml

    cfg = {"network_params": {"input_channel": 1, "output_channel": 256, "hidden_size": 256}, "imgH": 64, "lang_list": ["th"],
           "character_list": "0123456789กขค€"}
    cfg.update(over)
    (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(cfg, allow_unicode=True), encoding="utf8")


def test_custom_network_yaml(tmp_path):
    from bb_ocr_amd.reader import CHARACTER, resolve_recog_network

    _yaml(tmp_path, "thai")
    net = resolve_recog_network(["th"], "thai", model_storage_directory=str(tmp_path / "m"), user_network_directory=str(tmp_path))
    assert net["character"] == ["[blank]"] + list("0123456789กขค€") and net["lang_char"] == list("0123456789กขค€")
    assert net["model_path"] == str(tmp_path / "m" / "thai.pth") and net["lang_list"] == ["th"]
    assert resolve_recog_network(["th"], "thai", None, str(tmp_path), lang_char="012")["lang_char"] == ["0", "1", "2"]
    _yaml(tmp_path, "gen1", network_params={"input_channel": 1, "output_channel": 512, "hidden_size": 512})
    with pytest.raises(ValueError, match="network_params"):
        resolve_recog_network(["th"], "gen1", None, str(tmp_path))
    _yaml(tmp_path, "tall", imgH=32)
    with pytest.raises(ValueError, match="imgH"):
        resolve_recog_network(["th"], "tall", None, str(tmp_path))
    with pytest.raises(FileNotFoundError):
        resolve_recog_network(["th"], "absent", None, str(tmp_path))
    # the standard network is english_g2: another language names the argument that would change that
    with pytest.raises(ValueError, match="recog_network"):
        resolve_recog_network(["ch_sim"], "standard")
    assert resolve_recog_network(["en"], "standard")["character"] == CHARACTER
    # character= stands in for the yaml: a string or a list of class strings
    net = resolve_recog_network(["xx"], "standard", character="ab€")
    assert net["character"] == ["[blank]", "a", "b", "€"] and net["lang_char"] == ["a", "b", "€"]
    assert resolve_recog_network(["xx"], "standard", character=["a", "bc"])["character"] == ["[blank]", "a", "bc"]
    with pytest.raises(ValueError, match="classes"):
        resolve_recog_network(["xx"], "standard", character=["x"] * 8192)


def test_mask_builder_any_width():
    from bb_ocr_amd.reader import CHARACTER, CHARSET, ignore_mask

    assert ignore_mask(CHARACTER, list(CHARSET)) == [0, 0, 0, 0]                      # english_g2: the four words of bbocr_params
    chars = ["[blank]"] + [chr(0x4E00 + i) for i in range(6718)]
    assert len(ignore_mask(chars, chars[1:])) == 210 and not any(ignore_mask(chars, chars[1:]))
    allow = ignore_mask(chars, chars[1:], allowlist=chars[1] + chars[6718])
    bits = W.mask_bits(allow, 6719)
    assert not bits[0] and not bits[1] and not bits[6718] and bits[2:6718].all()
    block = ignore_mask(chars, chars[1:], blocklist=chars[128] + chars[4095])
    assert np.flatnonzero(W.mask_bits(block, 6719)).tolist() == [128, 4095]
    lang = ignore_mask(chars, chars[1:200])
    assert np.flatnonzero(~W.mask_bits(lang, 6719)).tolist() == list(range(200))
    assert tuple(block) == W.mask_words([128, 4095], 6719)


def test_text_table():
    from bb_ocr_amd.reader import decode_text, text_table

    chars = ["[blank]", "a", "€", "中", "\U0001F600", "z"]                              # a non-BMP code point among them
    tab = text_table(chars)
    assert isinstance(tab, np.ndarray) and tab.dtype == np.dtype("<u4")
    idx = np.array([1, 4, 3, 2, 5, 4], dtype=np.int32)
    assert decode_text(tab, idx, [0, 2, 2, 6]) == ["a\U0001F600", "", "中€z\U0001F600"]
    assert decode_text(tab, idx[:0], [0, 0]) == [""]
    multi = ["[blank]", "a", "क्ष", "é"]                                        # classes of several code points: the joined fallback
    tab = text_table(multi)
    assert isinstance(tab, list)
    assert decode_text(tab, np.array([2, 1, 3], dtype=np.int32), [0, 1, 3]) == ["क्ष", "aé"]


def test_synthetic_state_class_count():
    from bb_ocr_amd import weights

    a, b = weights.synthetic_crnn_state(0), weights.synthetic_crnn_state(0, num_class=352)
    assert a["Prediction.weight"].shape == (97, 256) and b["Prediction.weight"].shape == (352, 256) and b["Prediction.bias"].shape == (352,)
    assert all(np.array_equal(a[k], b[k]) for k in a if not k.startswith("Prediction."))
    assert np.array_equal(a["Prediction.weight"], weights.synthetic_crnn_state(0, num_class=97)["Prediction.weight"])


# ------------------------------------------------------------------------------------------------ the context's validation
def test_create_refuses_bad_class_counts():
    """refused before anything touches a device, like an unknown precision"""
    from bb_ocr_amd import _lib

    lib = _lib.load()
    assert _lib.REC_CLASSES_MAX == 8192
    exact_rec = _lib.PRECISIONS["exact_rec"]
    # rec_quant goes with english_g2's 97 classes alone: wide counts, and the narrow ones whose logits stride would be 64, 80, 112 or 128 columns
    for kw in ({"rec_classes": 1}, {"rec_classes": 8193}, {"rec_classes": -5}, {"rec_classes": 129, "rec_quant": 1, "precision": exact_rec},
               {"rec_classes": 6719, "rec_quant": 1, "precision": exact_rec}, {"rec_classes": 120, "rec_quant": 1, "precision": exact_rec},
               {"rec_classes": 64, "rec_quant": 1, "precision": exact_rec}, {"rec_classes": 70, "rec_quant": 1, "precision": exact_rec},
               {"rec_classes": 98, "rec_quant": 1, "precision": exact_rec}):
        h = C.c_void_p()
        cfg = _lib.bbocr_config(device=0, **kw)
        assert lib.bbocr_create(C.byref(cfg), C.byref(h)) == -1 and not h.value, kw
    assert lib.bbocr_set_class_mask(None, None, 0) == -1 and lib.bbocr_last_ctc_route(None, None) == -1
    # the Reader names the pair before it asks for a device or a context
    import bb_ocr_amd

    for chars in ("a" * 119, "a" * 63, [chr(0x4E00 + k) for k in range(351)]):
        with pytest.raises(ValueError, match="rec_quant.*97"):
            bb_ocr_amd.Reader(["xx"], character=chars, rec_quant=True, weights="empty")
    assert C.sizeof(_lib.bbocr_config) == 32                                         # the field took the reserved word: the layout stands
