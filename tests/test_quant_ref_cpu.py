"""tests/quant_ref.py -- the numpy statement of the rec_quant arithmetic -- pinned to torch's own dynamic int8 modules on the CPU (no GPU
needed).  What must be exact is exact: weights, scales, activation parameters, codes and the fp32 output of a quantised product, bit for
bit; what passes through exp / tanh is bounded by the fp32 precision of those (2e-6 on values within [-1, 1]); whole sequences are MEASURED
(a last-bit difference in a non-linearity moves a 7-bit code of h by one level now and then), and those figures are the yardsticks of
tests/test_gpu_rec_quant.py."""
import warnings

import numpy as np
import pytest
import torch

import quant_cases as QC
import quant_ref as Q

pytestmark = pytest.mark.skipif(not QC.quant_engine_ok(), reason="torch reports no fbgemm / x86 quantised engine")

N_CASES = 2048


@pytest.fixture(scope="module")
def crnn(oracle_trained):
    return oracle_trained.recognizer


@pytest.fixture(scope="module")
def qcrnn(crnn):
    return QC.quantize_dynamic(crnn)


@pytest.fixture(scope="module")
def qseq(crnn):
    return Q.QSequence(QC.state_numpy(crnn))


def _dyn_linear(w, b):
    lin = torch.nn.Linear(w.shape[1], w.shape[0])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w))
        lin.bias.copy_(torch.from_numpy(b))
    return QC.quantize_dynamic(torch.nn.Sequential(lin))[0]


def test_weights_and_scales_equal_the_observers(crnn, qcrnn, qseq):
    """All eleven tensors: int8 codes and scale equal what quantize_dynamic left in the modules."""
    seen = 0
    for l in range(2):
        rnn = qcrnn.SequenceModeling[l].rnn
        tw = rnn.get_weight()
        fwd, bwd, ql, sl, _ = qseq.layers[l]
        for sfx, d in (("", fwd), ("_reverse", bwd)):
            for name, q, s in (("weight_ih_l0", d.q_ih, d.s_ih), ("weight_hh_l0", d.q_hh, d.s_hh)):
                t = tw[name + sfx]
                assert t.qscheme() == torch.per_tensor_affine and t.q_zero_point() == 0
                assert np.float32(t.q_scale()) == s and np.array_equal(t.int_repr().numpy(), q), (l, name + sfx)
                seen += 1
        t = qcrnn.SequenceModeling[l].linear.weight()
        assert np.float32(t.q_scale()) == sl and np.array_equal(t.int_repr().numpy(), ql)
        seen += 1
    t = qcrnn.Prediction.weight()
    assert np.float32(t.q_scale()) == qseq.s_pred and np.array_equal(t.int_repr().numpy(), qseq.q_pred)
    assert seen + 1 == 11


@pytest.fixture(scope="module")
def matrix():
    return QC.case_matrix(2024, N_CASES, 256)


def test_qlinear_equals_torch_bit_for_bit(qcrnn, qseq, matrix):
    """Prediction (256 -> 97) on every case of the matrix: all-zero, one-signed, single-row, tie and zero-point-0 / 127 inputs included."""
    kinds, zps = set(), set()
    for kind, x in matrix:
        with torch.no_grad():
            want = qcrnn.Prediction(torch.from_numpy(x)).numpy()
        got, _, _, zp = Q.qlinear(x, qseq.q_pred, qseq.s_pred, qseq.b_pred)
        assert np.array_equal(got, want), (kind, x.shape, float(np.abs(got - want).max()))
        kinds.add(kind)
        zps.add(zp)
    assert kinds == set(QC.case_kinds()) and {0, 127} <= zps and len(matrix) >= 2000


def test_the_rejected_roundings_differ_on_the_matrix(qcrnn, qseq, matrix):
    """Keeps the matrix honest: an unfused x * inv + zp, rounding before the zero point is added, and x / scale each miss torch somewhere."""
    bad = {"unfused": 0, "round_first": 0, "divide": 0}
    fns = {"unfused": Q.codes_unfused, "round_first": Q.codes_round_first, "divide": Q.codes_divide}
    for kind, x in matrix[:512]:
        with torch.no_grad():
            want = qcrnn.Prediction(torch.from_numpy(x)).numpy()
        for name, fn in fns.items():
            bad[name] += not np.array_equal(Q.qlinear(x, qseq.q_pred, qseq.s_pred, qseq.b_pred, code_fn=fn)[0], want)
    print("cases of 512 on which a rejected variant differs from torch:", bad)
    assert all(v > 0 for v in bad.values()), bad


def test_one_lstm_step(crnn, qseq):
    """From a given (G[t], h, c): the pre-activation gates equal G[t] + torch's own dynamic Linear(W_hh, b_hh) applied to h bit for bit
    (step 0's h = 0, which takes the scale-0.1 branch, included); h and c are within 2e-6 of torch's sigmoid / tanh on those gates."""
    rng = np.random.default_rng(5)
    sd = QC.state_numpy(crnn)
    d = qseq.layers[0][0]
    lin = _dyn_linear(sd["SequenceModeling.0.rnn.weight_hh_l0"], sd["SequenceModeling.0.rnn.bias_hh_l0"])
    for it in range(64):
        h = np.zeros(256, np.float32) if it == 0 else np.tanh(rng.standard_normal(256) * rng.uniform(0.05, 2)).astype(np.float32)
        if it % 5 == 1:
            h = np.abs(h)
        c = (rng.standard_normal(256) * 0.7).astype(np.float32)
        g_t = (rng.standard_normal(1024) * 2).astype(np.float32)
        h2, c2, gates, _, scale, zp = Q.lstm_step(g_t, h, c, d.q_hh, d.s_hh, d.b_hh)
        if it == 0:
            assert scale == np.float32(0.1) and zp == 0
        with torch.no_grad():
            want = torch.from_numpy(g_t) + lin(torch.from_numpy(h[None]))[0]
            assert np.array_equal(gates, want.numpy()), it
            i, f, g, o = want.chunk(4)
            cw = torch.sigmoid(f) * torch.from_numpy(c) + torch.sigmoid(i) * torch.tanh(g)
            hw = torch.sigmoid(o) * torch.tanh(cw)
        assert np.abs(c2 - cw.numpy()).max() <= 2e-6 * max(1.0, float(np.abs(cw.numpy()).max())) and np.abs(h2 - hw.numpy()).max() <= 2e-6


def test_whole_sequences_distance_to_torch(crnn, qcrnn, qseq):
    """Measured, the yardsticks: how far the restatement is from torch's DynamicQuantizedLSTM over whole sequences (T = 15, 40, 160), and
    how far the fp32 LSTM is.  The first must be the smaller by far: the restatement follows the quantised module, not the fp32 one."""
    rng = np.random.default_rng(9)
    fwd, bwd = qseq.layers[0][:2]
    for T in (15, 40, 160):
        x = (rng.standard_normal((T, 256)) * 0.5).astype(np.float32)
        with torch.no_grad():
            want = qcrnn.SequenceModeling[0].rnn(torch.from_numpy(x[None]))[0][0].numpy()
            fp32 = crnn.SequenceModeling[0].rnn(torch.from_numpy(x[None]))[0][0].numpy()
        got = Q.bilstm(x, fwd, bwd)
        e_ref, e_f32 = got - want, fp32 - want
        print(f"T = {T}: restatement vs DynamicQuantizedLSTM max {np.abs(e_ref).max():.3e} rms {np.sqrt((e_ref ** 2).mean()):.3e}; "
              f"fp32 LSTM vs DynamicQuantizedLSTM max {np.abs(e_f32).max():.3e} rms {np.sqrt((e_f32 ** 2).mean()):.3e}")
        assert np.sqrt((e_ref ** 2).mean()) < 0.25 * np.sqrt((e_f32 ** 2).mean())


def test_reference_distance_on_the_test_pages(oracle_trained, crnn, qcrnn, qseq):
    """The crops of the GPU test's two pages, fed the oracle's fp32 features: the largest logit distance between the restatement and torch's
    quantised model is what QC.ARGMAX_TOL is four times of; and torch's quantised model alone leaves at least 99 % of the time steps with a
    top-2 margin above that tolerance, so the GPU test's margin rule excludes at most 1 %."""
    worst, steps, above = 0.0, 0, 0
    for img in QC.pages():
        for W, x in QC.page_crops(oracle_trained, img):
            want = QC.logits(qcrnn, x)
            got = qseq(QC.features(crnn, x))
            worst = max(worst, float(np.abs(got - want).max()))
            m = QC.margins(want)
            steps += m.size
            above += int((m > QC.ARGMAX_TOL).sum())
    print(f"{steps} time steps; restatement vs torch's quantised CRNN: max logit distance {worst:.3e} (recorded {QC.REF_MAX_MEASURED:.3e}); "
          f"steps with a margin above ARGMAX_TOL = {QC.ARGMAX_TOL:.3e}: {above}")
    assert worst <= QC.ARGMAX_TOL
    assert above >= (1 - QC.MAX_EXCLUDED) * steps
