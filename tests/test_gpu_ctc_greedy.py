"""-m gpu: the greedy CTC stage (ctc.hip: ctc_rows_kernel + ctc_collapse_kernel, then ctc_decode's host pow) ONE launch at a time through
tools/micro/stage_shim.hip::stage_ctc_greedy, which uploads a ragged sequence table and calls launch_ctc as a recognition pass does, into
tensors this test owns and has filled with sentinels.  Every row of tests/ctc_greedy_cases.py, in a bf16 and in an exact context (the
stage is float32 in both), under the rule of tests/ctc_greedy_ref.py:

* the device probabilities against float64, every element within the derived prob_bound;
* everything behind them -- idx, pmax, text, len, cnt, prod, confidence -- bit for bit from the device's own probabilities;
* nothing written outside what the stage owns; two runs bit-identical; idx / pmax identical whether or not probs is requested;
* idx against the float64 arg-max on every decidable row, with the cap on undecidable ones asserted here as well.

Measured on an MI355X with ctc.hip as it stood: all 79 cases pass in both contexts; worst |error| / prob_bound 0.771 (range/spread_80, an
element 65.3 below its row's maximum), 0.65 at C = 97 / cs = 112 and over the masked cases (mask/allow_digits, where the mask removes
most rows' arg-max), the same figures in both contexts; torch's float32 softmax on the CPU reaches 0.779 / 0.63 on the same table
(test_ctc_greedy_cpu.py).  No undecidable row outside the tie cases.

Set BBOCR_STAGE_STATS=<file> to collect one JSON line per case (worst |error| / prob_bound)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ctc_greedy_cases as K
import ctc_greedy_ref as R
from test_gpu_stages import Stage, _record, shim_path, stage_states  # noqa: F401  (the fixtures build the shim and the weights)

pytestmark = pytest.mark.gpu

SHIM_BAD_ARGS = 20000


@pytest.fixture(scope="module", params=["bf16", "exact"])
def ctc_st(request, shim_path, stage_states):  # noqa: F811
    s = Stage(shim_path, stage_states, request.param)
    s.lib.stage_ctc_decode.restype = C.c_double
    s.lib.stage_ctc_decode.argtypes = [C.c_int, C.c_int, C.c_float]
    K.assert_caps()                            # the exemption of undecidable rows below is bounded by the table alone
    yield s
    s.reader.close()


class Outs:
    """the stage's output tensors, sentinel-filled"""

    def __init__(self, case, want_probs):
        rows, nseq = len(case.logits), len(case.seqs)
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device="cuda")
        self.idx, self.pmax = full(rows, R.S_IDX, torch.int32), full(rows, float("nan"), torch.float32)
        self.out_idx, self.ctc_out = full(rows, R.S_OUT, torch.int32), full((nseq + 2) * 4, R.S_CTC, torch.int32)
        self.probs = torch.full((rows, case.cs), R.S_PROB, dtype=torch.float32, device="cuda") if want_probs else None

    def args(self):
        return self.idx, self.pmax, self.out_idx, self.ctc_out, self.probs

    def host(self):
        return [None if t is None else t.cpu().numpy() for t in self.args()]


def _args(case, d):
    seqs = np.ascontiguousarray(case.seqs)
    mask = (C.c_uint * 4)(*case.mask) if case.mask is not None else C.c_void_p(None)
    return seqs, (d, len(case.logits), case.C, case.cs, seqs.ctypes.data_as(C.c_void_p), len(case.seqs), mask)


def _launch(s, case, d, want_probs):
    o = Outs(case, want_probs)
    seqs, a = _args(case, d)
    s.call("stage_ctc_greedy", *a, *o.args())
    return o.host()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", list(K.BY_NAME))
def test_ctc_greedy_stage(ctc_st, name):
    case = K.BY_NAME[name]
    d = torch.from_numpy(case.logits).cuda()
    first, second, bare = _launch(ctc_st, case, d, True), _launch(ctc_st, case, d, True), _launch(ctc_st, case, d, False)
    for what, a, b in zip(("idx", "pmax", "out_idx", "ctc_out", "probs"), first, second):
        assert _same_bits(a, b), f"{name}: two runs on the same input differ in {what}"
    for what, a, b in zip(("idx", "pmax", "out_idx", "ctc_out"), first, bare):
        assert _same_bits(a, b), f"{name}: {what} differs between a launch with probs and one without"
    idx, pmax, out_idx, ctc_out, probs = first
    ctc_out = ctc_out.reshape(-1, 4)
    ratio = R.check_probs(case, probs)
    print(f"{name} {ctc_st.el}: worst |error| / prob_bound = {ratio:.3f}")
    R.check_exact(case, probs, idx, pmax, out_idx, ctc_out, decode=lambda ln, cn, prod: ctc_st.lib.stage_ctc_decode(ln, cn, float(prod)))
    undecided = R.check_fp64(case, idx)
    _record("ctc_greedy", ctc_st.el, name, {"worst_ratio": ratio, "undecidable_rows": undecided, "rows": len(case.logits)})


def test_ctc_greedy_refusals(ctc_st):
    """C = 129 through the public op: an error status, nothing written, the context usable afterwards.  A sequence that reaches past
    `rows`: refused by the shim before anything is queued."""
    case = K.BY_NAME["width/C97-cs131"]
    n, T = case.uniform()
    d = torch.from_numpy(case.logits).cuda()
    lib, h = ctc_st.reader._lib, ctc_st.h

    def op(Cn):
        off, idx, conf = (C.c_int * (n + 1))(*[-3] * (n + 1)), (C.c_int * (n * T))(*[-3] * (n * T)), (C.c_double * n)(*[-3.0] * n)
        torch.cuda.synchronize()
        return lib.bbocr_op_ctc(h, C.c_void_p(d.data_ptr()), n, T, Cn, case.cs, off, idx, conf, None, 0), list(off), list(idx), list(conf)

    rc, off, idx, conf = op(129)
    assert rc != 0 and set(off) == {-3} and set(idx) == {-3} and set(conf) == {-3.0}
    rc, off, idx, conf = op(97)
    assert rc == 0 and case.decidable.all()
    want = case.p64.argmax(axis=1)
    for k in range(n):
        assert idx[off[k]:off[k + 1]] == R.collapse(want[k * T:(k + 1) * T]), k
        assert 0.0 < conf[k] <= 1.0
    # the shim: a table entry that ends one row past the logits
    o = Outs(case, True)
    seqs = np.array([[0, T], [n * T - 4, 5]], dtype=np.int32)
    torch.cuda.synchronize()
    a = [C.c_void_p(d.data_ptr()), C.c_size_t(d.numel()), n * T, case.C, case.cs, seqs.ctypes.data_as(C.c_void_p), 2, C.c_void_p(None)]
    for t in o.args():
        a += [C.c_void_p(t.data_ptr()), C.c_size_t(t.numel())]
    assert ctc_st.lib.stage_ctc_greedy(h, *a) == SHIM_BAD_ARGS
    torch.cuda.synchronize()
    idx, pmax, out_idx, ctc_out, probs = o.host()
    assert (idx == R.S_IDX).all() and np.isnan(pmax).all() and (out_idx == R.S_OUT).all() and (ctc_out == R.S_CTC).all() and (probs == R.S_PROB).all()
    first = _launch(ctc_st, case, d, True)          # and the context still runs the stage
    ctc_out = first[3].reshape(-1, 4)
    R.check_exact(case, first[4], first[0], first[1], first[2], ctc_out)
    for k in range(n):                              # the public op's confidence is the stage's CtcOut through the same pow
        ref = R.conf(ctc_out[k, 2:3].view(np.float32)[0], int(ctc_out[k, 1]))
        assert abs(conf[k] - ref) <= math.ulp(ref), k
