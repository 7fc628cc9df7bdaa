"""numpy restatement of the recogniser's ``rec_quant`` arithmetic: torch's x86 / fbgemm DYNAMIC int8 quantisation of ``nn.LSTM`` and
``nn.Linear`` (``torch.quantization.quantize_dynamic(model, dtype=torch.qint8)``), per crop.  DESIGN.md section 4 states the definition;
tests/test_quant_ref_cpu.py pins this file to torch bit for bit, tests/test_gpu_rec_quant.py pins the device to this file.

Everything that is float32 in the definition is float32 here (numpy scalars, never Python floats), everything that is double is float64.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
QMAX = 127                    # reduce_range: the activation PARAMETERS are chosen for codes 0..127 ...
CODE_MAX = 255                # ... but fbgemm's Quantize<uint8_t> clamps to the uint8 range.  The only code above 127 that can occur is 128:
                              # x = max maps to 127 + (zp - z) with z the unrounded zero point, i.e. to 127.5 when z = k + 1/2 was rounded up
                              # (h = +-1 exactly: z = 63.5 -> 64), and 127.5 rounds to 128.  code - zp still fits a signed byte (zp >= 1 then).


# ------------------------------------------------------------------------------------------------ weights
def quantize_weight(w: np.ndarray):
    """Symmetric per-tensor qint8 (default_weight_observer + torch.quantize_per_tensor) -> (int8 codes, float32 scale)."""
    w = np.ascontiguousarray(w, dtype=F32)
    mn = min(F32(w.min()), F32(0))
    mx = max(F32(w.max()), F32(0))
    amax = max(-mn, mx)                                      # float32
    scale = F32(amax / F32(127.5))                           # (quant_max - quant_min) / 2 = 127.5, float32 division
    scale = max(scale, np.finfo(F32).eps)
    inv = F32(1.0) / scale
    q = np.clip(np.rint(w * inv), -128, 127).astype(np.int8)     # quantize_per_tensor: nearbyint(x * inv_scale) + 0, clamped
    return q, F32(scale)


# ------------------------------------------------------------------------------------------------ activations
def qparams(x: np.ndarray):
    """fbgemm ChooseQuantizationParams(min, max, 0, 127) of one tensor -> (float32 scale, int zero point)."""
    x = np.asarray(x, dtype=F32)
    mn = min(F32(x.min()), F32(0))
    mx = max(F32(x.max()), F32(0))
    scale = (np.float64(mx) - np.float64(mn)) / np.float64(QMAX)
    with np.errstate(divide="ignore", over="ignore"):
        if F32(scale) == 0 or np.isinf(F32(1.0) / F32(scale)):
            scale = np.float64(0.1)
    zmin = np.float64(0) - np.float64(mn) / scale
    zmax = np.float64(QMAX) - np.float64(mx) / scale
    emin = abs(np.float64(0)) + abs(np.float64(mn) / scale)
    emax = abs(np.float64(QMAX)) + abs(np.float64(mx) / scale)
    z = zmin if emin < emax else zmax
    if z < 0:
        zp = 0
    elif z > QMAX:
        zp = QMAX
    else:
        zp = int(np.rint(z))
    return F32(scale), zp


def fma32(a: np.ndarray, b, c) -> np.ndarray:
    """float32 fused multiply-add of float32 operands, correctly rounded.  The product of two float32 values is exact in float64; the float64
    sum is rounded once, and rounding it again to float32 gives the fused result except where the float64 sum sits exactly half-way between
    two float32 values although the exact sum does not (double rounding).  Those elements -- the low 29 bits of the float64 significand
    are 1 0 ... 0 -- are decided with exact rational arithmetic."""
    from fractions import Fraction

    a64, c64 = np.asarray(a, np.float64), np.asarray(c, np.float64)
    s = np.atleast_1d(a64 * np.float64(b) + c64)
    out = s.astype(F32)
    half = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    if half.any():
        ab, cb = np.broadcast_to(a64, s.shape), np.broadcast_to(c64, s.shape)
        for i in zip(*np.nonzero(half)):
            exact = Fraction(float(ab[i])) * Fraction(float(b)) + Fraction(float(cb[i]))
            mid = Fraction(float(s[i]))
            if exact != mid:          # the float64 sum was itself rounded on to the mid-point: the exact sum says which neighbour is nearer
                lo, hi = np.nextafter(out[i], F32(-np.inf)), np.nextafter(out[i], F32(np.inf))
                below = out[i] if Fraction(float(out[i])) < mid else lo
                above = out[i] if Fraction(float(out[i])) > mid else hi
                out[i] = above if exact > mid else below
    return out.reshape(np.broadcast(a64, c64).shape)


def codes(x: np.ndarray, scale, zp: int) -> np.ndarray:
    """uint8 codes: clamp(nearbyint(x * inv + zp), 0, 255), the sum in float32 (fused), ties to even."""
    inv = F32(1.0) / F32(scale)
    t = fma32(np.asarray(x, F32), inv, F32(zp))
    return np.clip(np.rint(t), 0, CODE_MAX).astype(np.uint8)


def codes_unfused(x, scale, zp):            # x * inv rounded to float32, then + zp rounded again
    inv = F32(1.0) / F32(scale)
    t = (np.asarray(x, F32) * inv).astype(F32) + F32(zp)
    return np.clip(np.rint(t.astype(F32)), 0, CODE_MAX).astype(np.uint8)


def codes_round_first(x, scale, zp):        # rejected variant: round x * inv, add zp as an integer
    inv = F32(1.0) / F32(scale)
    t = np.rint((np.asarray(x, F32) * inv).astype(F32)).astype(np.int64) + zp
    return np.clip(t, 0, CODE_MAX).astype(np.uint8)


def codes_divide(x, scale, zp):             # rejected variant: x / scale
    t = (np.asarray(x, F32) / F32(scale)).astype(F32) + F32(zp)
    return np.clip(np.rint(t.astype(F32)), 0, CODE_MAX).astype(np.uint8)


def qlinear(x: np.ndarray, qw: np.ndarray, sw, bias: np.ndarray, code_fn=codes):
    """One dynamically quantised matrix product over the whole tensor x [T, K] -> (out [T, N] float32, codes, scale, zp)."""
    x = np.asarray(x, F32)
    scale, zp = qparams(x)
    cd = code_fn(x, scale, zp)
    acc = (cd.astype(np.int32) - zp) @ qw.astype(np.int32).T                   # exact: |acc| < 2^31
    mult = F32(F32(scale) * F32(sw))
    out = fma32(acc.astype(F32), mult, np.asarray(bias, F32)[None, :])
    return out, cd, scale, zp


# ------------------------------------------------------------------------------------------------ LSTM
def _sigmoid(x):
    x = np.asarray(x, F32)
    return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)


def lstm_step(g_t: np.ndarray, h: np.ndarray, c: np.ndarray, qw_hh, sw_hh, b_hh):
    """One step of one direction: gates = G[t] + qlinear(h) (h quantised from its own 256 values) -> (h', c', pre-activation gates,
    codes of h, scale, zp).  Gate order i, f, g, o."""
    hq, cd, scale, zp = qlinear(np.asarray(h, F32)[None, :], qw_hh, sw_hh, b_hh)
    gates = (np.asarray(g_t, F32) + hq[0]).astype(F32)
    H = h.shape[0]
    i, f, g, o = (gates[k * H:(k + 1) * H] for k in range(4))
    c2 = (_sigmoid(f) * np.asarray(c, F32) + _sigmoid(i) * np.tanh(g, dtype=F32)).astype(F32)
    h2 = (_sigmoid(o) * np.tanh(c2, dtype=F32)).astype(F32)
    return h2, c2, gates, cd[0], scale, zp


class QLSTMDir:
    """Quantised tensors of one direction of one layer."""

    def __init__(self, w_ih, w_hh, b_ih, b_hh):
        self.q_ih, self.s_ih = quantize_weight(w_ih)
        self.q_hh, self.s_hh = quantize_weight(w_hh)
        self.b_ih, self.b_hh = np.asarray(b_ih, F32), np.asarray(b_hh, F32)


def bilstm(x: np.ndarray, fwd: QLSTMDir, bwd: QLSTMDir) -> np.ndarray:
    """x [T, in] of ONE crop -> [T, 2H]: per direction one input projection over the whole tensor, then T steps."""
    T = x.shape[0]
    H = fwd.q_hh.shape[1]
    out = np.zeros((T, 2 * H), F32)
    for d, p in enumerate((fwd, bwd)):
        G = qlinear(x, p.q_ih, p.s_ih, p.b_ih)[0]
        h, c = np.zeros(H, F32), np.zeros(H, F32)
        for step in range(T):
            t = T - 1 - step if d else step
            h, c = lstm_step(G[t], h, c, p.q_hh, p.s_hh, p.b_hh)[:2]
            out[t, d * H:(d + 1) * H] = h
    return out


class QSequence:
    """The sequence half of the recogniser from a state-dict of numpy arrays (oracle.nets.CRNN key names)."""

    def __init__(self, state):
        g = lambda k: np.asarray(state[k], F32)
        self.layers = []
        for l in range(2):
            sm = f"SequenceModeling.{l}."
            dirs = [QLSTMDir(g(sm + "rnn.weight_ih_l0" + s), g(sm + "rnn.weight_hh_l0" + s), g(sm + "rnn.bias_ih_l0" + s), g(sm + "rnn.bias_hh_l0" + s))
                    for s in ("", "_reverse")]
            ql, sl = quantize_weight(g(sm + "linear.weight"))
            self.layers.append((dirs[0], dirs[1], ql, sl, g(sm + "linear.bias")))
        self.q_pred, self.s_pred = quantize_weight(g("Prediction.weight"))
        self.b_pred = g("Prediction.bias")

    def __call__(self, v: np.ndarray) -> np.ndarray:
        """v [T, 256]: the 3-row mean of one crop's conv features -> logits [T, 97]."""
        x = np.asarray(v, F32)
        for fwd, bwd, ql, sl, bl in self.layers:
            x = qlinear(bilstm(x, fwd, bwd), ql, sl, bl)[0]
        return qlinear(x, self.q_pred, self.s_pred, self.b_pred)[0]
