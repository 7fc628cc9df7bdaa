"""fp64 references of the fast-mode detector's fused launches and of the BiLSTM recurrence, and the tolerance rule they are held to.

One function per stage (tests/test_gpu_stages.py runs the kernel through tools/micro/stage_shim.hip, tests/test_stage_ref_cpu.py pins these
functions to ``oracle.nets`` and shows that each check fails for a wrong kernel).  Pure torch / numpy, no GPU.

Every stage function computes in ``dt`` (float64 for the references) and takes

* ``q=True``: a round-to-element-type at every point where the kernel stores a value, or feeds it to an MFMA, as 16 bits -- and nowhere else
  (``ref_q``); ``q=False``: no internal rounding (``ref_nq``);
* ``mut``: one named mistake (the sensitivity tests), ``None`` for the operation itself.

``refs_*`` return ``(ref_q, ref_nq, E)``; ``E`` is the allowance of the tolerance rule (below), 0 for single-rounding stages.  Running a stage
function with ``dt=float32, q=True`` and rounding its output is the "stand-in kernel" of the CPU suite.

Weights (``Weights``): BatchNorm is folded with the fp32 operations of ``weights.cpp::fold_conv`` in the same order, so that the value rounded to
the element type is the one the packers round (folding in fp64 first would move a few weights per layer across a rounding boundary); biases,
``w2`` and ``b2`` of the classifier tail stay fp32.  ``el=None`` folds in fp64 and rounds nothing: the composition test's network.

Tolerance rule, per element, with hu = 2^-8 (bf16) / 2^-11 (fp16) / 0 (fp32 outputs), acc = 2e-5 * max(1, max |ref|) (the fp32-output bound
of test_conv_mfma_vs_fp64):

  tight       |got - ref_q|  <= hu |ref_q|  (1 + 1e-3) + 2 acc + 2^-24
  allowance   |got - ref_nq| <= hu |ref_nq| (1 + 1e-3) + 2 acc + 2^-24 + E      for EVERY element
  cap         at most 1 element in 1,000 may miss the tight bound
  no bias     rms(got - ref_nq) <= 1.10 rms(round_el(ref_q) - ref_nq)

E = the image, through the stage's second linear map with |W|, of one element-type ulp of every internally rounded value (ReLU and max-pool are
1-Lipschitz and pass it through); for the recurrence, which has no single second map, E = 2 max |ref_q - ref_nq| of the case.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
HU = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, None: 0.0}
# normalizeMeanVariance's constants as the kernel spells them (fp32 products)
_MEAN = (np.array([0.485, 0.456, 0.406], dtype=np.float32) * np.float32(255.0)).astype(np.float32)
_STD = (np.array([0.229, 0.224, 0.225], dtype=np.float32) * np.float32(255.0)).astype(np.float32)


def craft_state(seed):
    """weights.synthetic_craft_state with conv1_1's BatchNorm shift raised by 1.  The synthetic state draws every BN shift from N(0, 0.05), so
    relu(bias) of conv1_1 -- what a kernel that forgets conv1_2's zero padding writes into the ring beyond the canvas -- is ~30 times smaller
    than conv1_1's activations and that mistake (~0.02 on border outputs) would sit below the bf16 allowance of this two-rounding stage
    (E ~ 1.7).  With a shift of the order of the activations, as in a trained first layer, it exceeds the allowance 2.1 (bf16) / 17 (fp16) times."""
    from bb_ocr_amd import weights

    sd = weights.synthetic_craft_state(seed)
    sd["basenet.slice1.1.bias"] = (sd["basenet.slice1.1.bias"] + np.float32(1.0)).astype(np.float32)
    return sd


def rnd(t, el):
    """round to the element type (RNE), back in t's dtype; el None: identity"""
    return t if el is None else t.to(DTYPES[el]).to(t.dtype)


def ulp_el(t, el):
    """one element-type ulp at |t| (0 at 0), fp64"""
    a = t.abs().double()
    _, e = torch.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    p, emin = (7, -126) if el == "bf16" else (10, -14)
    u = torch.ldexp(torch.ones_like(a), torch.clamp(e - 1, min=emin) - p)
    return torch.where(a > 0, u, torch.zeros_like(a))


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Weights:
    """Folded (and, for el in DTYPES, rounded) parameters of a CRAFT state dict, fp64 tensors: ``layer(conv, bn) -> (w, b)``."""

    def __init__(self, sd, el):
        self.sd, self.el, self._c = sd, el, {}

    def layer(self, conv, bn=None):
        key = (conv, bn)
        if key not in self._c:
            sd = self.sd
            ft = np.float64 if self.el is None else np.float32
            w = np.asarray(sd[conv + ".weight"]).astype(ft)
            b = np.asarray(sd[conv + ".bias"]).astype(ft) if conv + ".bias" in sd else np.zeros(w.shape[0], dtype=ft)
            if bn:
                g, be = np.asarray(sd[bn + ".weight"]).astype(ft), np.asarray(sd[bn + ".bias"]).astype(ft)
                mu, var = np.asarray(sd[bn + ".running_mean"]).astype(ft), np.asarray(sd[bn + ".running_var"]).astype(ft)
                sc = (g / np.sqrt(var + ft(1e-5))).astype(ft)     # weights.cpp::fold_conv, same order
                w = (w * sc[:, None, None, None]).astype(ft)
                b = (((b - mu).astype(ft) * sc).astype(ft) + be).astype(ft)
            self._c[key] = (rnd(torch.from_numpy(w.astype(np.float64)), self.el), torch.from_numpy(b.astype(np.float64)))
        return self._c[key]

    def tail(self):
        """conv_cls.6 (W1 rounded: it is an MFMA operand; b1 fp32), conv_cls.8 (fp32)"""
        sd = self.sd
        f = lambda k: torch.from_numpy(np.asarray(sd[k]).astype(np.float64))
        return rnd(f("conv_cls.6.weight"), self.el), f("conv_cls.6.bias"), f("conv_cls.8.weight"), f("conv_cls.8.bias")

    # the layers the stages use
    def c11(self): return self.layer("basenet.slice1.0", "basenet.slice1.1")
    def c12(self): return self.layer("basenet.slice1.3", "basenet.slice1.4")
    def up1a(self): return self.layer("upconv1.conv.0", "upconv1.conv.1")
    def up3b(self): return self.layer("upconv3.conv.3", "upconv3.conv.4")
    def up4b(self): return self.layer("upconv4.conv.3", "upconv4.conv.4")
    def cls4(self): return self.layer("conv_cls.4")

    def upN(self, level):
        """(W_y, W_s, b) of upconv{level}'s 1x1 over cat[up(y), skip]"""
        w, b = self.layer(f"upconv{level}.conv.0", f"upconv{level}.conv.1")
        cy = {2: 256, 3: 128, 4: 64}[level]
        return w[:, :cy], w[:, cy:], b


def conv(x, w, b=None, pad=0, dil=1):
    return F.conv2d(x, w.to(x.dtype), None if b is None else b.to(x.dtype), padding=pad, dilation=dil)


# ------------------------------------------------------------------------------------------------ stages (NHWC in, NHWC out)
def normalise(rgb_u8, Himg, Wimg, H32, W32, el, q, dt, mut=None):
    """uint8 pages [N, Himg, Wimg, 3] on the raw-zero canvas -> normalised NCHW [N, 3, H32, W32]"""
    N = rgb_u8.shape[0]
    canvas = torch.zeros((N, H32, W32, 3), dtype=torch.float32)
    canvas[:, :Himg, :Wimg] = rgb_u8.float()
    if q:
        xn = ((canvas - torch.from_numpy(_MEAN)) / torch.from_numpy(_STD)).to(dt)       # the kernel's fp32 subtraction and (IEEE) division
        xn = rnd(xn, el)
    else:
        xn = (canvas.double() - torch.from_numpy(_MEAN).double()) / torch.from_numpy(_STD).double()
        xn = xn.to(dt)
    if mut == "canvas_norm0":                      # beyond the page but on the canvas: normalised 0 instead of the normalised raw 0
        m = torch.zeros((H32, W32), dtype=torch.bool)
        m[:Himg, :Wimg] = True
        xn = xn * m[None, :, :, None].to(dt)
    return nchw(xn)


def c11_conv1_2_pool(W, rgb_u8, Himg, Wimg, H32, W32, el, q=True, dt=torch.float64, mut=None):
    xn = normalise(rgb_u8, Himg, Wimg, H32, W32, el, q, dt, mut)
    w1, b1 = W.c11()
    w2, b2 = W.c12()
    a = F.relu(conv(xn, w1, b1, pad=1))
    if q:
        a = rnd(a, el)
    if mut == "pad_relu_bias":                     # beyond the canvas: relu(bias) where conv1_2's zero padding belongs
        ap = F.relu(b1.to(dt))[None, :, None, None].expand(a.shape[0], -1, H32 + 2, W32 + 2).clone()
        ap[:, :, 1:-1, 1:-1] = a
        y = conv(ap, w2, b2, pad=0)
    else:
        y = conv(a, w2, b2, pad=1)
    return nhwc(F.max_pool2d(F.relu(y), 2))


def refs_c11(W, rgb_u8, Himg, Wimg, H32, W32, el):
    rq = c11_conv1_2_pool(W, rgb_u8, Himg, Wimg, H32, W32, el, True)
    rn = c11_conv1_2_pool(W, rgb_u8, Himg, Wimg, H32, W32, el, False)
    xn = normalise(rgb_u8, Himg, Wimg, H32, W32, el, False, torch.float64)
    w1, b1 = W.c11()
    w2, _ = W.c12()
    a = F.relu(conv(xn, w1, b1, pad=1))
    e1 = conv(ulp_el(xn, el), w1.abs(), pad=1) + ulp_el(a, el)       # both intermediates, chained
    return rq, rn, nhwc(F.max_pool2d(conv(e1, w2.abs(), pad=1), 2))


def up1a(W, f7, s4, el, q=True, dt=torch.float64, mut=None):
    w, b = W.up1a()
    wa, wb = (w[:, 512:], w[:, :512]) if mut == "concat_swapped" else (w[:, :1024], w[:, 1024:])
    return nhwc(F.relu(conv(nchw(f7.to(dt)), wa) + conv(nchw(s4.to(dt)), wb, b)))


def upsample2(z, mut=None):
    """F.interpolate(scale 2, bilinear, align_corners=False) of NCHW z, or one of the mistakes"""
    if mut == "align_corners":
        return F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=True)
    if mut == "nearest":
        return F.interpolate(z, scale_factor=2, mode="nearest")
    u = F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)
    if mut == "edge_unclamped":                    # the far edge takes its neighbour's value
        u = u.clone()
        u[:, :, :, -1] = u[:, :, :, -2]
        u[:, :, -1, :] = u[:, :, -2, :]
    if mut == "page_off_by_one" and u.shape[0] > 1:    # first pixel of page 1 gathered from page 0
        u = u.clone()
        u[1, :, 0, 0] = u[0, :, 0, 0]
    return u


def addup(W, level, skip, z, el, q=True, dt=torch.float64, mut=None):
    """ReLU(up(z) + W_s skip + b): the skip half of upconv{level}'s 1x1 (single rounding: z arrives in the element type)"""
    _, ws, b = W.upN(level)
    return nhwc(F.relu(upsample2(nchw(z.to(dt)), mut) + conv(nchw(skip.to(dt)), ws, b)))


def up3b_post(W, u3a, el, q=True, dt=torch.float64, mut=None):
    w3, b3 = W.up3b()
    wy, _, _ = W.upN(4)
    y = conv(nchw(u3a.to(dt)), w3, b3, pad=1)
    if mut == "relu_after_post":
        return nhwc(F.relu(conv(rnd(y, el) if q else y, wy)))
    u = F.relu(y)
    if q:
        u = rnd(u, el)
    return nhwc(conv(u, wy))


def refs_up3b_post(W, u3a, el):
    w3, b3 = W.up3b()
    wy, _, _ = W.upN(4)
    u = F.relu(conv(nchw(u3a.double()), w3, b3, pad=1))
    return up3b_post(W, u3a, el, True), up3b_post(W, u3a, el, False), nhwc(conv(ulp_el(u, el), wy.abs()))


def up4(W, s1, z, el, q=True, dt=torch.float64, mut=None):
    _, ws, b = W.upN(4)
    w3, b3 = W.up4b()
    u = F.relu(upsample2(nchw(z.to(dt)), mut) + conv(nchw(s1.to(dt)), ws, b))
    if q:
        u = rnd(u, el)
    return nhwc(F.relu(conv(u, w3, b3, pad=1)))


def refs_up4(W, s1, z, el):
    _, ws, b = W.upN(4)
    w3, _ = W.up4b()
    u = F.relu(upsample2(nchw(z.double())) + conv(nchw(s1.double()), ws, b))
    return up4(W, s1, z, el, True), up4(W, s1, z, el, False), nhwc(conv(ulp_el(u, el), w3.abs(), pad=1))


def cls_tail(W, c2, el, q=True, dt=torch.float64, mut=None):
    w4, b4 = W.cls4()
    w1, b1, w2, b2 = W.tail()
    if mut == "w1_transposed":
        w1 = w1.transpose(0, 1).contiguous()
    c3 = F.relu(conv(nchw(c2.to(dt)), w4, b4, pad=1))
    if q:
        c3 = rnd(c3, el)
    return nhwc(conv(F.relu(conv(c3, w1, b1)), w2, b2))


def refs_cls_tail(W, c2, el):
    w4, b4 = W.cls4()
    w1, _, w2, _ = W.tail()
    c3 = F.relu(conv(nchw(c2.double()), w4, b4, pad=1))
    return cls_tail(W, c2, el, True), cls_tail(W, c2, el, False), nhwc(conv(conv(ulp_el(c3, el), w1.abs()), w2.abs()))


def pool5(x, mut=None):
    """MaxPool2d(3, 1, 1) on an element-type NHWC tensor, in that type's values (a selection: bit-exact)"""
    xc = nchw(x if x.dtype == torch.float64 else x.float())
    if mut == "zero_pad":
        return nhwc(F.max_pool2d(F.pad(xc, (1, 1, 1, 1), value=0.0), 3, 1, 0)).to(x.dtype)
    return nhwc(F.max_pool2d(xc, 3, 1, 1)).to(x.dtype)


# ------------------------------------------------------------------------------------------------ BiLSTM recurrence
def lstm_weights(sd, layer, el):
    """(W_hh forward, W_hh backward) [1024, 256] fp64, rounded where pack_lstm_whh8 rounds them"""
    k = f"SequenceModeling.{layer}.rnn.weight_hh_l0"
    f = lambda s: rnd(torch.from_numpy(np.asarray(sd[s]).astype(np.float64)), el)
    return f(k), f(k + "_reverse")


def lstm_dir(whh, x, reverse, el, q=True, dt=torch.float64, mut=None, pad_x=None):
    """One direction of torch.nn.LSTM(256, 256) behind the input projection: x [n, T, 1024] = x W_ih^T + b_ih + b_hh (gate order i, f, g, o)
    -> the UNROUNDED h_t [n, T, 256] of every step; with q the value that crosses to the next step is rounded (h crosses LDS as 16 bits).
    pad_x [n, P, 1024] (mut 'bwd_padded_start'): rows behind the sequence that a backward pass started at the padded length would consume."""
    n, T, _ = x.shape
    x = x.to(dt)
    w = whh.to(dt).t()
    h = torch.zeros((n, 256), dtype=dt)
    c = torch.zeros((n, 256), dtype=dt)
    out = torch.zeros((n, T, 256), dtype=dt)
    order = {"gate_order": (0, 2, 1, 3)}.get(mut, (0, 1, 2, 3))

    def step(xt, h, c):
        pre = xt + h @ w
        gi, gf, gg, go = (pre[:, 256 * k:256 * (k + 1)] for k in order)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        hu = torch.sigmoid(go) * torch.tanh(c)
        return hu, (rnd(hu, el) if q else hu), c

    if mut == "bwd_padded_start" and reverse:
        for t in range(pad_x.shape[1] - 1, -1, -1):
            _, h, c = step(pad_x[:, t].to(dt), h, c)
    for s in range(T):
        t = T - 1 - s if reverse else s
        hu, h, c = step(x[:, t], h, c)
        out[:, t] = hu
    return out


def lstm_seq_carry_c(whh, x, reverse, el, q=True, dt=torch.float64):
    """the 'c carried across sequences of a tile' mistake: sequence s starts from sequence s-1's final cell state"""
    outs, c_prev = [], None
    for s in range(x.shape[0]):
        n, T, _ = x[s:s + 1].shape
        w = whh.to(dt).t()
        h = torch.zeros((1, 256), dtype=dt)
        c = torch.zeros((1, 256), dtype=dt) if c_prev is None else c_prev
        o = torch.zeros((1, T, 256), dtype=dt)
        for k in range(T):
            t = T - 1 - k if reverse else k
            pre = x[s:s + 1, t].to(dt) + h @ w
            gi, gf, gg, go = (pre[:, 256 * j:256 * (j + 1)] for j in range(4))
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            hu = torch.sigmoid(go) * torch.tanh(c)
            h = rnd(hu, el) if q else hu
            o[:, t] = hu
        c_prev = c
        outs.append(o)
    return torch.cat(outs)


def bilstm(whh_f, whh_b, x, el, q=True, dt=torch.float64, mut=None, pad_x=None):
    """x [n, T, 2, 1024] (direction, gate * 256 + unit) -> [n, T, 512] (fwd | bwd)"""
    if mut == "carry_c":
        return torch.cat([lstm_seq_carry_c(whh_f, x[:, :, 0], False, el, q, dt), lstm_seq_carry_c(whh_b, x[:, :, 1], True, el, q, dt)], dim=2)
    return torch.cat([lstm_dir(whh_f, x[:, :, 0], False, el, q, dt, mut, None if pad_x is None else pad_x[:, :, 0]),
                      lstm_dir(whh_b, x[:, :, 1], True, el, q, dt, mut, None if pad_x is None else pad_x[:, :, 1])], dim=2)


def refs_bilstm(whh_f, whh_b, x, el):
    rq, rn = bilstm(whh_f, whh_b, x, el, True), bilstm(whh_f, whh_b, x, el, False)
    return rq, rn, 2.0 * (rq - rn).abs().max().item()


# ------------------------------------------------------------------------------------------------ the tolerance rule
def bounds(ref_q, ref_nq, E, el_out):
    """(tight, allowance) per element.  el_out: element type of the stage's OUTPUT (None: fp32)"""
    hu = HU[el_out]
    acc_q = 2e-5 * max(1.0, ref_q.abs().max().item())
    acc_n = 2e-5 * max(1.0, ref_nq.abs().max().item())
    tight = hu * ref_q.abs() * (1 + 1e-3) + 2 * acc_q + 2.0 ** -24
    allow = hu * ref_nq.abs() * (1 + 1e-3) + 2 * acc_n + 2.0 ** -24 + E
    return tight, allow


def rms(t):
    return float(torch.sqrt((t.double() ** 2).mean()))


def round_out(t, el_out):
    return rnd(t, el_out) if el_out is not None else t.float().double()


def localise(miss, beyond=None):
    """miss [N, H, W, C] bool -> counts by region (an element may fall in several)"""
    N, H, W, _ = miss.shape
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    border = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
    seam = ((ys % 16 == 0) | (ys % 16 == 15) | (xs % 16 == 0) | (xs % 16 == 15)) & ~border
    ends = ((ys == 0) & (xs == 0)) | ((ys == H - 1) & (xs == W - 1))
    px = miss.any(dim=3)
    cnt = lambda m: int((px & m[None]).sum())
    d = {"interior": cnt(~border & ~seam), "page border": cnt(border), "tile seam": cnt(seam), "first/last pixel of a page": cnt(ends)}
    if beyond is not None:
        d["beyond-page canvas"] = cnt(beyond)
    return d


def check(got, ref_q, ref_nq, E, el_out, name="", beyond=None, index_names=("n", "y", "x", "c")):
    """Apply the rule; returns {'share', 'worst', 'ratio'} and raises AssertionError with a localised report.  got: fp64, same shape."""
    got = got.double()
    assert got.shape == ref_q.shape == ref_nq.shape, (got.shape, ref_q.shape)
    finite = torch.isfinite(got)
    tight, allow = bounds(ref_q, ref_nq, E, el_out)
    dq, dn = (got - ref_q).abs(), (got - ref_nq).abs()
    miss_t = ~(dq <= tight)
    miss_a = ~(dn <= allow)
    share = float(miss_t.double().mean())
    rel = torch.where(finite, dn / allow, torch.full_like(dn, float("inf")))
    worst = float(rel.max())
    noise = rms(round_out(ref_q, el_out) - ref_nq)
    ratio = rms(torch.where(finite, got - ref_nq, torch.zeros_like(got))) / noise if noise > 0 else 0.0
    stats = {"share": share, "worst": worst, "ratio": ratio}
    print(f"[stage] {name}: share beyond tight {share:.3g}, max |got - ref_nq| / allowance {worst:.3g}, rms ratio {ratio:.4f}")
    problems = []
    if not finite.all():
        problems.append(f"{int((~finite).sum())} non-finite values")
    if miss_a.any():
        problems.append(f"{int(miss_a.sum())} elements beyond the allowance")
    if share > 1e-3:
        problems.append(f"share beyond the tight bound {share:.3g} > 1e-3")
    if noise > 0 and ratio > 1.10:
        problems.append(f"rms(got - ref_nq) is {ratio:.4f} x the reference's own quantisation noise (> 1.10)")
    if problems:
        bad = miss_a if miss_a.any() else miss_t
        w = int(torch.argmax(torch.where(bad, rel, torch.zeros_like(rel))))
        idx = np.unravel_index(w, tuple(got.shape))
        where = ", ".join(f"{k}={int(v)}" for k, v in zip(index_names, idx))
        msg = f"{name}: " + "; ".join(problems) + f"; worst element ({where}): got {got.flatten()[w].item():.9g}, ref_q {ref_q.flatten()[w].item():.9g}, " \
              f"ref_nq {ref_nq.flatten()[w].item():.9g}, allowance {allow.flatten()[w].item() if torch.is_tensor(allow) else allow:.3g}"
        if got.dim() == 4:
            msg += f"; beyond allowance by region {localise(miss_a, beyond)}; beyond tight by region {localise(miss_t, beyond)}"
        raise AssertionError(msg)
    return stats


def fails_allowance(mutated, ref_q, ref_nq, E, el_out):
    """does a kernel that computed `mutated` (exactly) miss the allowance bound somewhere?  (the sensitivity tests)"""
    _, allow = bounds(ref_q, ref_nq, E, el_out)
    m = mutated.double()
    return bool(((m - ref_q).abs() > allow).any()) and bool(((m - ref_nq).abs() > allow).any())
