"""fp64 references of the fast-mode detector's fused launches, of the BiLSTM recurrence and of the recogniser's conv stack (one crop at a
time), and the tolerance rule they are held to.

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

The exact mode's split-fp16 stages (pair tensors [hi | lo], split plans, the pair kernels, lstm_exact_kernel; second half of this module) have a
rule of their own -- the acc term above is two orders of magnitude over that mode's real error.  Per element (EXACT_RULE has the derivation):

  |got - ref| <= u |ref| + (2^-21 + 2 q32) S + 2^-35

u = 2^-22 (pair output) / 2^-24 (fp32 output); S = |W| * |x| + |b|; 2^-21 = the split representation's worst case; q32 = max |standin - ref| / S
of the same case, standin = the launch's three product terms accumulated in float32 32 products at a time (the float32 FMA chain for
pair_conv1_1, crnn_conv0_kernel and pair_cls_tail), computed on the CPU and required to stay <= 2^-22.  Selections (pair ReLU, MaxPool(3,1,1),
the same-size upcat) hold bit for bit; the up-sampling upcat: 2^-22 |ref| + 2^-23 (blend of the four |neighbours|); the recurrence, per tile:
max |got - ref| <= 8 max |fp32 - ref| + 2^-22.
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
    """round to the element type (RNE), back in t's dtype; el None / 'f32' (fp32-folded weights, nothing stored as 16 bits): identity"""
    return t if el in (None, "f32") else t.to(DTYPES[el]).to(t.dtype)


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

    # the recogniser's conv stack (a CRNN state dict)
    def r0(self):
        """FeatureExtraction.ConvNet.0 stays fp32: crnn_conv0_mfma_kernel's three-way split reproduces the weights exactly"""
        f = lambda k: torch.from_numpy(np.asarray(self.sd[k]).astype(np.float64))
        return f(_FE + "0.weight"), f(_FE + "0.bias")

    def r(self, k): return self.layer(*_REC_LAYERS[k])

    def upN(self, level):
        """(W_y, W_s, b) of upconv{level}'s 1x1 over cat[up(y), skip]"""
        w, b = self.layer(f"upconv{level}.conv.0", f"upconv{level}.conv.1")
        cy = {2: 256, 3: 128, 4: 64}[level]
        return w[:, :cy], w[:, cy:], b


_FE = "FeatureExtraction.ConvNet."
_REC_LAYERS = {1: (_FE + "3", None), 2: (_FE + "6", None), 3: (_FE + "8", None), 4: (_FE + "11", _FE + "12"), 5: (_FE + "14", _FE + "15"),
               6: (_FE + "18", None)}


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
    """(W_hh forward, W_hh backward) [1024, 256] fp64, rounded where pack_lstm_whh8 rounds them (el None / 'exact': the fp32 weights; the
    exact mode's split happens in lstm_dir)"""
    k = f"SequenceModeling.{layer}.rnn.weight_hh_l0"
    f = lambda s: rnd(torch.from_numpy(np.asarray(sd[s]).astype(np.float64)), None if el == "exact" else el)
    return f(k), f(k + "_reverse")


def lstm_dir(whh, x, reverse, el, q=True, dt=torch.float64, mut=None, pad_x=None, s=None, c0=None, c_out=None):
    """One direction of torch.nn.LSTM(256, 256) behind the input projection: x [n, T, 1024] = x W_ih^T + b_ih + b_hh (gate order i, f, g, o)
    -> the UNROUNDED h_t [n, T, 256] of every step; with q the value that crosses to the next step is rounded (h crosses LDS as 16 bits).
    pad_x [n, P, 1024] (mut 'bwd_padded_start'): rows behind the sequence that a backward pass started at the padded length would consume.
    el = 'exact' (lstm_exact_kernel): x is the fp32 input projection; with q, h (an fp32 register) crosses a step as the UNSCALED pair
    hi = fp16(h), lo = fp16(h - hi) and W_hh is split like pack_lstm_whh_split with the exponent s (one over both directions: bilstm passes
    it): pre = x + (h_hi w_hi + h_hi w_lo + h_lo w_hi) 2^-s; the returned h_t are the fp32 values the kernel stores as pairs.  Its mistakes:
    'h_lo_dropped', 'bwd_t_off_by_one' (the backward direction writes step t at row t - 1 and drops t = 0).
    c0: the initial cell state (the 'cell state carried into the next tile' mistake); c_out: a list that receives the final one."""
    n, T, _ = x.shape
    x = x.to(dt)
    split = el == "exact" and q
    if split:
        s, w_hi, _, w_lo = split_weights(whh, 1.0, split_exponent(whh) if s is None else s)
        w, wl, sc = w_hi.to(dt).t(), w_lo.to(dt).t(), 2.0 ** -s
    else:
        w = whh.to(dt).t()
    h = torch.zeros((n, 256), dtype=dt)
    hl = torch.zeros((n, 256), dtype=dt)
    c = torch.zeros((n, 256), dtype=dt) if c0 is None else c0.to(dt)
    out = torch.zeros((n, T, 256), dtype=dt)
    order = {"gate_order": (0, 2, 1, 3)}.get(mut, (0, 1, 2, 3))

    def step(xt, h, hl, c):
        pre = xt + ((h @ w + h @ wl + hl @ w) * sc if split else h @ w)
        gi, gf, gg, go = (pre[:, 256 * k:256 * (k + 1)] for k in order)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        hu = torch.sigmoid(go) * torch.tanh(c)
        if split:
            hu = hu.float()
            hi, lo = pair_encode(hu, 1.0)
            return hu.to(dt), hi.to(dt), (torch.zeros_like(hi) if mut == "h_lo_dropped" else lo).to(dt), c
        return hu, (hu if el == "exact" or not q else rnd(hu, el)), hl, c

    if mut == "bwd_padded_start" and reverse:
        for t in range(pad_x.shape[1] - 1, -1, -1):
            _, h, hl, c = step(pad_x[:, t].to(dt), h, hl, c)
    for k in range(T):
        t = T - 1 - k if reverse else k
        hu, h, hl, c = step(x[:, t], h, hl, c)
        tw = t - 1 if (mut == "bwd_t_off_by_one" and reverse) else t
        if tw >= 0:
            out[:, tw] = hu
    if c_out is not None:
        c_out.append(c)
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


def bilstm(whh_f, whh_b, x, el, q=True, dt=torch.float64, mut=None, pad_x=None, c0=None, c_out=None):
    """x [n, T, 2, 1024] (direction, gate * 256 + unit) -> [n, T, 512] (fwd | bwd).  el = 'exact' with q: as lstm_exact_kernel's pair store
    leaves it (lo scale 1); c0 = (fwd, bwd) initial cell states, c_out: a list that receives the final (fwd, bwd)"""
    if mut == "carry_c":
        return torch.cat([lstm_seq_carry_c(whh_f, x[:, :, 0], False, el, q, dt), lstm_seq_carry_c(whh_b, x[:, :, 1], True, el, q, dt)], dim=2)
    s = split_exponent(whh_f, whh_b) if el == "exact" else None
    cs = []
    o = torch.cat([lstm_dir(w, x[:, :, d], bool(d), el, q, dt, mut, None if pad_x is None else pad_x[:, :, d], s, None if c0 is None else c0[d], cs)
                   for d, w in enumerate((whh_f, whh_b))], dim=2)
    if c_out is not None:
        c_out.append(tuple(cs))
    return pair_roundtrip(o, 1.0) if (el == "exact" and q) else o


def refs_bilstm(whh_f, whh_b, x, el):
    """(ref_q, ref_nq, E).  el = 'exact': ref_q = the split recurrence in fp64, ref_nq = fp64 without any split, and E = the tile's bound
    8 max |fp32 - ref_nq| + 2^-22 with fp32 = the un-split recurrence in float32 (EXACT_RULE)"""
    rq, rn = bilstm(whh_f, whh_b, x, el, True), bilstm(whh_f, whh_b, x, el, False)
    if el == "exact":
        return rq, rn, lstm_exact_bound(rn, bilstm(whh_f, whh_b, x, el, False, torch.float32).double())
    return rq, rn, 2.0 * (rq - rn).abs().max().item()


# ------------------------------------------------------------------------------------------------ recogniser conv stack, one crop at a time
# Stage k of crnn_features_stages (recognizer.cpp): 0 conv0 + ReLU + pool | 1 r1 + pool | 2 r2 | 3 r3 + (2,1) pool | 4 r4 | 5 r5 + (2,1) pool |
# 6 r6 (2x2, no padding) | 7 mean over the 3 rows.  The kernels run every crop of a pass side by side in one wide image with REC_GAP zero
# columns between neighbours, cleared again after every layer.  The references know nothing of that: a crop is the image [1, C, H, imgW >> s]
# with ordinary zero padding, which is the statement "crops do not see each other".  The wide layout appears only in rec_wide_mut, the model of
# the named mistakes.
REC_GAP = 4
REC_STAGES = 8
REC_IN = [(64, 0, 1), (32, 1, 32), (16, 2, 64), (16, 2, 128), (8, 2, 128), (8, 2, 256), (4, 2, 256), (3, 2, 256)]     # stage input: H, log2 of the width's down-scale, C
REC_PART_A = [320] + [64] * 5 + [128] + [64] * 6 + [128] + [64] * 6       # 17 x 64, 2 x 128, 1 x 320 in box order: 1,744 columns, three buckets
REC_PART_B = [64]                                                          # 68 columns, T = 15: the smallest image any layer's tile code can see
REC_MUTS = [f"gap_uncleared@{k}" for k in range(6)] + [f"gap_shift@{k}" for k in range(6)] + \
    ["gap_first_only", "conv0_tap8", "conv0_pool_pair", "gather_plus1", "gather_T", "gather_rows_swapped", "mean_rows01"]


def rec_in_shape(k, imgW):
    """(H, W, C) of one crop's input of stage k; k = 8: the gathered rows (1, T, 256)"""
    if k == REC_STAGES:
        return 1, imgW // 4 - 1, 256
    H, s, C = REC_IN[k]
    return H, (imgW >> s) - (1 if k == 7 else 0), C


def rec_plan_like(widths):
    """rec_plan_part restated for the CPU suite and rec_wide_mut ONLY (the GPU tests take the layout from production and assert that it is
    this one): buckets by ascending width, box order kept inside a bucket -> (slot, row0, order, cols, rows) per plan position"""
    order = sorted(range(len(widths)), key=lambda i: (widths[i], i))
    slot, row0, cols, rows = [], [], 0, 0
    for i in order:
        slot.append(cols)
        row0.append(rows)
        cols += widths[i] + REC_GAP
        rows += widths[i] // 4 - 1
    return slot, row0, order, cols, rows


def rec_pixels(widths, seed, order=None):
    """the stage-0 inputs of the GPU tests: uint8 grey noise per crop [64, imgW], smoothed as in test_crnn_logits_fp16_and_exact; the first
    and last two columns of every crop are 255 and those of its neighbours in the wide image 0 (alternating by plan position), so a leak
    across a separator has something to carry.  order: the plan's (box of every plan position); the GPU tests pass production's, the CPU
    suite leaves it to rec_plan_like"""
    rng = np.random.default_rng(seed)
    if order is None:
        order = rec_plan_like(widths)[2]
    out = [None] * len(widths)
    for k, i in enumerate(order):
        g = rng.integers(0, 256, (64, widths[i]), dtype=np.uint8)
        g = ((g.astype(np.int32) + np.roll(g, 1, 1) + np.roll(g, 1, 0)) // 3).astype(np.uint8)
        g[:, :2] = g[:, -2:] = 0 if k & 1 else 255
        out[i] = torch.from_numpy(g)
    return out


def rec_normalise(g_u8, el):
    """ToTensor + sub_(0.5).div_(0.5) in fp32 as crop_final / crnn_conv0_kernel spell it, rounded to the element type ('f32': not at all)
    -> [1, 64, imgW, 1] fp64"""
    x = (g_u8.float() / 255.0 - 0.5) / 0.5
    return rnd(x, el).double()[None, :, :, None]


def rec_acts(widths, k, el, seed):
    """the inputs of the GPU tests for stage k >= 1 alone: non-negative (they follow a ReLU) random element-type activations per crop"""
    g = torch.Generator().manual_seed(seed)
    return [rnd(torch.randn((1,) + rec_in_shape(k, w), generator=g, dtype=torch.float64).abs(), el) for w in widths]


REC_SEED = 40
REC_RANGES = [(k, k) for k in range(REC_STAGES)] + [(k, k + 1) for k in range(6)] + [(0, 7)]      # what the GPU tests run: every stage alone,
# every cleared stage with its reader (a clear left out after stage k shows in stage k + 1's edge columns), the whole chain


def rec_inputs(widths, first, el, order=None):
    """the GPU tests' inputs of a range starting at stage `first`, per crop in box order, fp64 holding element-type values (order: rec_pixels)"""
    if first == 0:
        return [rec_normalise(g, el) for g in rec_pixels(widths, REC_SEED, order)]
    return rec_acts(widths, first, el, REC_SEED + first)


def rec_stage(W, k, x, dt=torch.float64, mut=None, absw=False):
    """stage k on ONE image x NHWC (a crop -- or, in rec_wide_mut, the wide image as one picture) -> NHWC, nothing rounded.
    absw: the stage's map with |W|, no bias and no ReLU (the propagation of the allowance E; max-pool and mean pass an error bound through)"""
    xc = nchw(x.to(dt))
    act = (lambda t: t) if absw else F.relu
    if k == 7:
        y = xc[:, :, :2].mean(dim=2, keepdim=True) if mut == "mean_rows01" else xc.mean(dim=2, keepdim=True)
        return nhwc(y)
    w, b = W.r0() if k == 0 else W.r(k)
    if k == 0 and mut == "conv0_tap8":
        w = w.clone()
        w[:, :, 2, 2] = 0
    y = act(conv(xc, w.abs(), None, pad=0 if k == 6 else 1) if absw else conv(xc, w, b, pad=0 if k == 6 else 1))
    if k == 0 and mut == "conv0_pool_pair":        # the max over columns (2x - 1, 2x)
        y = F.pad(y, (1, 0), value=float("-inf"))[..., :-1]
    if k in (0, 1):
        y = F.max_pool2d(y, 2)
    elif k in (3, 5):
        y = F.max_pool2d(y, (2, 1))
    return nhwc(y)


def rec_chain(W, x, first, last, el, q=True, dt=torch.float64, mut=None):
    """stages first..last on one crop; with q the value between two stages is rounded to the element type (it is stored as 16 bits)"""
    for k in range(first, last + 1):
        x = rec_stage(W, k, x, dt, mut)
        if q and k < last:
            x = rnd(x, el)
    return x


def refs_rec(W, x, first, last, el):
    """(ref_q, ref_nq, E) of stages first..last on one crop.  A stage alone is a single-rounding stage (max-pool and ReLU commute with the
    monotone rounding; stage 7 rounds the fp32 mean once): E = 0.  A chain: one element-type ulp of every value rounded between two stages,
    carried through the |W| maps behind it, as refs_c11 does.  Over seven layers that allowance is LOOSE (each layer multiplies it by its
    sum of |w|): the chain 0..7 guards placement -- gather rows, T, crop order, a crop taking its neighbour's columns -- and the single
    stages carry the numerical weight."""
    rq, rn = rec_chain(W, x, first, last, el, True), rec_chain(W, x, first, last, el, False)
    if first == last:
        return rq, rn, 0.0
    a, e = x.double(), None
    for k in range(first, last + 1):
        a = rec_stage(W, k, a)
        e = rec_stage(W, k, e, absw=True) if e is not None else torch.zeros_like(a)
        if k < last:
            e = e + ulp_el(a, el)
    return rq, rn, e


REC_SEP7 = 7.0


def rec_wide_pack(slots, cols, xs, k, dtype):
    """the crops xs (box order; slots: their first pixel columns) as the wide input of stage k, NHWC [1, H, W, C].  Separator columns are 0,
    as production guarantees -- except in front of stage 7: r6's output is never cleared (its separator columns mix a crop with the gap, or
    two crops), so there they hold REC_SEP7, for a gather that reads one to show"""
    H, s, C = REC_IN[k]
    wide = torch.full((1, H, (cols >> s) - (1 if k == 7 else 0), C), REC_SEP7 if k == 7 else 0.0, dtype=dtype)
    for x, sl in zip(xs, slots):
        wide[:, :, sl >> s:(sl >> s) + x.shape[2]] = x.to(dtype)
    return wide


def rec_wide_mut(W, widths, xs, first, last, el, mut, dt=torch.float64, want_wide=False):
    """What the WIDE-image code computes from the crops xs (box order) when it makes the mistake `mut` (None: none): the crops side by side
    with REC_GAP zero columns after each, every stage on that picture, the separator columns cleared after stages 0..5, the gather after 7;
    values between stages rounded as the kernels store them.  Returns the per-crop outputs in box order, in the crop's own shape."""
    slot, row0, order, cols, rows = rec_plan_like(widths)
    n = len(widths)
    by_crop = [0] * n
    for k, i in enumerate(order):
        by_crop[i] = slot[k]
    wide = rec_wide_pack(by_crop, cols, xs, first, dt)
    at = lambda m: mut is not None and mut == m
    for st in range(first, min(last, 6) + 1):
        wide = rec_stage(W, st, wide, dt, mut)
        if st < last:
            wide = rnd(wide, el)
        if st <= 5 and not at(f"gap_uncleared@{st}"):
            shift = 1 if st == 0 else 2
            gapw = 1 if at("gap_first_only") else 4 >> shift
            for k, i in enumerate(order):
                x0 = (slot[k] + widths[i]) >> (shift + 1 if at(f"gap_shift@{st}") else shift)
                wide[:, :, x0:x0 + gapw] = 0
    if want_wide:                                              # last < 7: the stage's whole output, separator columns included
        return wide
    if last < 7:
        s = REC_IN[last + 1][1]
        return [wide[:, :, slot[k] >> s:(slot[k] >> s) + rec_in_shape(last + 1, widths[i])[1]].clone() for k, i in sorted(enumerate(order), key=lambda t: t[1])]
    pad = list(row0)
    if at("gather_rows_swapped"):
        pad[0], pad[1] = pad[1], pad[0]
    m = rec_stage(W, 7, wide, dt, mut)[0, 0]                   # [Wc, 256]
    out = torch.zeros((rows + 1, 256), dtype=dt)
    for k in reversed(range(n)):                               # gather_T: a crop's extra row lands on its successor's first one; let it win
        T = widths[order[k]] // 4 - (0 if at("gather_T") else 1)
        xs0 = (slot[k] >> 2) + (1 if at("gather_plus1") else 0)
        out[pad[k]:pad[k] + T] = m[xs0:xs0 + T]
    res = [None] * n
    for k, i in enumerate(order):
        res[i] = out[row0[k]:row0[k] + widths[i] // 4 - 1][None, None].clone()
    return res


def rec_misplaced(got, ref, widths):
    """The chain's placement check, without a tolerance: got / ref = per-crop gathered rows [T, 256] in box order.  Crop i's rows must lie
    nearer (L2) to its own reference than to the reference of any other crop of its bucket, and nearer than to its own reference one time
    step earlier or later.  Returns the list of violations (empty: every crop's rows are where the plan says, in the plan's order)."""
    bad = []
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = g.reshape(-1, 256).double(), r.reshape(-1, 256).double()
        own = float((g - r).norm())
        for j, rj in enumerate(ref):
            if j != i and widths[j] == widths[i] and not own < float((g - rj.reshape(-1, 256).double()).norm()):
                bad.append(f"crop {i} (bucket {widths[i]}): its rows are no nearer to its own reference than to crop {j}'s")
        for name, a, b in (("later", g[1:] - r[:-1], g[1:] - r[1:]), ("earlier", g[:-1] - r[1:], g[:-1] - r[:-1])):
            if not float(b.norm()) < float(a.norm()):
                bad.append(f"crop {i} (bucket {widths[i]}): its rows match its reference one time step {name} at least as well")
    return bad


def rec_chain_cap(W, widths, xs, ref_q, el):
    """The cap of the chain 0..7 (check): twice the share of elements that torch-fp32 arithmetic on the wide image, values between stages and
    the output stored in the element type, leaves beyond the tight bound of this part's ref_q (flattened, rec_flat) -- or 1e-3 where that
    is larger.  Returns (cap, the stand-in's share)."""
    got = round_out(rec_flat(rec_wide_mut(W, widths, xs, 0, 7, el, None, torch.float32)), el)
    tight, _ = bounds(ref_q, ref_q, 0.0, el)
    share = float((~((got - ref_q).abs() <= tight)).double().mean())
    return max(1e-3, 2.0 * share), share


def rec_flat(ts):
    """per-crop tensors -> one vector (the rule is applied to a part as a whole)"""
    return torch.cat([(t if torch.is_tensor(t) else torch.zeros(())).reshape(-1).double() for t in ts])


def rec_where(flat_mask, widths, shapes, ids=None):
    """a mask over rec_flat's vector -> which crops it touches (ids: their box numbers, default 0, 1, ..): bucket, count, and the first
    element's row, channel and column with its distance from the crop's left and right edge"""
    out, at = [], 0
    for i, w, (H, Wc, C) in zip(ids or range(len(widths)), widths, shapes):
        m = flat_mask[at:at + H * Wc * C].reshape(H, Wc, C)
        at += H * Wc * C
        if m.any():
            y, x, c = [int(v[0]) for v in torch.nonzero(m, as_tuple=True)]
            cols = sorted(set(torch.nonzero(m.any(dim=2).any(dim=0)).flatten().tolist()))
            out.append(f"crop {i} (bucket {w}): {int(m.sum())} elements in columns {cols[:6]}{'...' if len(cols) > 6 else ''} of {Wc}, first at row {y}, "
                       f"column {x} ({x} from the left edge, {Wc - 1 - x} from the right), channel {c}")
    return "; ".join(out)


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


def check(got, ref_q, ref_nq, E, el_out, name="", beyond=None, index_names=("n", "y", "x", "c"), cap=1e-3):
    """Apply the rule; returns {'share', 'worst', 'ratio'} and raises AssertionError with a localised report.  got: fp64, same shape.
    cap: the largest share of elements that may miss the tight bound, 1e-3 -- except for the recogniser's chain 0..7, whose caller passes
    rec_chain_cap(): behind seven roundings ref_q is one of many equally valid outcomes (an intermediate value that lands on the other side
    of a rounding boundary moves everything behind it by an ulp), torch-fp32 arithmetic standing in for the kernel itself misses 1e-3 there,
    and the bound becomes twice that stand-in's own share -- taken from the reference arithmetic, never from a kernel."""
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
    if share > cap:
        problems.append(f"share beyond the tight bound {share:.3g} > {cap:.3g}")
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


# ================================================================================================ exact mode: pair tensors, split-fp16 plans
# (the rule for these stages is stated in EXACT_RULE below and quoted in the module docstring's last paragraph)
EXACT_RULE = """Rule for the exact mode's split-fp16 stages, per element:

  |got - ref| <= u |ref| + (2^-21 + 2 q32) S + 2^-35

ref   fp64 on the decoded inputs with the fp32-folded weights, no split;
S     the stage's linear map with absolute values, |W| * |x| + |b| (max-pool passes the bound of its window through);
u     2^-22 for a pair output (hi carries 11 bits, lo 11 bits of the residual), 2^-24 for an fp32 output;
2^-21 the representation's worst case: w_hi + w_lo holds w 2^s to 2^-22, the dropped a_lo w_lo term is at most 2^-11 2^-11;
q32   max |standin - ref| / S of the same case, standin = the launch's three product terms accumulated in float32, 32 products at a time in
      k order: it stands for fp32 accumulation, which has no useful worst-case bound, and is computed from the reference on the CPU, never
      from a kernel; the factor 2 is there because the MFMA's summation order inside a k-step is not the stand-in's.  The CPU suite asserts
      q32 <= 2^-22 on every case the GPU tests run.

pair_conv1_1 and pair_cls_tail are fp32 FMA chains: the same formula with standin = the float32 chain in the kernel's tap order; the
classifier tail's two maps (16 -> 16 -> 2) share one S = |W2| (|W1| |x| + |b1|) + |b2|, which is the first map's bound carried through |W2|.
ReLU, MaxPool(3,1,1) and the same-size upcat are selections: bit for bit.  The up-sampling upcat: 2^-22 |ref| + 2^-23 (the blend of the four
|neighbours|) against the fp64 blend.  The recurrence has no S: per tile, max |got - ref| <= 8 max |fp32 - ref| + 2^-22, fp32 = the same
recurrence in float32 without any split (three extra 2^-22 roundings per step -- h, W_hh, device expf / tanhf -- on top of fp32's own, and a
factor 2 for accumulation order)."""
SPLIT_LO = 2048.0
U_PAIR, U_F32, SPLIT_REP, SPLIT_ABS, Q32_MAX = 2.0 ** -22, 2.0 ** -24, 2.0 ** -21, 2.0 ** -35, 2.0 ** -22


def pair_encode(v32, lo_scale=SPLIT_LO):
    """fp32 values -> (hi, lo) fp16: hi = fp16(v), lo = fp16((v - hi) lo_scale), round to nearest even (v - hi and the power-of-two product are
    exact in fp32)"""
    v = v32.float()
    hi = v.to(torch.float16)
    return hi, ((v - hi.float()) * np.float32(lo_scale)).to(torch.float16)


def pair_value(hi, lo, lo_scale=SPLIT_LO, dt=torch.float64):
    """decode; dt = float32 is pair_load8's arithmetic (hi + lo * (1 / lo_scale)) and is exact for every pair pair_encode makes"""
    return hi.to(dt) + lo.to(dt) * (1.0 / lo_scale)


def pair_pack(v32, lo_scale=SPLIT_LO):
    """[.., C] fp32 values -> the pair tensor [.., C hi | C lo] fp16"""
    return torch.cat(pair_encode(v32, lo_scale), dim=-1)


def pair_halves(t):
    C = t.shape[-1] // 2
    return t[..., :C], t[..., C:]


def pair_decode(t, lo_scale=SPLIT_LO, dt=torch.float64):
    return pair_value(*pair_halves(t), lo_scale, dt)


def pair_roundtrip(v, lo_scale=SPLIT_LO):
    """the value a kernel's pair store leaves, fp64 (v is cast to fp32 first: the kernels split an fp32 register)"""
    return pair_value(*pair_encode(v.float(), lo_scale), lo_scale)


def split_exponent(*ws):
    """s of upload_split_plan / pack_lstm_whh_split: 2^9 <= max |w| 2^s < 2^10, clamped to [-14, 24]"""
    mx = max(float(w.abs().max()) for w in ws)
    s = 9 - int(np.floor(np.log2(mx))) if mx > 0 else 0
    return max(-14, min(24, s))


def split_weights(w, lo_scale=SPLIT_LO, s=None):
    """w (fp32 values) -> (s, w_hi, w_mid, w_lo) fp64: w_hi = fp16(w 2^s), w_lo = fp16(w 2^s - w_hi), and the block the lo activations meet,
    w_mid = fp16(w_hi / lo_scale) (the packer rounds every block to fp16; for lo_scale 1 it is w_hi)"""
    s = split_exponent(w) if s is None else s
    v = w.float() * np.float32(2.0 ** s)
    hi = v.to(torch.float16).float()
    lo = (v - hi).to(torch.float16).float()
    mid = (hi * np.float32(1.0 / lo_scale)).to(torch.float16).float()
    return s, hi.double(), mid.double(), lo.double()


def _k_order(t):
    """[A, C, T, ...] -> [A, T * C, ...]: k runs over the taps, inside a tap over the channels [a_hi | a_lo | a_hi]"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[1] * t.shape[2], *t.shape[3:])


def split_conv(w, b, a_pair, pad=0, dil=1, lo_scale=SPLIT_LO, w_lo_scale=None, mut=None):
    """A split plan's launch on the pair tensor a_pair [N, H, W, C | C] (lo stored x lo_scale), before its epilogue: NCHW pre-activations
    {'ref', 'model', 'standin', 'S'}.  w [Cout, C, K, K], b: fp64 tensors of fp32 values.  w_lo_scale: what the plan was PACKED for (a mistake
    when it differs from lo_scale).  mut: 'drop_a_lo', 'drop_w_lo', 'mid_unscaled', 'no_acc_scale' -- None for the launch itself."""
    hi, lo = pair_halves(a_pair)
    ah, al = nchw(hi.double()), nchw(lo.double())                     # al: the STORED lo half
    x = ah + al / lo_scale
    s, wh, wm, wl = split_weights(w, lo_scale if w_lo_scale is None else w_lo_scale)
    if mut == "mid_unscaled":
        wm = wh
    if mut == "drop_a_lo":
        wm = torch.zeros_like(wm)
    if mut == "drop_w_lo":
        wl = torch.zeros_like(wl)
    sc = 1.0 if mut == "no_acc_scale" else 2.0 ** -s
    ref = conv(x, w, b, pad=pad, dil=dil)
    S = conv(x.abs(), w.abs(), b.abs(), pad=pad, dil=dil)
    model = (conv(ah, wh, None, pad, dil) + conv(al, wm, None, pad, dil) + conv(ah, wl, None, pad, dil)) * sc + b[None, :, None, None]
    # the stand-in: float32, the three terms as ONE k sequence, a partial sum of 32 products added to the accumulator at a time
    K = w.shape[-1]
    cols = F.unfold(torch.cat([ah, al, ah], dim=1).float(), K, dilation=dil, padding=pad)          # [N, 3C * T, L], channel-major
    N, C3 = cols.shape[0], 3 * ah.shape[1]
    cols = _k_order(cols.reshape(N, C3, K * K, -1))
    wk = _k_order(torch.cat([wh, wm, wl], dim=1).float().reshape(w.shape[0], C3, K * K))
    acc = torch.zeros((N, w.shape[0], cols.shape[-1]), dtype=torch.float32)
    for k in range(0, wk.shape[1], 32):
        acc = acc + torch.matmul(wk[None, :, k:k + 32], cols[:, k:k + 32])
    standin = (acc * np.float32(sc) + b.float()[None, :, None]).reshape(ref.shape).double()
    return {"ref": ref, "model": model, "standin": standin, "S": S}


def split_epilogue(y, relu_out, pool, pool_relu, keep_full, store=True, mut=None):
    """The conv epilogue on NCHW pre-activations -> {'full': .., 'pool': ..} NHWC (the outputs the row writes).  store: the value goes through
    an fp32 register and the pair store (model, standin, got); False: nothing is rounded (ref, S: max-pool passes a bound through).
    mut 'pool_split_first': the four values are split before the max, which is then taken on hi and lo separately."""
    full = F.relu(y) if relu_out else y
    if store:
        full = full.float().double()
    out = {}
    if keep_full or not pool:
        out["full"] = nhwc(pair_roundtrip(full) if store else full)
    if pool:
        if mut == "pool_split_first":
            hi, lo = pair_encode(full.float())
            p = pair_value(F.max_pool2d(hi.float(), 2).half(), F.max_pool2d(lo.float(), 2).half())
            out["pool"] = nhwc(F.relu(p) if pool_relu else p)
            return out
        p = F.max_pool2d(full, 2)
        p = F.relu(p) if pool_relu else p
        out["pool"] = nhwc(pair_roundtrip(p) if store else p)
    return out


def split_bound(ref, S, q32, u):
    return u * ref.abs() + (SPLIT_REP + 2.0 * q32) * S + SPLIT_ABS


def split_q32(standin_val, ref, S):
    """max |standin - ref| / S over the elements with S > 0 (standin_val: the stand-in's fp32 value BEFORE the output store)"""
    m = S > 0
    return float(((standin_val - ref).abs()[m] / S[m]).max()) if m.any() else 0.0


def split_check(got, ref, S, q32, u, name=""):
    """apply the rule -> {'worst': max |got - ref| / bound, 'q32', 'kernel': max |got - ref| / S}; AssertionError with a localised report"""
    got = got.double()
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    finite = torch.isfinite(got)
    bound = split_bound(ref, S, q32, u)
    d = (got - ref).abs()
    rel = torch.where(finite, d / bound, torch.full_like(d, float("inf")))
    m = S > 0
    stats = {"worst": float(rel.max()), "q32": q32, "kernel": float((d[m & finite] / S[m & finite]).max()) if (m & finite).any() else 0.0}
    print(f"[stage] {name}: max |got - ref| / bound {stats['worst']:.3g}, q32 {q32:.3g}, kernel max |got - ref| / S {stats['kernel']:.3g}")
    miss = ~(d <= bound)
    if miss.any():
        w = int(torch.argmax(rel))
        idx = np.unravel_index(w, tuple(got.shape))
        msg = f"{name}: {int(miss.sum())} of {miss.numel()} elements beyond the bound ({int((~finite).sum())} non-finite); worst at {tuple(int(v) for v in idx)}: got " \
              f"{got.flatten()[w].item():.9g}, ref {ref.flatten()[w].item():.9g}, bound {bound.flatten()[w].item():.3g}, S {S.flatten()[w].item():.3g}"
        if got.dim() == 4:
            msg += f"; by region {localise(miss)}"
        raise AssertionError(msg)
    return stats


def split_fails(mutated, ref, S, q32, u):
    return bool(((mutated.double() - ref).abs() > split_bound(ref, S, q32, u)).any())


# The conv launches of craft_forward_exact, in its order (detector.cpp's table; the GPU suite asserts that production's rows equal these):
# name, conv, bn, relu_out, store, pool, pool_relu, keep_full, K, dilation, input may be negative (its producer has no ReLU)
EXACT_CONVS = [
    ("conv1_2", "basenet.slice1.3", "basenet.slice1.4", True, 64, 1, False, False, 3, 1, False),
    ("conv2_1", "basenet.slice1.7", "basenet.slice1.8", True, 128, 0, False, False, 3, 1, False),
    ("conv2_2", "basenet.slice1.10", "basenet.slice1.11", False, 128, 1, True, True, 3, 1, False),
    ("conv3_1", "basenet.slice2.14", "basenet.slice2.15", True, 256, 0, False, False, 3, 1, False),
    ("conv3_2", "basenet.slice2.17", "basenet.slice2.18", False, 256, 0, False, False, 3, 1, False),
    ("conv3_3", "basenet.slice3.20", "basenet.slice3.21", True, 256, 1, False, False, 3, 1, False),
    ("conv4_1", "basenet.slice3.24", "basenet.slice3.25", True, 512, 0, False, False, 3, 1, False),
    ("conv4_2", "basenet.slice3.27", "basenet.slice3.28", False, 512, 0, False, False, 3, 1, False),
    ("conv4_3", "basenet.slice4.30", "basenet.slice4.31", True, 512, 1, False, False, 3, 1, False),
    ("conv5_1", "basenet.slice4.34", "basenet.slice4.35", True, 512, 0, False, False, 3, 1, False),
    ("conv5_2", "basenet.slice4.37", "basenet.slice4.38", False, 512, 0, False, False, 3, 1, False),
    ("fc6", "basenet.slice5.1", None, False, 1024, 0, False, False, 3, 6, True),
    ("fc7", "basenet.slice5.2", None, False, 1024, 0, False, False, 1, 1, True),
    ("up1a", "upconv1.conv.0", "upconv1.conv.1", True, 512, 0, False, False, 1, 1, True),
    ("up1b", "upconv1.conv.3", "upconv1.conv.4", True, 256, 0, False, False, 3, 1, False),
    ("up2a", "upconv2.conv.0", "upconv2.conv.1", True, 256, 0, False, False, 1, 1, True),
    ("up2b", "upconv2.conv.3", "upconv2.conv.4", True, 128, 0, False, False, 3, 1, False),
    ("up3a", "upconv3.conv.0", "upconv3.conv.1", True, 128, 0, False, False, 1, 1, True),
    ("up3b", "upconv3.conv.3", "upconv3.conv.4", True, 64, 0, False, False, 3, 1, False),
    ("up4a", "upconv4.conv.0", "upconv4.conv.1", True, 64, 0, False, False, 1, 1, True),
    ("up4b", "upconv4.conv.3", "upconv4.conv.4", True, 32, 0, False, False, 3, 1, False),
    ("cls0", "conv_cls.0", None, True, 32, 0, False, False, 3, 1, False),
    ("cls2", "conv_cls.2", None, True, 32, 0, False, False, 3, 1, False),
    ("cls4", "conv_cls.4", None, True, 16, 0, False, False, 3, 1, False),
]
EXACT_ROW = {r[0]: i for i, r in enumerate(EXACT_CONVS)}
# what the GPU tests run through the table: row, (N, H, W) at the layer's own resolution, and the route launch_conv_el takes for it
EXACT_CONV_CASES = [
    ("conv1_2", (1, 16, 16), "3x3 DMA, BN 64, pooled shared epilogue (one exact tile)"),
    ("conv1_2", (3, 34, 50), "3x3 DMA, BN 64, pooled shared epilogue (ragged, odd tile counts, pages 2 and 3)"),
    ("conv2_2", (2, 18, 30), "3x3 DMA, BN 128, pooled shared epilogue with store_full + pool_relu"),
    ("conv3_1", (1, 19, 37), "3x3 DMA, BN 128, two cout tiles, relu_out"),
    ("fc6", (1, 2, 2), "sub-lattice (LH = 1, most phases hold no pixel)"),
    ("fc6", (2, 15, 20), "sub-lattice (phases of 3 and of 2 rows, two pages stacked)"),
    ("fc6", (1, 13, 6), "sub-lattice (width below the dilation)"),
    ("fc7", (2, 7, 5), "1x1 DMA, K = 3 x 1,024"),
    ("up1a", (1, 2, 2), "1x1 DMA, K = 4,608"),
    ("up1a", (3, 7, 5), "1x1 DMA, K = 4,608"),
    ("up4b", (2, 16, 32), "3x3 DMA, 16x16 tiles, <= 32-cout route (64 -> 32: store 32, six k-chunks)"),
    ("up4b", (2, 18, 30), "3x3 DMA, BN 64, 8x32 tiles (10x34 patch: the three-deep ring, not the <= 32-cout instantiation)"),
    ("cls4", (1, 16, 16), "3x3 DMA, 16x16 tiles, <= 32-cout route (32 -> 16, store 16, pair pixel stride 32)"),
    ("cls4", (2, 24, 40), "3x3 DMA, 16x16 tiles, <= 32-cout route (32 -> 16, store 16, pair pixel stride 32)"),
]


def exact_conv_input(name, shape, cin, signed):
    """the GPU tests' input of a table row: a random pair tensor [N, H, W, cin | cin], negative values only where the producer has no ReLU"""
    N, H, W = shape
    g = torch.Generator().manual_seed(900 + EXACT_ROW[name] * 16 + N * H * W % 13)
    v = torch.randn((N, H, W, cin), generator=g)
    return pair_pack(v if signed else v.abs())


def exact_conv_case(W, name, shape, mut=None, cout=None):
    """One table row on the GPU tests' input -> (a_pair, {output name: {'ref', 'model', 'standin', 'S', 'q32'}}), outputs NHWC fp64.
    W: Weights(sd, 'f32').  cout: only the first `cout` output channels (the sensitivity tests' shortcut; a subset that fails is a failure)."""
    _, ck, bk, relu_out, store, pool, pool_relu, keep_full, K, dil, signed = EXACT_CONVS[EXACT_ROW[name]]
    w, b = W.layer(ck, bk)
    a_pair = exact_conv_input(name, shape, w.shape[1], signed)
    if cout:
        w, b = w[:cout], b[:cout]
    pad = dil if K == 3 else 0
    pre = split_conv(w, b, a_pair, pad, dil, mut=None if mut == "pool_split_first" else mut)
    epi = lambda y, st, m=None: split_epilogue(y, relu_out, pool, pool_relu, keep_full, st, m)
    ref, S = epi(pre["ref"], False), split_epilogue(pre["S"], False, pool, False, keep_full, False)
    model, standin = epi(pre["model"], True, mut if mut == "pool_split_first" else None), epi(pre["standin"], True)
    sval = split_epilogue(pre["standin"], relu_out, pool, pool_relu, keep_full, False)          # the stand-in's fp32 value before the store
    return a_pair, {k: {"ref": ref[k], "model": model[k], "standin": standin[k], "S": S[k], "q32": split_q32(sval[k], ref[k], S[k])} for k in ref}


# ------------------------------------------------------------------------------------------------ exact mode: element-wise pair kernels
def pair_relu(t, mut=None):
    """decode (fp32) -> max(v, 0) -> encode.  mut 'halves': ReLU taken on hi and lo separately"""
    if mut == "halves":
        return torch.clamp(t.float(), min=0).half()
    return pair_pack(torch.clamp(pair_decode(t, dt=torch.float32), min=0))


def pair_pool5(t, mut=None):
    """MaxPool2d(3, 1, 1) on the decoded fp32 values of a pair tensor [N, H, W, C | C].  mut 'halves': on hi and lo separately"""
    if mut == "halves":
        return nhwc(F.max_pool2d(nchw(t.float()), 3, 1, 1)).half()
    return pair_pack(nhwc(F.max_pool2d(nchw(pair_decode(t, dt=torch.float32)), 3, 1, 1)))


def pair_plane(shape, seed):
    """the selection kernels' input: a pair tensor [N, H, W, 512 | 512] with values of both signs and pairs whose halves have opposite signs;
    channel 0 holds ONE hi (1.0) with a lo that grows strictly along the scan order, so in every window the maximum by hi alone (a tie: the
    first pixel wins) is not the maximum by value (the last pixel)"""
    N, H, W = shape
    v = (torch.rand((N, H, W, 512), generator=torch.Generator().manual_seed(seed)) * 8 - 4).float()
    v[..., 0] = 1.0 + (torch.arange(H * W, dtype=torch.float32).reshape(1, H, W) - H * W / 2) / (H * W) * np.float32(1.9 * 2.0 ** -12)
    t = pair_pack(v)
    hi, lo = pair_halves(t)
    assert (hi[..., 0] == 1.0).all() and lo[0, ..., 0].unique().numel() == H * W
    assert ((hi.float() > 0) & (lo.float() < 0)).any() and ((hi.float() < 0) & (lo.float() > 0)).any()
    return t


def upcat_same_inputs(shape):
    """the same-size upcat cases' inputs: (f7-like pair [N, H, W, 1024 | 1024], s4-like pair [N, H, W, 512 | 512])"""
    N, H, W = shape
    g = torch.Generator().manual_seed(710)
    return pair_pack(torch.randn((N, H, W, 1024), generator=g) * 3), pair_pack(torch.randn((N, H, W, 512), generator=g) * 3)


def pair_upcat_same(y, skip, mut=None):
    """torch.cat([y, skip], dim = channels) of two pair tensors of one size (upcat(f7, s4)): decode -> encode of every value.
    mut 'halves_swapped': the skip's channels in front"""
    a, b = pair_decode(y, dt=torch.float32), pair_decode(skip, dt=torch.float32)
    return pair_pack(torch.cat([b, a] if mut == "halves_swapped" else [a, b], dim=-1))


def _up2_matrix(h, clamp0=True):
    """[2h, h]: torch's upsample_bilinear2d (scale 2, align_corners = False) along one axis; clamp0 False: the source index is not clamped at 0
    (dst 0 -> src -0.25, truncated to 0 with weight -0.25 on the neighbour; with h = 1 the neighbour is the pixel itself and nothing changes)"""
    M = torch.zeros((2 * h, h), dtype=torch.float64)
    for d in range(2 * h):
        sx = (d + 0.5) * 0.5 - 0.5
        if clamp0:
            sx = max(sx, 0.0)
        x0 = int(sx)
        x1 = x0 + (1 if x0 < h - 1 else 0)
        M[d, x0] += 1.0 - (sx - x0)
        M[d, x1] += sx - x0
    return M


def pair_upcat_up(y, mut=None):
    """the up-sampled half of upcat: decoded y [N, h, w, C] -> (fp64 blend [N, 2h, 2w, C], the blend of |y|: what the bound is taken from).
    mut 'edge_unclamped' / 'src_unclamped': upsample2's far-edge mistake / the source index not clamped at 0"""
    v = nchw(pair_decode(y))
    if mut == "src_unclamped":
        u = torch.einsum("ah,nchw,bw->ncab", _up2_matrix(v.shape[2], False), v, _up2_matrix(v.shape[3], False))
    else:
        u = upsample2(v, mut)
    return nhwc(u), nhwc(upsample2(v.abs()))


def upcat_up_bound(ref, blend_abs):
    return U_PAIR * ref.abs() + 2.0 ** -23 * blend_abs


# ------------------------------------------------------------------------------------------------ exact mode: conv1_1 and the classifier tail
C11_GEOMS = [(17, 33, 32, 64), (32, 32, 32, 32), (1, 1, 32, 32), (50, 70, 64, 96)]      # (Himg, Wimg, H32, W32)


def c11_pages(geom, N, content):
    """the pages of the exact conv1_1 cases, uint8 [N, Himg, Wimg, 3]: 'zeros', 'white', or 'random' = every channel of every pixel 0 or 255
    at random (seeded): per-pixel random, so a shifted or swapped tap shows, and with two input levels the float32 chain's q32 stays
    <= 2^-22 on all four geometries (the CPU suite asserts it)"""
    Hi, Wi = geom[:2]
    if content == "random":
        return torch.randint(0, 2, (N, Hi, Wi, 3), generator=torch.Generator().manual_seed(100 + Hi), dtype=torch.uint8) * 255
    return torch.full((N, Hi, Wi, 3), 255 if content == "white" else 0, dtype=torch.uint8)


def exact_c11(W, rgb_u8, Himg, Wimg, H32, W32, mut=None):
    """pair_conv1_1 -> {'ref', 'standin', 'S'} NHWC [N, H32, W32, 64] (ref: fp64 on the fp32-normalised canvas, ReLU'd; standin: the float32
    FMA chain from the bias over k = (ky 3 + kx) 3 + ch, ReLU'd, BEFORE the pair store).  mut 'canvas_as_padding': a canvas pixel beyond the
    page enters as the conv's zero padding instead of the normalised raw zero"""
    xn = normalise(rgb_u8, Himg, Wimg, H32, W32, "f32", True, torch.float32, "canvas_norm0" if mut == "canvas_as_padding" else None).double()
    w, b = W.c11()
    ref = F.relu(conv(xn, w, b, pad=1))
    S = conv(xn.abs(), w.abs(), b.abs(), pad=1)
    cols = F.unfold(xn.float(), 3, padding=1).reshape(xn.shape[0], 3, 9, -1)                     # [N, ch, tap, L]
    acc = b.float()[None, :, None].expand(xn.shape[0], 64, cols.shape[-1]).clone()
    w32 = w.float().reshape(64, 3, 9)
    for tap in range(9):
        for ch in range(3):
            acc = _fma32(w32[None, :, ch, tap, None], cols[:, None, ch, tap], acc)
    standin = F.relu(acc).reshape(ref.shape).double()
    return {"ref": nhwc(ref), "standin": nhwc(standin), "S": nhwc(S)}


def _fma32(a, b, c):
    """fmaf on float32 tensors: the product and the sum in fp64 (exact for fp32 operands up to one rounding of the sum: 48-bit product + 24-bit
    addend rounded to 53 bits, then to 24 -- a double rounding that differs from fmaf in at most a vanishing share of cases, inside the factor
    2 the rule puts on q32)"""
    return (a.double() * b.double() + c.double()).float()


def exact_cls_tail(W, c3_pair, mut=None):
    """pair_cls_tail on conv_cls.4's pair [N, H, W, 16 | 16] -> {'ref', 'standin', 'S'} [N, H, W, 2]: heat = W2 relu(W1 v + b1) + b2, everything
    fp32 in the kernel; S = |W2| (|W1| |v| + |b1|) + |b2|"""
    sd = W.sd
    f = lambda k: torch.from_numpy(np.asarray(sd[k]).astype(np.float64))
    w1, b1, w2, b2 = f("conv_cls.6.weight").reshape(16, 16), f("conv_cls.6.bias"), f("conv_cls.8.weight").reshape(2, 16), f("conv_cls.8.bias")
    v = pair_decode(c3_pair)
    h = F.relu(v @ w1.t() + b1)
    ref = h @ w2.t() + b2
    S = (v.abs() @ w1.abs().t() + b1.abs()) @ w2.abs().t() + b2.abs()
    v32 = v.float()
    p = b2.float().expand(*v.shape[:-1], 2).clone()
    for o in range(16):
        hh = b1.float()[o].expand(v.shape[:-1]).clone()
        for k in range(16):
            hh = _fma32(w1.float()[o, k], v32[..., k], hh)
        hh = F.relu(hh)
        p = torch.stack([_fma32(w2.float()[0, o], hh, p[..., 0]), _fma32(w2.float()[1, o], hh, p[..., 1])], dim=-1)
    return {"ref": ref, "standin": p.double(), "S": S}


# ------------------------------------------------------------------------------------------------ exact mode: the network composed
def exact_forward(W, rgb_u8, Himg, Wimg, H32, W32, dt=torch.float64):
    """craft_forward_exact's operation order on un-split values, the conv launches taken from EXACT_CONVS row by row -> (heat NHWC, u4b NCHW).
    With W = Weights(sd, None) this is oracle.nets.CRAFT in double (the CPU suite's composition test, which also proves the table's order)."""
    rows = iter(EXACT_CONVS)

    def cv(x):
        _, ck, bk, relu_out, _, pool, pool_relu, keep_full, K, dil, _ = next(rows)
        w, b = W.layer(ck, bk)
        y = conv(x, w, b, pad=dil if K == 3 else 0, dil=dil)
        full = F.relu(y) if relu_out else y
        if not pool:
            return full
        p = F.max_pool2d(full, 2)
        p = F.relu(p) if pool_relu else p
        return (p, full) if keep_full else p

    up = lambda y, skip: torch.cat([y if y.shape[2:] == skip.shape[2:] else upsample2(y), skip], dim=1)
    xn = normalise(rgb_u8, Himg, Wimg, H32, W32, None, False, dt)
    w, b = W.c11()
    x0 = F.relu(conv(xn, w, b, pad=1))
    p1 = cv(x0)
    a3 = cv(p1)
    p2, s1 = cv(a3)
    s2 = cv(cv(p2))
    p3 = cv(F.relu(s2))
    s3 = cv(cv(p3))
    p4 = cv(F.relu(s3))
    s4 = cv(cv(p4))
    f7 = cv(cv(F.max_pool2d(s4, 3, 1, 1)))
    u1b = cv(cv(up(f7, s4)))
    u2b = cv(cv(up(u1b, s3)))
    u3b = cv(cv(up(u2b, s2)))
    u4b = cv(cv(up(u3b, s1)))
    c3 = cv(cv(cv(u4b)))
    assert next(rows, None) is None
    w1, b1, w2, b2 = W.tail()
    return nhwc(conv(F.relu(conv(c3, w1, b1)), w2, b2)), u4b


# ------------------------------------------------------------------------------------------------ exact mode: sequence half
def seq_gemm_weights(sd, which, layer, perm=None):
    """(w [Cout, K, 1, 1], b, lo_scale of the INPUT pair) of the sequence half's GEMMs as weights.cpp builds them: which 0 xproj (both directions,
    rows permuted by perm = lstm8_xproj_channel; bias = b_ih + b_hh in fp32), 1 lin (the input is the LSTM's pair: lo unscaled), 2 pred"""
    f = lambda k: torch.from_numpy(np.asarray(sd[k]).astype(np.float32))
    sm = f"SequenceModeling.{layer}."
    if which == 0:
        w = torch.zeros((2048, 256), dtype=torch.float32)
        b = torch.zeros(2048, dtype=torch.float32)
        for d, sfx in enumerate(("", "_reverse")):
            w[perm[d * 1024:(d + 1) * 1024]] = f(sm + "rnn.weight_ih_l0" + sfx)
            b[perm[d * 1024:(d + 1) * 1024]] = f(sm + "rnn.bias_ih_l0" + sfx) + f(sm + "rnn.bias_hh_l0" + sfx)
        lo = SPLIT_LO
    elif which == 1:
        w, b, lo = f(sm + "linear.weight"), f(sm + "linear.bias"), 1.0
    else:
        w, b, lo = f("Prediction.weight"), f("Prediction.bias"), SPLIT_LO
    return w.double()[:, :, None, None], b.double(), lo


def lstm_exact_bound(ref, fp32):
    """the recurrence's bound of a tile (EXACT_RULE); refs_bilstm(.., 'exact') returns it as its allowance"""
    return 8.0 * float((fp32 - ref).abs().max()) + 2.0 ** -22


EXACT_TILES = lambda cap: [(cap, 15), (3, 79), (1, 15), (cap, 255), (5, 639)]


def exact_lstm_inputs(cap, layer, sigma):
    """the GPU test's fp32 input projections per tile [n, T, 2, 1024]"""
    gen = torch.Generator().manual_seed(850 + layer)
    return [(torch.randn((n, T, 2, 1024), generator=gen) * sigma).float() for n, T in EXACT_TILES(cap)]


# ------------------------------------------------------------------------------------------------ exact mode: models of the named mistakes
def fc6_phase_model(w, b, x, mut=None, d=6):
    """The dilated 3x3 (padding = dilation d) the way the sub-lattice path walks it: d * d plain 3x3 convs, one per phase image
    x[:, :, py::d, px::d], the phase images of a page stacked along y in the order q = py d + px with ONE shared zero row between neighbours.
    x NCHW fp64 -> NCHW.  mut None reproduces conv(x, w, b, pad = d, dil = d); the mistakes:
    'row_beyond'        a phase with fewer rows than LH = ceil(H / d) reads its missing row from memory: the rows behind the page (the next
                        page's first rows; zeros behind the last page) instead of treating it as padding
    'separator_nonzero' the shared row between two stacked phase images holds the neighbour's edge row instead of zero
    'page_offset'       the phase images of pages >= 1 are taken one phase image further along the stack"""
    N, Cc, H, Wd = x.shape
    LH = -(-H // d)
    behind = torch.cat([x, torch.zeros_like(x[:1])])[1:]                         # page n + 1 (zeros behind the last)
    subs = [x[:, :, q // d::d, q % d::d] for q in range(d * d)]

    def like(t, ref):                                                            # crop / zero-pad t to ref's spatial shape
        t = t[:, :, :ref.shape[2], :ref.shape[3]]
        return F.pad(t, (0, ref.shape[3] - t.shape[3], 0, ref.shape[2] - t.shape[2]))

    y = torch.zeros((N, w.shape[0], H, Wd), dtype=x.dtype)
    for q, sub in enumerate(subs):
        py, px = q // d, q % d
        lh, lw = sub.shape[2:]
        if lw == 0 or lh == 0:
            continue
        src = sub
        if mut == "page_offset" and N > 1:
            src = torch.cat([sub[:1], like(subs[(q + 1) % (d * d)][1:], sub)])
        p = F.pad(src, (1, 1, 1, 1))
        if mut == "row_beyond" and lh < LH and lh * d + py - H < H:
            p[:, :, -1, 1:-1] = behind[:, :, lh * d + py - H, px::d]
        if mut == "separator_nonzero":
            if q + 1 < d * d and subs[q + 1].shape[2] > 0:
                p[:, :, -1:, 1:-1] = like(subs[q + 1][:, :, :1], src[:, :, :1])
            if q > 0 and subs[q - 1].shape[2] > 0:
                p[:, :, :1, 1:-1] = like(subs[q - 1][:, :, -1:], src[:, :, :1])
        y[:, :, py::d, px::d] = conv(p, w, b)
    return y


# ------------------------------------------------------------------------------------------------ exact mode: the recogniser's conv stack, a stage alone
def exact_rec_inputs(widths, k, order=None):
    """the GPU tests' input of stage k alone, per crop in box order: k = 0 the fp32-normalised pixels [1, 64, w, 1] (fp64 values; the device gets
    the codes 1 + grey of rec_pixels); k >= 1 a pair tensor [1, H, w', C | C] of non-negative values (every producer ends on a ReLU)"""
    if k == 0:
        return [rec_normalise(g, "f32") for g in rec_pixels(widths, REC_SEED, order)]
    g = torch.Generator().manual_seed(REC_SEED + 100 + k)
    return [pair_pack(torch.randn((1,) + rec_in_shape(k, w), generator=g).abs()) for w in widths]


def rec_wide_pack_pair(slots, cols, xs, k):
    """pair tensors of the crops (box order; slots: their first pixel columns) as the wide input of stage k >= 1, [H, W, C | C] fp16; separator
    columns +0, in front of stage 7 the value REC_SEP7 (rec_wide_pack)"""
    H, s, C = REC_IN[k]
    wide = torch.zeros((H, (cols >> s) - (1 if k == 7 else 0), 2 * C), dtype=torch.float16)
    if k == 7:
        wide[..., :C] = REC_SEP7
    for x, sl in zip(xs, slots):
        wide[:, sl >> s:(sl >> s) + x.shape[2]] = x[0]
    return wide


def exact_rec_stage(W, k, x, mut=None):
    """stage k of crnn_features_stages on ONE crop in the exact mode -> NHWC {'ref', 'model', 'standin', 'sval', 'S'} (sval: the stand-in's fp32
    value before the pair store).  k = 0: crnn_conv0_kernel<REC_SPLIT>, a float32 chain of 9 FMAs from the bias in tap order, ReLU, 2x2 max;
    1..6: split plans r1..r6 + ReLU (+ the pools of rec_stage); 7: ((a + b) + c) / 3 in float32 on the decoded rows."""
    pool = {0: 2, 1: 2, 3: (2, 1), 5: (2, 1)}.get(k)
    post = lambda y: F.max_pool2d(F.relu(y), pool) if pool else F.relu(y)
    if k == 7:
        v = nchw(pair_decode(x))
        v32 = v.float()
        sval = (((v32[:, :, 0] + v32[:, :, 1]) + v32[:, :, 2]) / np.float32(3.0))[:, :, None].double()
        out = {"ref": v.mean(dim=2, keepdim=True), "model": sval, "sval": sval, "S": v.abs().mean(dim=2, keepdim=True)}
    elif k == 0:
        w, b = W.r0()
        xc = nchw(x.double())
        cols = F.unfold(xc.float(), 3, padding=1)                                   # [1, 9, L], tap = ky 3 + kx
        acc = b.float()[None, :, None].expand(1, 32, cols.shape[-1]).clone()
        w32 = w.float().reshape(32, 9)
        for tap in range(9):
            acc = _fma32(w32[None, :, tap, None], cols[:, None, tap], acc)
        sval = post(acc.reshape(1, 32, xc.shape[2], xc.shape[3])).double()
        out = {"ref": post(conv(xc, w, b, pad=1)), "model": sval, "sval": sval,
               "S": F.max_pool2d(conv(xc.abs(), w.abs(), b.abs(), pad=1), pool)}
    else:
        w, b = W.r(k)
        pre = split_conv(w, b, x, pad=0 if k == 6 else 1, mut=mut)
        out = {"ref": post(pre["ref"]), "model": post(pre["model"].float().double()), "sval": post(pre["standin"]),
               "S": F.max_pool2d(pre["S"], pool) if pool else pre["S"]}
    out["standin"] = pair_roundtrip(out["sval"])
    out["model"] = pair_roundtrip(out["model"])
    return {n: nhwc(t) for n, t in out.items()}


def exact_rec_part(W, k, xs, mut=None):
    """exact_rec_stage over the crops of a part, flattened (rec_flat) -> dict of vectors + 'q32' of the part + per-crop output shapes"""
    per = [exact_rec_stage(W, k, x, mut) for x in xs]
    out = {n: rec_flat([p[n] for p in per]) for n in per[0]}
    out["q32"] = split_q32(out["sval"], out["ref"], out["S"])
    out["shapes"] = [tuple(p["ref"].shape[1:]) for p in per]
    return out
