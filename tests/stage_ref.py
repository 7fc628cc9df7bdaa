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
