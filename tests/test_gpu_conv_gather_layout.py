"""-m gpu: the activation operand's LDS image of the two LDS-DMA conv kernels (conv3x3_dma_kernel: pair-interleaved patch
[2 planes][NP pixels][2 groups] x 16 B; conv1x1_dma_kernel: pixel-major [256 pixels][4 swizzled slots] x 16 B), through bbocr_op_conv2d (bf16 reader).

Per shape two checks that share one input:
  (i)  selector weights -- output channel o is 1.0 at ONE (tap, input channel), no bias: the output must equal the shifted input bit
       for bit (1.0 * x summed with zeros is exact in every format involved), so a wrong pixel, channel group or plane fails.  The
       selected (tap, 8-channel group) pairs cycle with o through ALL ntaps x Cin / 8 of them (a second launch where Cout is smaller).
  (ii) random weights against torch's fp64 convolution of the same bf16-rounded operands, tolerance of tests/test_gpu_ops.py.

Routing by launch_conv (bf16: first template argument 0), asserted per launch through the route the launch records (ROUTES below,
bbocr_op_conv2d_route):
  trunk_tile            3x3 64 -> 128, N 2, 19 x 37       conv3x3_dma_kernel<0, 2, 2, 8, 7, 3, 448>    4 x 64 tiles (6 x 66 patch: NPB = 7, 14 blocks per
                                                                                                plane), partial tiles on both axes, two chunks
  three_chunks_relu_in  3x3 96 -> 128, 16 x 16, relu_in   conv3x3_dma_kernel<0, 2, 2, 8, 6, 4, 384>    16 x 16 tile, in-place ReLU pass over the patch
  cout64_pool           3x3 64 -> 64, 33 x 18, pool 2x2   conv3x3_dma_kernel<0, 4, 1, 4, 6, 3, 384>    the tile rule picks 8 x 32 tiles here (10 x 34 patch
                                                                                                in 384 slots), not the 324-pixel patch: next row
  cout64_nps324_pool    3x3 64 -> 64, 32 x 32, pool 2x2   conv3x3_dma_kernel<0, 4, 1, 4, 6, 3, 324>    16 x 16 tiles, NPS = 324: 11 blocks per plane, the
                                                                                                odd waves fetch their last block twice
  dilated               3x3 d6 p6 32 -> 128, 13 x 20      conv3x3_dma_kernel<0, 2, 2, 8, 6, 4, 384>    36 phase images stacked, shared zero row
  ks2                   2x2 p0 64 -> 128, 4 x 70          conv3x3_dma_kernel<0, 2, 2, 8, 6, 4, 384, false, 4, 0, 2>
  1x1_4waves            160 -> 64, 558 pixels             conv1x1_dma_kernel<0, 4, 1, 4, 3, false>     four waves, five chunks, ragged last tile
  1x1_256couts          160 -> 256, 558 pixels            conv1x1_dma_kernel<0, 2, 2, 8, 3, false>     bbocr_op_conv2d plans 128-cout tiles (two); the
                                                                                                8-wave 256-cout tile is chosen only by the networks'
                                                                                                own plans (fc7, projections) and runs the same code
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = {
    # name: N, H, W, Cin, Cout, K, pad, dil, relu_in, pool_mode
    "trunk_tile": (2, 19, 37, 64, 128, 3, 1, 1, 0, 0),
    "three_chunks_relu_in": (1, 16, 16, 96, 128, 3, 1, 1, 1, 0),
    "cout64_pool": (1, 33, 18, 64, 64, 3, 1, 1, 0, 1),
    "cout64_nps324_pool": (1, 32, 32, 64, 64, 3, 1, 1, 0, 1),
    "dilated": (1, 13, 20, 32, 128, 3, 6, 6, 0, 0),
    "ks2": (1, 4, 70, 64, 128, 2, 0, 1, 0, 0),
    "1x1_4waves": (2, 9, 31, 160, 64, 1, 0, 1, 0, 0),
    "1x1_256couts": (2, 9, 31, 160, 256, 1, 0, 1, 0, 0),
}


# the docstring's routing table as bbocr_conv_route fields: what every launch of a case must record
ROUTES = {
    "trunk_tile": dict(id="DMA128_448", wm=2, wn=2, mf=8, npb=7, ring=3, nps=448, TH=4, TW=64, PH=6, PW=66, nchunks=2),
    "three_chunks_relu_in": dict(id="DMA128_384", wm=2, wn=2, mf=8, npb=6, ring=4, nps=384, TH=16, TW=16, nchunks=3),
    "cout64_pool": dict(id="DMA64_384", wm=4, wn=1, mf=4, npb=6, ring=3, nps=384, TH=8, TW=32, PH=10, PW=34),
    "cout64_nps324_pool": dict(id="DMA64_324", wm=4, wn=1, mf=4, npb=6, ring=3, nps=324, nf=4, TH=16, TW=16),
    "dilated": dict(id="DMA128_384", wm=2, wn=2, mf=8, npb=6, ring=4, nps=384, sub=6, stack=3),
    "ks2": dict(id="DMA2X2_128", wm=2, wn=2, mf=8, npb=6, ring=4, nps=384, fuse1=0, nf=4, epi=0, ks=2),
    "1x1_4waves": dict(id="DMA1X1_64", wm=4, wn=1, mf=4, ring=3, addup=0, nchunks=5, tiles_x=3),
    "1x1_256couts": dict(id="DMA1X1_128", wm=2, wn=2, mf=8, ring=3, addup=0, ntiles_n=2),
}


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _run(reader, xd, shape, w, b, relu_in, pool_mode):
    """One bbocr_op_conv2d launch; returns the (pooled, when pool_mode) NHWC bf16 output on the host as fp32."""
    N, H, W, Cin, Cout, K, pad, dil = shape
    OH, OW = H + 2 * pad - (K - 1) * dil, W + 2 * pad - (K - 1) * dil
    oh, ow = (OH // 2, OW // 2) if pool_mode else (OH, OW)
    out = torch.full((N, oh, ow, Cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    wn = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    bp = None
    if b is not None:
        bn = np.ascontiguousarray(b.numpy(), dtype=np.float32)
        bp = bn.ctypes.data_as(C.POINTER(C.c_float))
    rc = reader._lib.bbocr_op_conv2d(reader._h, C.c_void_p(xd.data_ptr()), N, H, W, Cin, wn.ctypes.data_as(C.POINTER(C.c_float)), bp, Cout, K, K,
                                     pad, dil, int(relu_in), 0, 0, None if pool_mode else C.c_void_p(out.data_ptr()), pool_mode, 0,
                                     C.c_void_p(out.data_ptr()) if pool_mode else None)
    reader._check(rc)
    return out.float().cpu()


def _assert_route(reader, name):
    from bb_ocr_amd import _lib

    r = _lib.bbocr_conv_route()
    reader._check(reader._lib.bbocr_op_conv2d_route(reader._h, C.byref(r)))
    got = r.as_dict()
    assert got["el"] == 0 and got["status"] == 0
    diff = {k: (v, got[k]) for k, v in ROUTES[name].items() if got[k] != v}
    assert not diff, f"{name}: the launch took another kernel than the table says (expected, recorded): {diff}"


@pytest.mark.parametrize("name", list(CASES))
def test_gather_layout(reader, name):
    N, H, W, Cin, Cout, K, pad, dil, relu_in, pool_mode = CASES[name]
    shape = (N, H, W, Cin, Cout, K, pad, dil)
    g = torch.Generator().manual_seed(11)
    x = _bf16(torch.randn(N, Cin, H, W, generator=g))
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    xin = F.relu(x) if relu_in else x
    ntaps, ngroups = K * K, Cin // 8

    # (i) selector weights: exact equality
    combos = ntaps * ngroups
    hit = set()
    for r in range((combos + Cout - 1) // Cout):
        w = torch.zeros(Cout, Cin, K, K)
        sel = []
        for o in range(Cout):
            combo = (o + r * Cout) % combos
            tap, grp = combo % ntaps, combo // ntaps
            cin = grp * 8 + (o * 3 + r) % 8
            w[o, cin, tap // K, tap % K] = 1.0
            sel.append((tap, cin))
            hit.add((tap, grp))
        xp = F.pad(xin, (pad, pad, pad, pad))
        OH, OW = H + 2 * pad - (K - 1) * dil, W + 2 * pad - (K - 1) * dil
        want = torch.stack([xp[:, cin, (tap // K) * dil:(tap // K) * dil + OH, (tap % K) * dil:(tap % K) * dil + OW] for tap, cin in sel], dim=-1)
        if pool_mode:
            want = F.max_pool2d(want.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        got = _run(reader, xd, shape, w, None, relu_in, pool_mode)
        _assert_route(reader, name)
        assert got.shape == want.shape
        bad = (got != want) & ~((got == 0) & (want == 0))         # -0.0 == 0.0; NaN (unwritten) != anything
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} selected values differ, first at {tuple(bad.nonzero()[0].tolist())}"
    assert len(hit) == combos            # every tap x every 8-channel group of every chunk

    # (ii) random weights against the fp64 convolution of the same rounded operands
    w = torch.randn(Cout, Cin, K, K, generator=g) / np.sqrt(Cin * K * K)
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(xin.double(), _bf16(w).double(), b.double(), padding=pad, dilation=dil)
    scale = ref.abs().max().item()
    if pool_mode:
        ref = F.max_pool2d(ref, 2)
    ref = ref.permute(0, 2, 3, 1).float()
    got = _run(reader, xd, shape, w, b, relu_in, pool_mode)
    _assert_route(reader, name)
    assert torch.isfinite(got).all()
    tol = 6e-3 * max(scale, 1.0)             # fp32 accumulate; bf16 output rounding 2^-8 relative (tests/test_gpu_ops.py)
    err = (got - ref).abs().max().item()
    print(f"{name}: conv err {err:.3e} (tol {tol:.3e}, scale {scale:.3f})")
    assert err <= tol, f"{name}: conv err {err} > {tol} (scale {scale})"
