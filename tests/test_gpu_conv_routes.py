"""-m gpu: every terminal of launch_conv's dispatch that bbocr_op_conv2d can reach, launched once per element type (`reader`: bf16,
`reader_fp16`), on the rows of tests/conv_route_cases.py -- the register-staged generic kernel (conv_mfma_kernel, all 12 instantiations)
among them.  The LDS-DMA rows come first, the generic rows behind them with the smallest patch first.

Per row and element type:
  route          the route the launch itself recorded (bbocr_op_conv2d_route) is the row's, and the dry run's;
  sentinel       the outputs are views inside larger buffers of 0xA5 bytes and are NaN-filled before the launch: the guard bytes stay
                 untouched, no NaN is left, and the stored channels Cout .. roundup16(Cout) - 1 (zero weights, zero bias) are exactly 0;
  per element    against the fp64 convolution of the same rounded operands under tests/stage_ref.py::check with ref_q = ref_nq, E = 0 and
                 the 1e-3 cap (a single rounding: DESIGN section 5) -- a failure names page border, tile seam or interior;
  repeatable     a second launch repeats the first bit for bit;
  selector       (generic rows) one 1.0 per output channel, cycling through every (tap, 8-channel group): the output equals the shifted
                 input bit for bit.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_route_cases as cc  # noqa: E402
import stage_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096                                                    # bytes before and behind every output
ORDER = cc.DMA + sorted(cc.GENERIC, key=lambda n: cc.BY_NAME[n].route["NP"])       # generic rows: smallest patch first
ELS = {"bf16": 0, "fp16": 1}


def _reader(request, el):
    return request.getfixturevalue("reader" if el == "bf16" else "reader_fp16")


@functools.lru_cache(maxsize=None)
def _case_data(name, el):
    """operands and fp64 references of a row, computed once and left unchanged"""
    c = cc.BY_NAME[name]
    x, w, b = cc.inputs(c, el)
    return x, w, b, cc.reference(c, x, w, b)


class _Sentinel:
    """a tensor of `shape` inside a larger 0xA5-filled allocation, NaN-filled"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        self.t.fill_(float("nan"))
        self.n = n

    def guards_untouched(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.n:] == 0xA5).all())


def _launch(reader, c, el, xd, w, b):
    """one bbocr_op_conv2d call of the row -> (full sentinel or None, pooled sentinel or None, recorded route)"""
    from bb_ocr_amd import _lib

    dt = R.DTYPES[el]
    OH, OW = cc.out_hw(c)
    store = (c.Cout + 15) // 16 * 16
    want_full, want_pool = cc.outputs_checked(c)
    full = _Sentinel((c.N, OH, OW, store), torch.float32 if c.out_f32 else dt) if want_full else None
    pooled = _Sentinel((c.N, OH // 2, OW // 2 if c.pool_mode == 1 else OW, store), dt) if want_pool else None
    wn = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    bp = None
    if b is not None:
        bn = np.ascontiguousarray(b.numpy(), dtype=np.float32)
        bp = bn.ctypes.data_as(C.POINTER(C.c_float))
    torch.cuda.synchronize()
    rc = reader._lib.bbocr_op_conv2d(reader._h, C.c_void_p(xd.data_ptr()), c.N, c.H, c.W, c.Cin, wn.ctypes.data_as(C.POINTER(C.c_float)), bp, c.Cout,
                                     c.KH, c.KW, c.pad, c.dil, c.relu_in, 0, c.out_f32, C.c_void_p(full.t.data_ptr()) if full else None, c.pool_mode, 0,
                                     C.c_void_p(pooled.t.data_ptr()) if pooled else None)
    reader._check(rc)
    r = _lib.bbocr_conv_route()
    reader._check(reader._lib.bbocr_op_conv2d_route(reader._h, C.byref(r)))
    return full, pooled, r.as_dict()


def _upload(x, el):
    return R.nhwc(x).to(R.DTYPES[el]).cuda()


@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("name", ORDER)
def test_route_row(request, name, el):
    reader = _reader(request, el)
    c = cc.BY_NAME[name]
    x, w, b, (ref_full, ref_pool) = _case_data(name, el)
    xd = _upload(x, el)
    full, pooled, route = _launch(reader, c, el, xd, w, b)

    # the route the launch recorded
    assert route["status"] == 0 and route["el"] == ELS[el]
    assert not cc.route_mismatch(c.route, route), f"{name}: launched {route}, expected {c.route}"
    rc, dry = cc.dry_route(reader._lib, c, ELS[el])
    assert rc == 0
    if route["persistent"]:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert route["grid"] == min(dry["grid"], route["persistent"] * cus)
        if name == "resw_persistent":
            assert dry["grid"] > route["grid"], "the persistent tile loop must iterate in this row"
        dry["grid"] = route["grid"]
    assert route == dry, {k: (route[k], dry[k]) for k in route if route[k] != dry[k]}

    first = []
    for which, s, ref, eo in (("full", full, ref_full, cc.el_out(c, el)), ("pooled", pooled, ref_pool, el)):
        if s is None:
            continue
        assert s.guards_untouched(), f"{name} {which}: bytes outside the output were written"
        got = s.t.double().cpu()
        assert not torch.isnan(got).any(), f"{name} {which}: {int(torch.isnan(got).sum())} elements were never written"
        assert bool((got[..., c.Cout:] == 0).all()), f"{name} {which}: stored channels beyond Cout are not zero"
        got = got[..., :c.Cout]
        if c.exact:
            assert torch.equal(got, ref), f"{name} {which}: exact operands, {int((got != ref).sum())} elements differ"
        R.check(got, ref, ref, 0.0, eo, f"conv route {name} {el} {which} [{route['id']}]", cap=1e-3)
        first.append(s.t.clone())

    # a second launch repeats the first bit for bit
    full2, pooled2, route2 = _launch(reader, c, el, xd, w, b)
    assert route2 == route
    again = [s.t for s in (full2, pooled2) if s is not None]
    for a, bb in zip(first, again):
        assert torch.equal(a.view(torch.uint8), bb.view(torch.uint8)), f"{name}: the second launch differs from the first"


@pytest.mark.parametrize("el", list(ELS))
@pytest.mark.parametrize("name", [n for n in ORDER if n in cc.GENERIC])
def test_generic_selector_weights(request, name, el):
    """output channel o is 1.0 at ONE (tap, input channel), no bias: 1.0 * x summed with zeros is exact in every format involved, so the output
    must equal the shifted input bit for bit -- a wrong patch slot, channel group, tap offset or staging part fails"""
    reader = _reader(request, el)
    c = cc.BY_NAME[name]
    x = _case_data(name, el)[0]
    xd = _upload(x, el)
    xin = F.relu(x) if c.relu_in else x
    OH, OW = cc.out_hw(c)
    xp = F.pad(xin, (c.pad, c.pad, c.pad, c.pad))
    hit = set()
    for r in range(cc.selector_rounds(c)):
        w, sel = cc.selector_weights(c, r)
        hit |= {(tap, cin // 8) for tap, cin in sel}
        want = torch.stack([xp[:, cin, (tap // c.KW) * c.dil:(tap // c.KW) * c.dil + OH, (tap % c.KW) * c.dil:(tap % c.KW) * c.dil + OW]
                            for tap, cin in sel], dim=-1)
        full, pooled, route = _launch(reader, c, el, xd, w, None)
        assert route["id"] == c.route["id"]
        for s, wt in ((full, want), (pooled, R.nhwc(cc._pool(c, R.nchw(want))) if c.pool_mode else None)):
            if s is None:
                continue
            got = s.t.float().cpu()[..., :c.Cout]
            assert got.shape == wt.shape
            bad = (got != wt) & ~((got == 0) & (wt == 0))         # -0.0 == 0.0; NaN (unwritten) != anything
            assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} selected values differ, first at {tuple(bad.nonzero()[0].tolist())}"
    assert len(hit) == c.KH * c.KW * (c.Cin // 8)                 # every tap x every 8-channel group of every chunk
