"""GPU: every kernel route of the pre-processing chain at its edges, through bbocr_op_preprocess_stage alone (the rows of
tests/preproc_cases.py; tests/test_preproc_routes_cpu.py shows that they reach every member of the route enum).

Each row runs on uniform noise and on a designed plane, at chosen low pointer bits, between guard bytes, and must
* take the routes it names -- asked of the host route functions for these very pointers before the call,
* equal oracle/preprocess.py bit for bit,
* leave every byte outside the destination plane as it was, and
* give the same bytes again into a destination dirtied with another fill (nothing read from the destination, nothing left unwritten).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import preproc_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL, FILL2 = 0xEE, 0x11
BBOCR_ERR_ARG = -1


def run_guarded(reader, c, a, fill=FILL, expect_rc=0):
    """one bbocr_op_preprocess_stage call of row `c` on plane `a`: source at byte GUARD + so of its buffer, destination at GUARD + do of a
    buffer filled with `fill`, GUARD more bytes behind it.  Asserts the row's routes for these pointers, the status and the guards;
    -> the destination plane"""
    from bb_ocr_amd import _lib

    lib = reader._lib
    n_out = c.dh * c.dw
    host = np.zeros(GUARD + c.so + a.size + GUARD, dtype=np.uint8)
    host[GUARD + c.so:GUARD + c.so + a.size] = np.ascontiguousarray(a).reshape(-1)
    src = torch.from_numpy(host).cuda()
    dst = torch.from_numpy(np.full(GUARD + c.do + n_out + GUARD, fill, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()     # the uploads run on torch's stream, the library on its own non-blocking one
    sp, dp = src.data_ptr() + GUARD + c.so, dst.data_ptr() + GUARD + c.do
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0
    if expect_rc == 0:
        assert pc.routes_reported(lib, _lib.PP_ROUTE_IDS, c, src_bits=sp & 3, dst_bits=dp & 3) == c.routes, c
    rc = lib.bbocr_op_preprocess_stage(reader._h, c.stage, C.c_void_p(sp), c.H, c.W, C.c_void_p(dp), c.dh, c.dw, c.param)
    assert rc == expect_rc, (c, rc, lib.bbocr_last_error(reader._h))
    out = dst.cpu().numpy()
    lo, hi = GUARD + c.do, GUARD + c.do + n_out
    if expect_rc != 0:
        lo = hi                                                   # a refused call writes nothing at all
    outside = out != fill
    outside[lo:hi] = False
    touched = np.flatnonzero(outside)
    assert touched.size == 0, f"{c}: {touched.size} bytes outside the plane written, the first {int(touched[0]) - (GUARD + c.do)} bytes from its start"
    return out[GUARD + c.do:GUARD + c.do + n_out].reshape(c.dh, c.dw)


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_routes_bit_exact_between_guards(reader, group):
    for c in pc.GROUPS[group]:
        for name, a in pc.planes(c).items():
            want = pc.reference(c, a)
            got = run_guarded(reader, c, a)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{c} on {name}: {len(bad)} bytes differ from the oracle, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
            again = run_guarded(reader, c, a, fill=FILL2)
            assert np.array_equal(again, got), f"{c} on {name}: a second call into a dirtied destination differs"


@pytest.mark.parametrize("shape", pc.CLAHE_REFUSED, ids=[f"{h}x{w}" for h, w in pc.CLAHE_REFUSED])
def test_clahe_refuses_planes_below_the_tile_grid(reader, shape):
    H, W = shape
    c = pc.Case(4, H, W, H, W, 2.5, 0, 0, {})
    got = run_guarded(reader, c, pc.planes(c)["noise"], expect_rc=BBOCR_ERR_ARG)
    assert (got == FILL).all()
    assert b"smaller than the CLAHE tile grid" in reader._lib.bbocr_last_error(reader._h)
