"""-m gpu: the folded fc6 -> fc7 -> upconv1.conv.0 stage of the fast-mode detector (detector.cpp::craft_fc_stage, weights from
bb-ocr_amd/csrc/fc_fold.h), through tools/micro/stage_shim.hip on a live context, fp16 and bf16.

References are built from tests/stage_ref.py's layers in fp64 and held to that file's rule (R.check).  The quantised model of the stage:

  Wc   = the product Wy W7 W6 of the fp32-folded layers, formed in fp64, rounded ONCE to fp32 and then to the element type (what
         load_fc_fold packs); Ws = upconv1.conv.0's skip columns, rounded; b' = Wy (W7 b6 + b7) + b, fp32
  z    = Wc (*)dil6 p5, rounded once to the element type (launch 1 stores it)
  out  = ReLU(z + Ws s4 + b'), rounded once (launch 2)

ref_q rounds z, ref_nq does not, and the allowance E is one element-type ulp of z: z reaches the output through the identity, and ReLU is
1-Lipschitz.  stage_addsame (launch 2 alone, z given) is a single-rounding stage: E = 0.  stage_addsame_route is launch 2's dry run: the
route it reports, and the launcher's refusal of a z that is not N * H * W x cout.

Last, one 64 x 96 designed-weight page through heatmap_device: within HEAT_TOL_FP16 / HEAT_TOL of the oracle's fp32 maps, boxes the oracle's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_ref as R
from test_gpu_pipeline import HEAT_TOL
from test_gpu_precision import HEAT_TOL_FP16
from test_gpu_stages import Stage, _act, _check, shim_path, st, stage_states  # noqa: F401  (fixtures: the shim and a Reader per element type)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def product(stage_states):
    """(Wc, Ws, b') of the fp32-folded layers in fp64, each rounded once to fp32 -- computed once, rounded to the element type per test"""
    W = R.Weights(stage_states[0], "f32")
    (w6, b6), (w7, b7), (wu, bu) = W.layer("basenet.slice5.1"), W.layer("basenet.slice5.2"), W.up1a()
    wy, ws, w7 = wu[:, :1024, 0, 0], wu[:, 1024:], w7[:, :, 0, 0]
    wc = torch.einsum("ok,kiyx->oiyx", wy @ w7, w6)
    bp = wy @ (w7 @ b6 + b7) + bu
    f32 = lambda t: t.float().double()
    return f32(wc), f32(ws), f32(bp)


def _weights(product, el):
    wc, ws, bp = product
    return R.rnd(wc, el), R.rnd(ws, el), bp


def _fc_stage(Wf, p5, s4, el, q):
    wc, ws, bp = Wf
    z = R.conv(R.nchw(p5.double()), wc, pad=6, dil=6)
    if q:
        z = R.rnd(z, el)
    return R.nhwc(F.relu(z + R.conv(R.nchw(s4.double()), ws, bp))), R.nhwc(z)


# fc6's sub-lattice cases (stage_ref.EXACT_CONV_CASES) and one shape that is a multiple of no tile
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 15, 20), (1, 13, 6), (3, 7, 5)])
def test_fc_fold_stage(st, product, shape):
    N, H, W = shape
    p5, s4 = _act((N, H, W, 512), st.el, 500), _act((N, H, W, 512), st.el, 501)
    dp, ds = p5.cuda(), s4.cuda()

    def run():
        o = st.out((N, H, W, 512))
        st.call("stage_fc_fold", dp, ds, N, H, W, o)
        return o

    Wf = _weights(product, st.el)
    rq, _ = _fc_stage(Wf, p5, s4, st.el, True)
    rn, z = _fc_stage(Wf, p5, s4, st.el, False)
    _check(st, "fc_fold", f"{N}x{H}x{W}", st.twice(run), (rq, rn, R.ulp_el(z, st.el)), st.el)


# (2, 16, 24): three 256-pixel tiles exactly
@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 7, 5), (2, 16, 24)])
def test_addsame(st, product, shape):
    N, H, W = shape
    s4, z = _act((N, H, W, 512), st.el, 510), _act((N, H, W, 512), st.el, 511)
    z[..., 64:72] *= 64                         # one lane's run of 8 channels, 64 x the rest (exact): a wrong channel offset moves it
    ds, dz = s4.cuda(), z.cuda()

    def run(fill):
        o = torch.full((N, H, W, 512), fill, dtype=st.dtype, device="cuda")
        st.call("stage_addsame", ds, dz, N, H, W, o)
        return o

    a, b = run(float("nan")), run(-7.0)         # two runs from differently dirtied outputs: bit-equal
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"two runs differ in {int((a.view(torch.int16) != b.view(torch.int16)).sum())} values"
    _, ws, bp = _weights(product, st.el)
    rq = R.nhwc(F.relu(R.nchw(z.double()) + R.conv(R.nchw(s4.double()), ws, bp)))
    _check(st, "addsame", f"{N}x{H}x{W}", a.cpu(), (rq, rq, 0.0), st.el)


def test_addsame_route_and_refusals(st):
    """dry runs of launch 2 (launch_conv's own dispatch, nothing launched): a z of N * H * W x 512 takes conv1x1_dma_kernel's same-resolution
    epilogue and the route report says so; any other z is refused with hipErrorInvalidValue before a kernel could read past it"""
    import ctypes as C

    from bb_ocr_amd import _lib

    def dry(zH, zW, zC):
        rid, add = C.c_int(-1), C.c_int(-1)
        rc = st.lib.stage_addsame_route(st.h, 2, 7, 5, zH, zW, zC, C.byref(rid), C.byref(add))
        return rc, _lib.CONV_ROUTE_IDS[rid.value], add.value

    assert dry(7, 5, 512) == (0, "DMA1X1_ADDUP", 2)
    for z in [(8, 5, 512), (7, 6, 512), (6, 5, 512), (7, 5, 256), (7, 5, 1024), (5, 7, 512)]:
        assert dry(*z) == (1, "NONE", 0), z                   # 1 = hipErrorInvalidValue


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_designed_page_heatmap_and_boxes(precision, reader, reader_fp16, oracle_reader):
    from bb_ocr_amd import synth

    r, tol = (reader_fp16, HEAT_TOL_FP16) if precision == "fp16" else (reader, HEAT_TOL)
    img = synth.page(8, width=96, height=64, lines=1, margin=8)[0]
    st_, sl, r2 = oracle_reader.heatmap(img)
    heat, ratio = r.heatmap_device(torch.from_numpy(img[None]).cuda())
    got = heat[0].cpu().numpy()
    e_text, e_link = float(np.abs(got[..., 0] - st_).max()), float(np.abs(got[..., 1] - sl).max())
    print(f"{precision}: 64 x 96 page, max |heat - oracle| text {e_text:.5f} link {e_link:.5f} (bound {tol})")
    assert ratio == r2 and got.shape[:2] == st_.shape and st_.max() > 0.7
    assert e_text <= tol and e_link <= tol
    oh, of = oracle_reader.detect(img)
    hl, fl = r.detect(img)
    assert len(oh) >= 1
    assert [list(map(int, b)) for b in oh] == hl[0]
    assert len(of) == len(fl[0]) and all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)) for a, b in zip(fl[0], of))
