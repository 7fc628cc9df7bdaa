"""-m gpu: the BiLSTM input projection's own kernel (bb-ocr_amd/csrc/seq_proj.hip: weights resident in registers, rows streamed through a
LDS ring, stores never waited for) against the 1x1-conv path it replaces and against fp64, through tools/micro/seq_proj_shim.hip on a
live context, for both layers and both 16-bit element types.

Row counts: 256 (fewer slots than row chunks: most workgroups get an empty chunk and must do nothing), 2304 = 9 x 256, a count whose last
chunk is shorter than the others, and the smallest count at which every chunk wraps the ring three times -- the last two computed from the
launcher's chunk rule (seq_proj_shim_plan), not from constants.  Inputs are seeded normal values rounded to the element type; a few rows are
all zero and a few are scaled until their largest output sits near the top of the element type's range (fp16: 0.75 x 65504; bf16 shares
fp32's exponent range, so the fp32 accumulators' partial sums get 8 binades of headroom: 2^-8 x max), the inputs themselves staying below half
the type's maximum.

Checks per case: (1) bit-equal to the conv path on the same input; (2) the fast-mode single-GEMM rule of tests/stage_ref.py (check, one
rounding: ref_q = ref_nq = the fp64 product of the rounded operands, E = 0) -- applied to the ordinary rows and to the scaled rows
separately, because the rule's absolute term follows the largest reference value of what it is given; (3) 256 sentinel rows before and after
the output are untouched; (4) two runs are bit-equal.  The fp64 product is taken on the device (torch), once per case."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

import stage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3
GUARD = 256                     # sentinel rows on either side of the output


@pytest.fixture(scope="module")
def shim_path(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    lib = os.path.join(ROOT, "bb-ocr_amd")
    so = str(tmp_path_factory.mktemp("seq_proj_shim") / "seq_proj_shim.so")
    cc = subprocess.run([hipcc, "-O2", "-std=c++20", "-shared", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(lib, "csrc"), "-I" + os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tools", "micro", "seq_proj_shim.hip"), "-L" + lib, "-lbbocr", "-Wl,-rpath," + lib, "-o", so],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert cc.returncode == 0, cc.stdout.decode()[-2000:]
    return so


@pytest.fixture(scope="module")
def states():
    from bb_ocr_amd import weights

    return R.craft_state(SEED), weights.synthetic_crnn_state(SEED)


class Proj:
    """a Reader of one 16-bit precision + the shim bound to its context"""

    def __init__(self, so, states, el):
        import bb_ocr_amd

        self.el, self.dtype = el, R.DTYPES[el]
        self.reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=states, precision=el)      # loads libbbocr.so (after torch's HIP runtime)
        self.lib = C.CDLL(so)
        self.lib.seq_proj_shim_error.restype = C.c_char_p
        self.h = self.reader._h
        self.crnn = states[1]
        assert self.lib.seq_proj_shim_rec_el(self.h) == (0 if el == "bf16" else 1)
        perm = torch.tensor([self.lib.seq_proj_shim_xproj_channel(d, g, u) for d in range(2) for g in range(4) for u in range(256)], dtype=torch.long)
        assert sorted(perm.tolist()) == list(range(2048))
        self.wb = []
        for layer in range(2):
            w, b, _ = R.seq_gemm_weights(self.crnn, 0, layer, perm)
            self.wb.append((R.rnd(w[:, :, 0, 0], el).cuda(), b.cuda()))              # the packed image holds the weights rounded to the element type

    def plan(self, rows_pad):
        p = (C.c_longlong * 5)()
        rc = self.lib.seq_proj_shim_plan(self.h, C.c_size_t(rows_pad), p)
        assert rc == 0, f"seq_proj_shim_plan: status {rc} {self.lib.seq_proj_shim_error().decode()}"
        return {"grid": p[0], "chunks": p[1], "nslots": p[2], "chunk_slots": p[3], "ring": p[4]}

    def run(self, path, layer, x, rows_pad):
        """-> the guarded buffer [GUARD + rows_pad + GUARD, 2048], NaN-filled before the launch"""
        buf = torch.full((rows_pad + 2 * GUARD, 2048), float("nan"), dtype=self.dtype, device="cuda")
        torch.cuda.synchronize()
        rc = self.lib.seq_proj_shim_run(self.h, path, layer, C.c_void_p(x.data_ptr()), C.c_size_t(x.numel()), C.c_size_t(rows_pad),
                                        C.c_void_p(buf.data_ptr() + GUARD * 2048 * 2), C.c_size_t(rows_pad * 2048))
        assert rc == 0, f"seq_proj_shim_run(path {path}): status {rc}" + \
            (" (hipErrorNotSupported: production would take the conv path)" if rc == 801 else "") + f" {self.lib.seq_proj_shim_error().decode()}"
        return buf


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def pj(request, shim_path, states):
    p = Proj(shim_path, states, request.param)
    yield p
    p.reader.close()


def _rows(pj, case):
    """the case's row count from the launcher's chunk rule on this device"""
    if case == "one_tile":
        return 256
    if case == "nine_tiles":
        return 2304
    first = pj.plan(256)
    chunks, ring = first["chunks"], first["ring"]
    if case == "ragged":                                       # the smallest count whose last non-empty chunk is shorter than the others
        rows = 256
        while True:
            p = pj.plan(rows)
            if p["chunk_slots"] >= 2 and p["nslots"] % p["chunk_slots"]:
                return rows
            rows += 256
    assert case == "ring_wraps"                                # every chunk holds more than 3 x ring slots: each ring slot is refilled three times
    rows = (chunks * ring * 3 * 64 + 256) // 256 * 256
    while pj.plan(rows)["chunk_slots"] <= ring * 3:
        rows += 256
    return rows


ZERO_ROWS = (0, 17, 63, 64, -1)
BIG_ROWS = (5, 100, 255, -2)


def _inputs(pj, layer, rows_pad):
    """x [rows_pad, 256] of the element type (device) and the indices of its scaled rows"""
    el_max = float(torch.finfo(pj.dtype).max)
    target = 0.75 * el_max if pj.el == "fp16" else el_max * 2.0 ** -8
    g = torch.Generator().manual_seed(900 + layer)
    x = torch.randn((rows_pad, 256), generator=g).double()
    w, _ = pj.wb[layer]
    big = torch.tensor([r % rows_pad for r in BIG_ROWS])
    unit = R.rnd(x[big], pj.el)
    out_unit = (unit.cuda() @ w.T).abs().amax(dim=1).cpu()
    scale = torch.minimum(target / out_unit, 0.5 * el_max / unit.abs().amax(dim=1))
    x[big] = unit * scale[:, None]
    x[torch.tensor([r % rows_pad for r in ZERO_ROWS])] = 0
    return x.to(pj.dtype).cuda(), big


@pytest.mark.parametrize("case", ["one_tile", "nine_tiles", "ragged", "ring_wraps"])
@pytest.mark.parametrize("layer", [0, 1])
def test_seq_proj(pj, layer, case):
    rows_pad = _rows(pj, case)
    plan = pj.plan(rows_pad)
    print(f"[seq_proj] {pj.el} layer {layer} {case}: {rows_pad} rows, plan {plan}")
    if case == "one_tile":
        assert plan["nslots"] < plan["chunks"]                 # empty chunks exist
    if case == "ragged":
        assert plan["nslots"] % plan["chunk_slots"] and plan["chunk_slots"] >= 2
    if case == "ring_wraps":
        assert plan["chunk_slots"] > plan["ring"] * 3
    x, big = _inputs(pj, layer, rows_pad)
    bits = lambda t: t.view(torch.int16)
    new = pj.run(0, layer, x, rows_pad)
    again = pj.run(0, layer, x, rows_pad)
    alone = pj.run(2, layer, x, rows_pad)                      # the launcher must not decline these shapes
    kept = pj.run(1, layer, x, rows_pad)
    body = slice(GUARD, GUARD + rows_pad)
    # (3) sentinels: the NaN fill on either side is still the fill, in every buffer
    fill = bits(torch.full((1,), float("nan"), dtype=pj.dtype, device="cuda"))[0]
    for name, buf in (("new", new), ("conv path", kept)):
        for side, part in (("before", buf[:GUARD]), ("after", buf[GUARD + rows_pad:])):
            touched = int((bits(part) != fill).sum())
            assert touched == 0, f"{name}: {touched} values of the {GUARD} sentinel rows {side} the output were written"
    # (4) and (1)
    assert torch.equal(bits(new), bits(again)), f"two runs differ in {int((bits(new) != bits(again)).sum())} values"
    assert torch.equal(bits(new), bits(alone)), "crnn_seq_xproj and launch_seq_proj alone differ"
    diff = bits(new[body]) != bits(kept[body])
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} values differ from the conv path, first at row {int(torch.nonzero(diff)[0][0])}, " \
        f"channel {int(torch.nonzero(diff)[0][1])}"
    # (2) fp64 product of the same rounded operands
    w, b = pj.wb[layer]
    ref = x.double() @ w.T + b
    assert float(ref.abs().max()) < float(torch.finfo(pj.dtype).max)
    got = new[body].double()
    ordinary = torch.ones(rows_pad, dtype=torch.bool, device="cuda")
    ordinary[big.cuda()] = False
    for name, sel in (("ordinary rows", ordinary), ("scaled rows", ~ordinary)):
        r = ref[sel]
        R.check(got[sel], r, r, 0.0, pj.el, f"seq_proj {pj.el} layer {layer} {case} {name}", index_names=("row", "c"))
    zero = torch.tensor([r % rows_pad for r in ZERO_ROWS], device="cuda")
    assert torch.equal(bits(new[body][zero]), bits(b.to(pj.dtype)[None].expand(len(ZERO_ROWS), -1).contiguous())), "an all-zero row must give the rounded bias"
