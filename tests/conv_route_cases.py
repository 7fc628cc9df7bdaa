"""The case table of the conv route tests: one row per terminal of launch_conv's dispatch that bbocr_op_conv2d can reach, shared by
tests/test_conv_route_cpu.py (dry-run routes, invariants, references, planted defects) and tests/test_gpu_conv_routes.py (the launches).

A row = a name, the bbocr_op_conv2d arguments and the route the launch must take: the id (include/bbocr.h BBOCR_ROUTE_*) and the fields of
bbocr_conv_route that make the row what it is (template numbers, tile, patch slots, epilogue).  The authority for a route is the dry run of
the launch code (bbocr_host_conv_route); the expected values below were first derived by reading the dispatch and are compared with it for
both element types.  Sizes are ragged (partial tiles on both axes) unless the row's note says why not, and tiny.

STAGE_ONLY lists the route ids -- and the two epilogue switches -- that no bbocr_op_conv2d call can produce, with the test of
tests/test_gpu_stages.py that runs each; REFUSALS the argument sets the dispatch must decline.

Pure torch / numpy, no GPU."""
from __future__ import annotations

import ctypes as C
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import stage_ref as R

Case = namedtuple("Case", "name family N H W Cin Cout KH KW pad dil relu_in out_f32 pool_mode store_full route note exact")


def _c(name, family, N, H, W, Cin, Cout, KH, KW, pad, dil, route, note, relu_in=0, out_f32=0, pool_mode=0, store_full=0, exact=False):
    return Case(name, family, N, H, W, Cin, Cout, KH, KW, pad, dil, relu_in, out_f32, pool_mode, store_full, route, note, exact)


def _gen(bn, piter, **kw):
    return dict(id=f"GEN{bn}_P{piter}", wm=4 if bn == 64 else 2, wn=bn // 64, mf=4 if bn == 64 else 8, piter=piter, ring=2, **kw)


CASES = [
    # ------------------------------------------------------------------ conv_mfma_kernel, the register-staged generic kernel
    _c("g_1x1_pad1", "generic", 2, 9, 21, 96, 64, 1, 1, 1, 1, _gen(64, 4, TH=16, TW=16, NP=256, nchunks=3, ntaps=1),
       "ntaps < 3: one staging part, the next chunk loaded at the chunk's start and stored at its last tap; three chunks reuse both patch "
       "buffers; the zero border comes from padding alone"),
    _c("g_1x1_pool", "generic", 1, 10, 37, 64, 128, 1, 1, 0, 1, _gen(128, 4, TH=16, TW=16, NP=256, ntaps=1),
       "a pooled 1x1 does not take the DMA 1x1; odd width: floor pooling", pool_mode=1),
    _c("g_3x3_valid", "generic", 1, 19, 37, 64, 64, 3, 3, 0, 1, _gen(64, 8, NP=400, ntaps=9), "two staging parts over nine taps: S = 4"),
    _c("g_3x3_valid_pool21", "generic", 1, 18, 40, 64, 128, 3, 3, 0, 1, _gen(128, 8, TH=16, TW=16, NP=336, ntaps=9),
       "pooling epilogue (2,1) plus the full store", pool_mode=2, store_full=1),
    _c("g_1x3", "generic", 1, 17, 33, 64, 64, 1, 3, 1, 1, _gen(64, 8, PH=4, PW=66, NP=272, ntaps=3),
       "three taps, two parts: S = 1, every part loaded and stored within one tap; kx wraps where KH != KW"),
    _c("g_3x1", "generic", 1, 17, 33, 64, 64, 3, 1, 1, 1, _gen(64, 8, PH=6, PW=64, NP=384, ntaps=3), "as g_1x3 with ky"),
    _c("g_2x2_pad1", "generic", 1, 9, 40, 64, 128, 2, 2, 1, 1, _gen(128, 8, NP=304, ntaps=4), "four taps, two parts (S = 1); not the DMA 2x2, which needs pad 0"),
    _c("g_dil2_pad1", "generic", 1, 21, 27, 32, 128, 3, 3, 1, 2, _gen(128, 8, NP=432, sub=1, nchunks=1, ntaps=9), "tap offset (ky PW + kx) dil with pad != dil"),
    _c("g_dil4", "generic", 1, 26, 30, 96, 64, 3, 3, 1, 4, _gen(64, 16, NP=640, ntaps=9, nchunks=3), "PITER 16 with nine taps: four parts, S = 2"),
    _c("g_5x5_dil2", "generic", 1, 17, 35, 64, 128, 5, 5, 4, 2, _gen(128, 16, NP=864, ntaps=25), "PITER 16 with 25 taps: S = 6"),
    _c("g_patch_1024", "generic", 1, 20, 20, 64, 128, 3, 3, 1, 8, _gen(128, 16, TH=16, TW=16, PH=32, PW=32, NP=1024, lds_bytes=144 * 1024),
       "the largest accepted patch: 1024 slots, 144 KiB of LDS, only the 16 x 16 tile qualifies (one partial tile: the output is 6 x 6)"),
    _c("g_dil6_pool", "generic", 1, 16, 24, 64, 128, 3, 3, 6, 6, _gen(128, 16, sub=1, PH=28, PW=28, NP=784),
       "the sub-lattice route declines pooling: a dilated patch on the generic kernel", pool_mode=1),
    _c("g_f32_97", "generic", 1, 6, 40, 256, 97, 3, 3, 0, 1, _gen(128, 8, NP=400, nchunks=8),
       "112 of a 128-cout tile stored, run 1 partly present on the fp32 store path.  Operands are small dyadic numbers: every product and "
       "partial sum is exact in fp32, so the fp32 output must EQUAL the fp64 reference (the rule's rms term compares against the "
       "reference's own rounding noise, which for an fp32 output of random operands is below any fp32 accumulation)", out_f32=1, exact=True),
    _c("g_relu_in", "generic", 1, 19, 37, 64, 64, 3, 3, 0, 1, _gen(64, 8, NP=400), "ReLU on load as an integer max on the bits: -0 and negative inputs",
       relu_in=1),
    # ------------------------------------------------------------------ the LDS-DMA families
    _c("resw_pool64", "dma", 1, 18, 35, 32, 64, 3, 3, 1, 1, dict(id="RESW_POOL64", resw=1, nf=4, nps=324, persistent=2, TH=16, TW=16),
       "resident weights, 64 couts, pooled output only", pool_mode=1),
    _c("resw_1ch", "dma", 2, 27, 30, 32, 32, 3, 3, 1, 1, dict(id="RESW_1CH", resw=2, nf=2, nchunks=1, persistent=2), "resident weights, one chunk, double-buffered patch"),
    _c("resw_2ch", "dma", 1, 27, 30, 64, 16, 3, 3, 1, 1, dict(id="RESW_2CH", resw=3, nf=2, nchunks=2, persistent=2), "resident weights, two chunks"),
    _c("resw_persistent", "dma", 1, 368, 368, 32, 32, 3, 3, 1, 1, dict(id="RESW_1CH", resw=2, tiles_x=23, tiles_y=23),
       "529 tiles > 2 x 256 compute units: the persistent tile loop iterates (whole tiles: the point is the loop)"),
    _c("nf2", "dma", 1, 30, 30, 96, 32, 3, 3, 1, 1, dict(id="DMA64_324_NF2", nf=2, nps=324, ring=3, nchunks=3), "NF = 2 outside resw: three chunks"),
    _c("nps324_pool", "dma", 1, 32, 32, 64, 64, 3, 3, 1, 1, dict(id="DMA64_324", nf=4, nps=324, lean=3), "NPS 324 with four fragments; lean epilogue 3", pool_mode=1),
    _c("c64_nps384_pool", "dma", 1, 33, 18, 64, 64, 3, 3, 1, 1, dict(id="DMA64_384", nps=384, npb=6, TH=8, TW=32, lean=0), "64 couts at NPS 384", pool_mode=1),
    _c("npb7_64", "dma", 1, 19, 37, 64, 64, 3, 3, 1, 1, dict(id="DMA64_448", npb=7, nps=448, TH=4, TW=64, lean=1), "NPB 7 at 64 couts; lean epilogue 1"),
    _c("npb7_128", "dma", 2, 19, 37, 64, 128, 3, 3, 1, 1, dict(id="DMA128_448", npb=7, ring=3, lean=1), "NPB 7 at 128 couts"),
    _c("ring4_128", "dma", 1, 21, 27, 96, 128, 3, 3, 1, 1, dict(id="DMA128_384", npb=6, ring=4, lean=1, nchunks=3), "ring 4 at 128 couts; lean 1", relu_in=1),
    _c("lean3_128", "dma", 1, 30, 30, 64, 128, 3, 3, 1, 1, dict(id="DMA128_384", TH=16, TW=16, lean=3), "lean epilogue 3 (pooled only)", pool_mode=1),
    _c("lean0_pool_full", "dma", 1, 30, 30, 64, 128, 3, 3, 1, 1, dict(id="DMA128_384", TH=16, TW=16, lean=0), "pool + full store: the shared epilogue",
       pool_mode=1, store_full=1),
    _c("sub_128", "dma", 1, 13, 20, 32, 128, 3, 3, 6, 6, dict(id="DMA128_384", sub=6, stack=3), "sub-lattice route, 36 phase images stacked"),
    _c("sub_64", "dma", 2, 13, 21, 64, 64, 3, 3, 2, 2, dict(id="DMA64_324", sub=2, stack=7, lean=0), "sub-lattice route at 64 couts"),
    _c("k2_64", "dma", 1, 4, 70, 64, 64, 2, 2, 0, 1, dict(id="DMA2X2_64", ks=2, ring=3, nps=384), "2x2 route, 4 x 64 tiles (height 3 of 4, width 69 of 128)"),
    _c("k2_128", "dma", 2, 4, 70, 64, 128, 2, 2, 0, 1, dict(id="DMA2X2_128", ks=2, ring=4), "2x2 route at 128 couts"),
    _c("p1_64", "dma", 2, 9, 31, 160, 64, 1, 1, 0, 1, dict(id="DMA1X1_64", ring=3, nchunks=5, tiles_x=3), "DMA 1x1, four waves, ragged last tile of the flat pixel axis"),
    _c("p1_128", "dma", 2, 9, 31, 160, 256, 1, 1, 0, 1, dict(id="DMA1X1_128", ntiles_n=2), "DMA 1x1 at 128 couts per tile, two cout tiles"),
]
BY_NAME = {c.name: c for c in CASES}
GENERIC = [c.name for c in CASES if c.family == "generic"]
DMA = [c.name for c in CASES if c.family == "dma"]

# route ids bbocr_op_conv2d cannot produce -> the tests/test_gpu_stages.py test that runs the launch
STAGE_ONLY = {
    "DMA64_FUSE1": "test_c11_conv1_2_pool",        # conv1_2 with the conv1_1 producer fused in
    "DMA64_POSTW": "test_up3b_post_w",             # the 1x1 behind upconv3's 3x3
    "DMA1X1_ADDUP": "test_addup",                  # the up-sampling epilogue of the U-net 1x1 layers
    "DMA1X1_256": "test_up1a_two_sources",         # the 8-wave 256-cout tile, chosen only by the networks' own plans
}
# epilogue switches of ConvArgs that select no kernel of their own (bbocr_conv_route::tail / ::split_off), likewise out of the entry point's reach
STAGE_ONLY_SWITCHES = {"tail": "test_cls_tail", "split_off": "test_exact_conv_rows"}

# (name, N, H, W, Cin, Cout, KH, KW, pad, dil, why)
REFUSALS = [
    ("r_1x2_pad0", 1, 9, 21, 64, 64, 1, 2, 0, 1, "two taps want ONE staging part (PITER 4: at most 256 patch slots); every tile's patch is larger"),
    ("r_dil9", 1, 30, 30, 64, 64, 3, 3, 1, 9, "the smallest patch, 34 x 34, has more than 1024 slots"),
    ("r_height0", 1, 2, 30, 64, 64, 3, 3, 0, 1, "output height 0"),
]


# ---------------------------------------------------------------------------------------------------- the dry run
def dry_route(lib, c, el):
    """-> (status of bbocr_host_conv_route, route as a dict); el 0 bf16 / 1 fp16"""
    from bb_ocr_amd import _lib

    r = _lib.bbocr_conv_route()
    rc = lib.bbocr_host_conv_route(el, c.N, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.pad, c.dil, c.relu_in, 0, c.out_f32, c.pool_mode, 0, c.store_full,
                                   C.byref(r))
    return rc, r.as_dict()


def route_mismatch(want, got):
    return {k: (v, got[k]) for k, v in want.items() if got[k] != v}


# ---------------------------------------------------------------------------------------------------- operands and references
def out_hw(c):
    return c.H + 2 * c.pad - (c.KH - 1) * c.dil, c.W + 2 * c.pad - (c.KW - 1) * c.dil


def inputs(c, el):
    """x [N, Cin, H, W], w [Cout, Cin, KH, KW] (both already rounded to `el`), b [Cout] fp32 -- float32 tensors, seeded by the row's name"""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    if c.exact:
        x = torch.randint(-16, 17, (c.N, c.Cin, c.H, c.W), generator=g).float() / 8
        w = torch.randint(-8, 9, (c.Cout, c.Cin, c.KH, c.KW), generator=g).float() / 16
        b = torch.randint(-32, 33, (c.Cout,), generator=g).float() / 16
        return x, w, b
    x = torch.randn(c.N, c.Cin, c.H, c.W, generator=g)
    if c.relu_in:
        x[:, :, ::3, 1::4] = -0.0                      # the integer max must turn the sign bit's pattern into +0 too
    w = torch.randn(c.Cout, c.Cin, c.KH, c.KW, generator=g) / float(np.sqrt(c.Cin * c.KH * c.KW))
    b = torch.randn(c.Cout, generator=g) * 0.1
    return R.rnd(x, el), R.rnd(w, el), b


def selector_weights(c, r):
    """Round r of the selector-weight pass (tests/test_gpu_conv_gather_layout.py): output channel o is 1.0 at ONE (tap, input channel); o
    cycles through every (tap, 8-channel group).  -> (w, [(tap, cin)] per output channel)"""
    ntaps, combos = c.KH * c.KW, c.KH * c.KW * (c.Cin // 8)
    w = torch.zeros(c.Cout, c.Cin, c.KH, c.KW)
    sel = []
    for o in range(c.Cout):
        combo = (o + r * c.Cout) % combos
        tap, grp = combo % ntaps, combo // ntaps
        cin = grp * 8 + (o * 3 + r) % 8
        w[o, cin, tap // c.KW, tap % c.KW] = 1.0
        sel.append((tap, cin))
    return w, sel


def selector_rounds(c):
    return (c.KH * c.KW * (c.Cin // 8) + c.Cout - 1) // c.Cout


def _pool(c, y, mut=None):
    """y [N, C, OH, OW] -> the pooled tensor of the row's pool_mode (floor sizes, as MaxPool2d)"""
    if mut == "pool_off":                                  # pairs (1,2), (3,4), ... instead of (0,1), (2,3), ...
        y = torch.cat([y[:, :, 1:], y[:, :, -1:]], dim=2)
    return F.max_pool2d(y, (2, 2) if c.pool_mode == 1 else (2, 1))


def conv_taps(c, x, w, b, dt, mut=None, geom=None):
    """The convolution written tap by tap, so that a named mistake can be planted (mut):
      dil1         tap offsets computed with dil = 1
      pad_off      the image sits one pixel off in its padding
      last_tap     the last tap is dropped
      chunk_reuse  the second 32-channel chunk is read from the first chunk's channels
      no_relu_in   ReLU on load left out
      stale_part   the patch slots 256.. of every chunk but the first still hold the previous chunk (one staging part not stored); needs
                   geom = the route's TH, TW, PH, PW
    -> [N, Cout, OH, OW] in dt"""
    OH, OW = out_hw(c)
    x = x.to(dt)
    if c.relu_in and mut != "no_relu_in":
        x = F.relu(x)
    if mut == "chunk_reuse":
        x = x.clone()
        x[:, 32:64] = x[:, 0:32]
    w = w.to(dt)
    ext = (c.KH - 1) * c.dil + OH + 64, (c.KW - 1) * c.dil + OW + 64            # room for whole tiles beyond the image
    xp = torch.zeros(c.N, c.Cin, ext[0] + 1, ext[1] + 1, dtype=dt)
    o0 = c.pad + (1 if mut == "pad_off" else 0)
    xp[:, :, o0:o0 + c.H, o0:o0 + c.W] = x
    d = 1 if mut == "dil1" else c.dil
    taps = [(ky, kx) for ky in range(c.KH) for kx in range(c.KW)]
    if mut == "last_tap":
        taps = taps[:-1]

    def run(src, oh, ow, y0=0, x0=0):
        acc = torch.zeros(c.N, c.Cout, oh, ow, dtype=dt)
        for ky, kx in taps:
            acc += torch.einsum("nchw,oc->nohw", src[:, :, y0 + ky * d:y0 + ky * d + oh, x0 + kx * d:x0 + kx * d + ow], w[:, :, ky, kx])
        return acc

    if mut == "stale_part":
        TH, TW, PH, PW = geom
        y = torch.zeros(c.N, c.Cout, OH + TH, OW + TW, dtype=dt)
        slot = (torch.arange(PH)[:, None] * PW + torch.arange(PW)[None, :]) >= 256
        for ty in range(0, OH, TH):
            for tx in range(0, OW, TW):
                patch = xp[:, :, ty:ty + PH, tx:tx + PW].clone()
                for ch in range(1, c.Cin // 32):
                    patch[:, 32 * ch:32 * ch + 32] = torch.where(slot, xp[:, 32 * (ch - 1):32 * ch, ty:ty + PH, tx:tx + PW], patch[:, 32 * ch:32 * ch + 32])
                y[:, :, ty:ty + TH, tx:tx + TW] = run(patch, TH, TW)
        y = y[:, :, :OH, :OW]
    else:
        y = run(xp, OH, OW)
    return y + b.to(dt)[None, :, None, None]


def reference(c, x, w, b, dt=torch.float64, mut=None, geom=None):
    """-> (full [N, OH, OW, Cout], pooled [N, OH/2, OW or OW/2, Cout] or None) in dt; mut None: torch's own convolution"""
    if mut in (None, "pool_off"):
        xin = F.relu(x.to(dt)) if c.relu_in else x.to(dt)
        y = F.conv2d(xin, w.to(dt), b.to(dt), padding=c.pad, dilation=c.dil)
    else:
        y = conv_taps(c, x, w, b, dt, mut, geom)
    return R.nhwc(y), (R.nhwc(_pool(c, y, mut)) if c.pool_mode else None)


def el_out(c, el):
    return None if c.out_f32 else el


def outputs_checked(c):
    """which of (full, pooled) the row's launch writes"""
    return (not c.pool_mode or bool(c.store_full)), bool(c.pool_mode)
