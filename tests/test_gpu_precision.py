"""-m gpu: the fp16 MFMA path (bbocr_config::precision FP16, BASELINE.json configs[4]) and the exact recogniser mode (EXACT: split
fp16, decoded text identical to the fp32 CPU path) against the oracle / torch fp64, through the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HEAT_TOL_FP16 = 0.008      # max |heat - oracle fp32| on designed-weight pages, fp16 storage (bf16: 0.03); values span 0..6


def _conv(reader, dtype, N, H, W, Cin, Cout, K, pad, dil, relu_in, relu_out, out_f32, pool_mode=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = lambda t: t.to(dtype).to(torch.float32)
    x = q(torch.randn(N, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, K, K, generator=g) / np.sqrt(Cin * K * K)
    b = torch.randn(Cout, generator=g) * 0.1
    xin = F.relu(x) if relu_in else x
    ref = F.conv2d(xin.double(), q(w).double(), b.double(), padding=pad, dilation=dil)
    if relu_out:
        ref = F.relu(ref)
    if pool_mode:
        ref = F.max_pool2d(ref, (2, 2) if pool_mode == 1 else (2, 1))
    ref = ref.permute(0, 2, 3, 1).float()
    store = (Cout + 15) // 16 * 16
    xd = x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()
    out = torch.full((N, ref.shape[1], ref.shape[2], store), float("nan"), dtype=torch.float32 if out_f32 else dtype, device="cuda")
    wn = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    bn = np.ascontiguousarray(b.numpy(), dtype=np.float32)
    rc = reader._lib.bbocr_op_conv2d(reader._h, C.c_void_p(xd.data_ptr()), N, H, W, Cin, wn.ctypes.data_as(C.POINTER(C.c_float)),
                                     bn.ctypes.data_as(C.POINTER(C.c_float)), Cout, K, K, pad, dil, int(relu_in), int(relu_out), int(out_f32),
                                     None if pool_mode else C.c_void_p(out.data_ptr()), pool_mode, 0, C.c_void_p(out.data_ptr()) if pool_mode else None)
    reader._check(rc)
    got = out.float().cpu()[..., :Cout]
    assert torch.isfinite(got).all()
    return (got - ref).abs().max().item(), max(ref.abs().max().item(), 1.0)


@pytest.mark.parametrize("cfg", [
    # N, H, W, Cin, Cout, K, pad, dil, relu_in, relu_out, out_f32, pool_mode
    (2, 19, 37, 64, 64, 3, 1, 1, 0, 1, 0, 0),      # BN=64 DMA kernel, ragged edges
    (1, 24, 40, 64, 128, 3, 1, 1, 1, 0, 0, 0),     # BN=128, ReLU on load (integer max on fp16 bits)
    (1, 15, 20, 64, 256, 3, 6, 6, 0, 0, 0, 0),     # dilation 6 (fc6 phases)
    (2, 12, 20, 96, 256, 1, 0, 1, 0, 1, 0, 0),     # 1x1 DMA kernel
    (1, 4, 70, 64, 256, 2, 0, 1, 0, 1, 0, 0),      # 2x2 valid: the LDS-DMA kernel with KS = 2 (route DMA2X2_128; the generic kernel's rows: tests/conv_route_cases.py)
    (1, 5, 40, 256, 97, 1, 0, 1, 0, 0, 1, 0),      # fp32 out
    (3, 40, 52, 512, 512, 3, 1, 1, 0, 1, 0, 0),    # long K loop
    (2, 32, 48, 64, 64, 3, 1, 1, 0, 1, 0, 1),      # fused 2x2 pool
    (2, 16, 70, 128, 128, 3, 1, 1, 0, 1, 0, 2),    # fused (2,1) pool
])
def test_conv_fp16_vs_fp64(reader_fp16, cfg):
    """The templated conv kernels on fp16 operands (v_mfma_f32_16x16x32_f16): fp32 accumulate, fp16 output rounding 2^-11 relative."""
    err, scale = _conv(reader_fp16, torch.float16, *cfg)
    tol = (2e-5 if cfg[10] else 8e-4) * scale
    assert err <= tol, (err, tol)


def test_heatmaps_fp16(reader_fp16, reader, oracle_reader):
    """Detector in fp16: the designed-weight heat-maps sit ~4x closer to the fp32 oracle than the bf16 ones, boxes stay identical; a fully
    random detector (27 stored layers) reaches relative L2 < 5e-3 (bf16: < 4e-2)."""
    import bb_ocr_amd
    from bb_ocr_amd import synth, weights
    from oracle import pipeline

    imgs = np.stack([synth.page(21 + i, width=384, height=256, lines=5, margin=24, colour=bool(i & 1))[0] for i in range(3)])
    dev = torch.from_numpy(imgs).cuda()
    h16, ratio = reader_fp16.heatmap_device(dev)
    hbf, _ = reader.heatmap_device(dev)
    e16 = ebf = 0.0
    for i in range(3):
        st, sl, r2 = oracle_reader.heatmap(imgs[i])
        want = np.stack([st, sl], -1)
        assert ratio == r2
        e16 = max(e16, np.abs(h16[i].cpu().numpy() - want).max())
        ebf = max(ebf, np.abs(hbf[i].cpu().numpy() - want).max())
    print(f"heat-map max |err|: fp16 {e16:.5f}  bf16 {ebf:.5f}")
    assert e16 <= HEAT_TOL_FP16 and e16 < ebf
    hori, free, polys = reader_fp16.boxes_from_heatmap(h16, ratio)
    hori2, free2, polys2 = reader.boxes_from_heatmap(hbf, ratio)
    assert polys == polys2 and hori == hori2 and free == free2
    cs, rs = weights.synthetic_craft_state(3), weights.synthetic_crnn_state(3)
    r = bb_ocr_amd.Reader(["en"], weights=(cs, rs), precision="fp16")
    try:
        ref = pipeline.OracleReader({k: torch.from_numpy(v) for k, v in cs.items()}, {k: torch.from_numpy(v) for k, v in rs.items()})
        img = synth.page(5, width=352, height=224, lines=4, margin=24, colour=True)[0]
        heat, _ = r.heatmap_device(torch.from_numpy(img[None]).cuda())
        st, sl, _ = ref.heatmap(img)
        want = np.stack([st, sl], -1)
        rel = np.linalg.norm(heat[0].cpu().numpy() - want) / np.linalg.norm(want)
        print(f"random detector, fp16: relative L2 {rel:.2e}")
        assert rel < 5e-3, rel
    finally:
        r.close()


def _logits(reader, crops16, n, W):
    T = W // 4 - 1
    out = torch.zeros((n, T, 112), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_crnn_logits(reader._h, C.c_void_p(crops16.data_ptr()), n, W, C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()[:, :, :97]


def test_crnn_logits_fp16_and_exact(reader, reader_fp16, reader_exact, oracle_reader):
    """Recogniser network alone on uint8-derived crops (what AlignCollate produces): relative L2 of the logits against the fp32 oracle --
    bf16 < 3e-2, fp16 < 4e-3, exact (split fp16, fp32 LSTM) < 2e-5 -- and in exact mode the arg-max of EVERY time step equals the oracle's."""
    rng = np.random.default_rng(23)
    for n, W in [(3, 128), (17, 64), (2, 320)]:
        g = rng.integers(0, 256, (n, 64, W), dtype=np.uint8)
        g = ((g.astype(np.int32) + np.roll(g, 1, 2) + np.roll(g, 1, 1)) // 3).astype(np.uint8)       # stroke-like rather than white noise
        x = ((g.astype(np.float32) / 255.0 - 0.5) / 0.5)[:, None]                                      # ToTensor + sub_(0.5).div_(0.5), fp32
        ref = oracle_reader._logits(x)
        lbf = _logits(reader, torch.from_numpy(x[:, 0]).to(torch.bfloat16).contiguous().cuda(), n, W)
        l16 = _logits(reader_fp16, torch.from_numpy(x[:, 0]).to(torch.float16).contiguous().cuda(), n, W)
        codes = torch.from_numpy((g.astype(np.int32) + 1).astype(np.int16)).contiguous().cuda()       # exact mode: 1 + grey level
        lex = _logits(reader_exact, codes, n, W)
        rel = lambda a: float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
        print(f"n={n} W={W}: logits relative L2  bf16 {rel(lbf):.2e}  fp16 {rel(l16):.2e}  exact {rel(lex):.2e}; "
              f"arg-max agreement bf16 {np.mean(lbf.argmax(-1) == ref.argmax(-1)):.4f} fp16 {np.mean(l16.argmax(-1) == ref.argmax(-1)):.4f}")
        assert rel(lbf) < 3e-2 and rel(l16) < 4e-3 and rel(lex) < 2e-5
        assert rel(l16) < rel(lbf)
        assert np.array_equal(lex.argmax(-1), ref.argmax(-1))


def _same_boxes(got, want):
    """Horizontal boxes are python ints on both sides, free boxes keep their float corners (upstream's shapes): equal values either way."""
    return len(got) == len(want) and all(np.array_equal(np.asarray(g[0], dtype=np.float64), np.asarray(w[0], dtype=np.float64))
                                         for g, w in zip(got, want))


def test_readtext_text_identity_by_mode(reader, reader_fp16, reader_exact, oracle_reader):
    """RANDOM recogniser weights (a stress test: near-zero top-2 margins on almost every box).  EXACT mode: every box's text equals the
    oracle's and the confidence agrees to 1e-3.  bf16 / fp16: identical boxes; their TEXT identity is asserted with hard counts on the
    trained recogniser in tests/test_gpu_parity_trained.py (with random weights 16 of 19 boxes flip in bf16, measured in round 2 -- that
    says nothing about a recogniser that reads)."""
    from bb_ocr_amd import synth

    n_exact = 0
    agree = {"bf16": [0, 0], "fp16": [0, 0]}
    for seed, colour in ((101, False), (102, True), (103, False)):
        img = synth.page(seed, width=512, height=320, lines=6, margin=24, colour=colour)[0]
        want = oracle_reader.readtext(img)
        assert len(want) >= 4
        for name, r in (("bf16", reader), ("fp16", reader_fp16)):
            got = r.readtext(img)
            assert _same_boxes(got, want), name
            agree[name][0] += sum(g[1] == w[1] for g, w in zip(got, want))
            agree[name][1] += len(want)
        got = reader_exact.readtext(img)
        assert _same_boxes(got, want)
        for (_, tg, cg), (_, tw, cw) in zip(got, want):
            assert tg == tw
            assert abs(cg - float(cw)) <= 1e-3 * max(float(cw), 1e-3)
        n_exact += len(got)
    print(f"random-weight recogniser: exact mode identical on {n_exact} boxes; boxes with identical text bf16 {agree['bf16']}, fp16 {agree['fp16']}")
    # no ordering of two noisy counts -- per TIME STEP instead: wherever the bf16 / fp16 recogniser's arg-max differs from the fp32
    # oracle's on these random weights, the oracle's own top-2 margin at that step is below the mode's logit noise bound
    from oracle import imgproc, recog

    img = synth.page(101, width=512, height=320, lines=6, margin=24)[0]
    _, grey = imgproc.reformat_input(img)
    hori, _ = oracle_reader.detect(img)
    crops = {}
    for b in hori:
        il, mw = recog.get_image_list([b], [], grey, model_height=64)
        if il:
            crops.setdefault(int(mw), []).append(il[0][1])
    bound = {"bf16": 6e-2, "fp16": 8e-3}                # of max |logit| (tests/test_gpu_parity_trained.py::STEP_MARGIN_BOUND)
    flips, steps = {"bf16": 0, "fp16": 0}, 0
    for Wc, lst in sorted(crops.items()):
        x = np.stack([recog.align_collate_one(c, 64, Wc)[0] for c in lst])
        ref = oracle_reader._logits(x[:, None])
        srt = np.sort(ref, axis=2)
        margin = (srt[..., -1] - srt[..., -2]) / np.abs(ref).max(axis=(1, 2), keepdims=True)[..., 0]
        steps += margin.size
        for name, r, dt in (("bf16", reader, torch.bfloat16), ("fp16", reader_fp16, torch.float16)):
            dev = torch.from_numpy(x).to(dt).contiguous().cuda()
            out = torch.zeros((len(lst), Wc // 4 - 1, 112), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r._check(r._lib.bbocr_crnn_logits(r._h, C.c_void_p(dev.data_ptr()), len(lst), Wc, C.c_void_p(out.data_ptr())))
            diff = out.cpu().numpy()[:, :, :97].argmax(-1) != ref.argmax(-1)
            flips[name] += int(diff.sum())
            assert not (diff & (margin >= bound[name])).any(), f"{name}: arg-max differs at a step whose oracle margin is {margin[diff].max():.3e}"
    print(f"random-weight recogniser, {steps} time steps: arg-max flips {flips}, all at oracle margins below {bound}")


def test_exact_mode_batch_and_retry_paths(reader_exact, oracle_reader):
    """EXACT mode through the batched entry (wide recogniser image, pooled sequence stage) with contrast_ths raised so that most boxes
    take the contrast-retry pass too: page results equal the single-page results and the oracle's texts / confidences."""
    from bb_ocr_amd import synth

    imgs = [synth.page(300 + i, width=448, height=288, lines=6, margin=24, colour=bool(i & 1))[0] for i in range(4)]
    kw = dict(contrast_ths=0.3)
    single = [reader_exact.readtext(im, **kw) for im in imgs]
    batched = reader_exact.readtext_batched(imgs, **kw)
    assert batched == single
    retried = 0
    for im, got in zip(imgs, single):
        want = oracle_reader.readtext(im, **kw)
        plain = oracle_reader.readtext(im)
        retried += sum(float(w[2]) != float(p[2]) for w, p in zip(want, plain))
        assert _same_boxes(got, want)
        assert [g[1] for g in got] == [w[1] for w in want]
        assert all(abs(g[2] - float(w[2])) <= 1e-3 * max(float(w[2]), 1e-3) for g, w in zip(got, want))
    assert retried > 0          # the retry pass really changed some results


@pytest.mark.parametrize("precision", ["bf16", "fp16", "exact"])
def test_weight_blob_export_import(states, precision):
    """Multi-GPU weight path on one card: a reader built from state-dicts exports its packed device blob (what rank 0 broadcasts over
    RCCL), a reader whose plans were only laid out (weights="empty") imports it and returns exactly the same results; blobs of another
    precision are refused with an error, not a fault."""
    import bb_ocr_amd
    from bb_ocr_amd import synth

    a = bb_ocr_amd.Reader(["en"], weights=states, precision=precision)
    b = bb_ocr_amd.Reader(["en"], weights="empty", precision=precision)
    try:
        blob = a.export_weights_blob()
        assert blob.is_cuda and blob.dtype == torch.uint8 and blob.numel() == b.weights_blob_size()
        mb = blob.numel() / 1e6
        assert (45 < mb < 60) if precision != "exact" else (130 < mb < 160), mb     # ~49 MB packed bf16 / fp16; exact: every layer of BOTH networks as a split plan, 3x
        img = synth.page(41, width=384, height=256, lines=5, margin=24, colour=True)[0]
        assert b.readtext(img) != a.readtext(img) or a.readtext(img) == []         # before the import: zero weights
        b.import_weights_blob(blob)
        for seed in (41, 42):
            img = synth.page(seed, width=384, height=256, lines=5, margin=24, colour=bool(seed & 1))[0]
            assert b.readtext(img) == a.readtext(img) and len(a.readtext(img)) >= 4
        other = bb_ocr_amd.Reader(["en"], weights="empty", precision="fp16" if precision == "bf16" else "bf16")
        try:
            with pytest.raises((RuntimeError, ValueError)):
                other.import_weights_blob(blob)
        finally:
            other.close()
    finally:
        a.close()
        b.close()


def test_a4_batch16_fp16_properties(reader_fp16, reader, reader_exact, oracle_reader):
    """BASELINE.json configs[4] per-GPU share on the fp16 MFMA path: 16 dense A4@300dpi scans (2480x3504 -> canvas 1824x2560, the resize
    path at full size) in one call.  Size-independent properties: copies of a page agree, a page's result does not depend on its batch,
    no page-height box arises from the black canvas stripe, fp16 and bf16 find the same boxes; and one page against the oracle's
    detector (boxes identical)."""
    from bb_ocr_amd import synth

    kw = dict(width=2480, height=3504, lines=110, font_size=20, word_gap=14, line_pitch=31, margin=60)
    uniq = [synth.page(1234 + i, colour=bool(i & 1), **kw)[0] for i in range(4)]
    rgb = torch.from_numpy(np.stack([uniq[i % 4] for i in range(16)])).cuda()
    out = reader_fp16.readtext_device(rgb)
    assert len(out) == 16 and all(out[i] == out[i % 4] for i in range(16))
    assert all(90 <= len(p) <= 130 for p in out), [len(p) for p in out]
    for page in out[:4]:
        heights = [max(pt[1] for pt in b) - min(pt[1] for pt in b) for b, _, _ in page]
        assert max(heights) < 120                                   # line boxes, never the 3504-pixel stripe box
    assert reader_fp16.readtext_device(rgb[5:6])[0] == out[5]
    # (on the 0.73x down-scaled page the strokes are anti-aliased and some threshold decisions sit inside bf16's 0.04 heat-map noise:
    #  bf16 finds the same lines with a few box edges one pixel off; fp16's 0.0025 keeps the oracle's boxes, asserted below)
    bf = reader.readtext_device(rgb[:2])
    assert all(abs(len(a) - len(b)) <= 2 for a, b in zip(bf, out[:2]))       # (bf16 flips ~100 of 1.2 M threshold decisions per page: tools/flip_report.py)
    # integer stages at full A4 scale: the product's boxes == the oracle's box extraction run on the SAME (device) heat-map, exactly
    from oracle import boxes as obox

    heat, ratio = reader_fp16.heatmap_device(rgb[1:2])
    hori, free, polys = reader_fp16.boxes_from_heatmap(heat, ratio)
    hh = heat[0].cpu().numpy()
    oh, of, op = obox.detect_from_heatmap(hh[..., 0], hh[..., 1], ratio)
    assert [list(map(int, p)) for p in op] == polys[0] and [list(map(int, b)) for b in oh] == hori[0] and len(of) == len(free[0])
    # against the oracle's own fp32 detector (one CRAFT forward on the CPU, ~15 s per page): box indices are integer outputs -- the fp16 path
    # returns the oracle's boxes EXACTLY (grouped and free, same order), on two pages, and none of the threshold decisions flips
    # ... and so does the exact mode's split-fp16 detector (round 4), whose heat-maps follow the oracle's to ~1e-5 on the canvas-resized scan
    for k in (1, 2):
        st, sl, r2 = oracle_reader.heatmap(uniq[k])
        oh, of, op = obox.detect_from_heatmap(st, sl, r2)
        for name, rd in (("fp16", reader_fp16), ("exact", reader_exact)):
            heat, ratio = rd.heatmap_device(rgb[k:k + 1])
            hori, free, polys = rd.boxes_from_heatmap(heat, ratio)
            hh = heat[0].cpu().numpy()
            flips = int(((hh[..., 0] > 0.4) != (st > 0.4)).sum() + ((hh[..., 1] > 0.4) != (sl > 0.4)).sum())
            err = max(float(np.abs(hh[..., 0] - st).max()), float(np.abs(hh[..., 1] - sl).max()))
            print(f"A4 page {k}, {name} vs the fp32 oracle detector: {flips} threshold flips, max |heat error| {err:.2e}, {len(oh)} grouped + {len(of)} free boxes")
            assert flips == 0 and ratio == r2, name
            assert name != "exact" or err < 5e-5
            assert [list(map(int, p)) for p in op] == polys[0], name
            assert [list(map(int, b)) for b in oh] == hori[0], name
            assert len(of) == len(free[0]) and all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)) for a, b in zip(of, free[0])), name


def test_noise_sensitive_detector_flip_rates(reader, reader_fp16):
    """VERDICT r2 item 8 / SURVEY.md section 7 "measure flip rate": a detector in which EVERY trunk layer feeds every heat-map pixel (seeded
    random CRAFT, last 1x1 layer rescaled so the maps span the thresholds) -- unlike the designed ink detector, whose lattice-valued maps
    keep every decision far from rounding noise.  Reduced precision then flips a measurable share of the `> 0.4` / `>= 0.7` decisions
    against the fp32 oracle; the measured rates (profiles/r03_flip_report.json: bf16 ~0.3 % of the pixels, fp16 ~0.04 %) are pinned here
    with a 2x allowance, and fp16 must stay >= 4x below bf16.  Box identity on such maps is therefore statistical in bf16 / fp16 -- with a
    trained CRAFT the flip rate lies between this detector's and the designed one's (0)."""
    import bb_ocr_amd
    from bb_ocr_amd import synth
    from conftest import noise_sensitive_craft
    from oracle import pipeline

    cs, rs = noise_sensitive_craft()
    ref = pipeline.OracleReader({k: torch.from_numpy(v) for k, v in cs.items()}, {k: torch.from_numpy(v) for k, v in rs.items()})
    pages = [synth.page(910 + i, width=640, height=480, lines=10, margin=24, colour=bool(i & 1))[0] for i in range(2)]
    want = [ref.heatmap(p) for p in pages]
    rate = {}
    for prec in ("bf16", "fp16"):
        r = bb_ocr_amd.Reader(["en"], weights=(cs, rs), precision=prec)
        try:
            flips = px = 0
            for img, (st, sl, ratio) in zip(pages, want):
                heat, _ = r.heatmap_device(torch.from_numpy(img[None].copy()).cuda())
                h = heat[0].cpu().numpy()
                flips += int(((h[..., 0] > 0.4) != (st > 0.4)).sum() + ((h[..., 1] > 0.4) != (sl > 0.4)).sum() + ((h[..., 0] >= 0.7) != (st >= 0.7)).sum())
                px += 3 * st.size
            rate[prec] = flips / px
        finally:
            r.close()
    print(f"noise-sensitive detector: share of threshold decisions that differ from the fp32 oracle: {rate}")
    assert 0 < rate["bf16"] <= FLIP_BOUND["bf16"] and rate["fp16"] <= FLIP_BOUND["fp16"] and rate["fp16"] * 4 <= rate["bf16"]


def test_exact_mode_detector_follows_the_fp32_oracle_on_arbitrary_maps():
    """precision="exact" runs the DETECTOR in split fp16 too (pair tensors, three MFMA product terms per layer, the reference's operation order):
    on the noise-sensitive detector above -- where fp16 flips 0.03 % and bf16 0.3 % of the threshold decisions -- its heat-maps follow the fp32
    oracle's to ~1e-6 and NONE of the `> 0.4` / `> 0.4` / `>= 0.7` decisions of 4 pages differs; polygons, grouped boxes and free boxes are
    the oracle's, in order (getDetBoxes_core thresholds behind enhanced_extractor.py:520)."""
    import bb_ocr_amd
    from bb_ocr_amd import synth
    from conftest import noise_sensitive_craft
    from oracle import boxes as obox
    from oracle import pipeline

    cs, rs = noise_sensitive_craft()
    ref = pipeline.OracleReader({k: torch.from_numpy(v) for k, v in cs.items()}, {k: torch.from_numpy(v) for k, v in rs.items()})
    pages = [synth.page(910 + i, width=640, height=480, lines=10, margin=24, colour=bool(i & 1))[0] for i in range(4)]
    r = bb_ocr_amd.Reader(["en"], weights=(cs, rs), precision="exact")
    try:
        heat, ratio = r.heatmap_device(torch.from_numpy(np.stack(pages)).cuda())
        hori, free, polys = r.boxes_from_heatmap(heat, ratio)
        n_boxes = worst = 0
        for i, img in enumerate(pages):
            st, sl, r2 = ref.heatmap(img)
            h = heat[i].cpu().numpy()
            err = max(float(np.abs(h[..., 0] - st).max()), float(np.abs(h[..., 1] - sl).max()))
            worst = max(worst, err)
            flips = int(((h[..., 0] > 0.4) != (st > 0.4)).sum() + ((h[..., 1] > 0.4) != (sl > 0.4)).sum() + ((h[..., 0] >= 0.7) != (st >= 0.7)).sum())
            oh, of, op = obox.detect_from_heatmap(st, sl, r2)                     # the oracle's boxes from ITS OWN fp32 maps
            n_boxes += len(oh) + len(of)
            assert flips == 0 and ratio == r2, (i, flips, err)
            assert [list(map(int, p)) for p in op] == polys[i], i
            assert [list(map(int, b)) for b in oh] == hori[i], i
            assert len(of) == len(free[i]) and all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)) for a, b in zip(of, free[i])), i
        print(f"exact detector vs fp32 oracle on the noise-sensitive CRAFT: max |heat error| {worst:.2e}, 0 flips of {3 * 4 * 240 * 320} decisions, {n_boxes} boxes identical")
        assert worst < 2e-5 and n_boxes > 40
    finally:
        r.close()


FLIP_BOUND = {"bf16": 0.012, "fp16": 0.0016}      # 2x the measured share (profiles/r03_flip_report.json)


def test_detector_heatmaps_are_bit_reproducible():
    """Round 4: the fused upconv4 kernel (conv3x3_up4_kernel, round 2) passed a bare s_barrier with a patch read still queued; on tiles after a
    workgroup's first a faster wave's LDS writes for the NEXT tile could be served before it, and ~1 % of the heat-map values then differed
    from run to run (hidden by the designed detector's lattice-valued maps, inside every tolerance test).  A detector in which every layer
    feeds every pixel shows it: heat-maps must be bit-identical call to call, after other work has dirtied the work buffers, and page by
    page vs batched -- at a size with one tile per persistent workgroup and at 1280x960 (many tiles per workgroup), in every mode."""
    import bb_ocr_amd
    from bb_ocr_amd import synth
    from conftest import noise_sensitive_craft

    cs, rs = noise_sensitive_craft()
    small = np.stack([synth.page(910 + i, width=640, height=480, lines=10, margin=24, colour=bool(i & 1))[0] for i in range(4)])
    big = np.stack([synth.page(50 + i)[0] for i in range(3)])
    for prec in ("bf16", "fp16", "exact"):
        r = bb_ocr_amd.Reader(["en"], weights=(cs, rs), precision=prec)
        try:
            for pages, other in ((small, big), (big, small)):
                rgb, rgb_other = torch.from_numpy(pages).cuda(), torch.from_numpy(other).cuda()
                first = r.heatmap_device(rgb)[0].cpu().numpy()
                for _ in range(8 if prec != "exact" else 2):
                    assert np.array_equal(first, r.heatmap_device(rgb)[0].cpu().numpy()), (prec, pages.shape)
                r.readtext_device(rgb_other)
                assert np.array_equal(first, r.heatmap_device(rgb)[0].cpu().numpy()), (prec, pages.shape, "after other work")
                single = np.concatenate([r.heatmap_device(rgb[i:i + 1])[0].cpu().numpy() for i in range(len(pages))])
                assert np.array_equal(first, single), (prec, pages.shape, "page by page")
            # ... and with two calls in flight on the context (two call slots, sequence stages on their own streams)
            if prec != "exact":
                from concurrent.futures import ThreadPoolExecutor

                tb, ts = torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()
                wb, ws = r.heatmap_device(tb)[0].cpu().numpy(), r.heatmap_device(ts)[0].cpu().numpy()
                full = r.readtext_device(tb)

                def job(k):
                    if k % 3 == 0:
                        return np.array_equal(wb, r.heatmap_device(tb)[0].cpu().numpy())
                    if k % 3 == 1:
                        return np.array_equal(ws, r.heatmap_device(ts)[0].cpu().numpy())
                    return r.readtext_device(tb) == full

                with ThreadPoolExecutor(max_workers=2) as ex:
                    assert all(ex.map(job, range(18))), (prec, "two calls in flight")
            # the recogniser network alone: logits of 40 random crops, call to call
            g = torch.Generator().manual_seed(5)
            x = torch.rand(40, 64, 512, generator=g) * 2 - 1
            dev = ((x * 127.5 + 127.5).round().clamp(0, 255) + 1).to(torch.int16) if prec == "exact" else x.to(torch.bfloat16 if prec == "bf16" else torch.float16)
            dev = dev.contiguous().cuda()
            outs = []
            for _ in range(4):
                out = torch.zeros((40, 127, 112), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                r._check(r._lib.bbocr_crnn_logits(r._h, C.c_void_p(dev.data_ptr()), 40, 512, C.c_void_p(out.data_ptr())))
                outs.append(out.cpu().numpy()[:, :, :97])
            assert all(np.array_equal(outs[0], o) for o in outs[1:]), (prec, "recogniser logits")
        finally:
            r.close()
