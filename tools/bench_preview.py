"""The processing trace's previews (enhanced_extractor.py:184-199) on the device against the host path.

    python tools/bench_preview.py [--pages 4] [--rounds 3] [--dir DIR] [--out profiles/bench_preview.jsonl]

Generates its own 5712x4284 4:2:0 JPEG pages (synth.py pages up-scaled, quality 92) in DIR (default: a temporary directory) and writes
JSON lines, each pair measured alternately `--rounds` times on the same box:
  * previews per second of preprocess.preview_device against preprocess.preview_host (one host core) over the pages, 800 px -- both
    return the same strings, which is checked;
  * the device time per page of the scaled decode (bbocr_jpeg_decode_scaled, scale 2, + bbocr_thumbnail_box) against the full-scale
    decode followed by the whole-image thumbnail (bbocr_jpeg_decode + bbocr_ocr_thumbnail) -- these two give different pixels; only
    the first is Pillow's -- and of the two decodes alone;
  * where a device preview's time goes, part by part: reading the file, planning it, the second Image.open for the ICC profile, the
    pixels on the card (host-side unstuffing and upload included), the download, Pillow's PNG writer + base64;
  * extractor_batch.trace_previews per page with the shared entropy pass (one bbocr_jpeg_decode_scales call: the 1/2 decode and the
    oriented full-scale page) against the two-pass sequence it replaces, the whole trace and the card's share alone, with the entropy
    runs per page that bbocr_jpeg_counters saw;
  * preview_device(device_decode="chroma") on 4:4:4 and 4:2:2 versions of the pages against preview_host (same strings, checked).
Every figure is a WALL time of the host around work that ends in a device synchronise (each row says so in `timing`), not a kernel time.
A directory the tool created itself is removed when it ends.
"""
import argparse
import json
import io
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pages(d, n):
    from PIL import Image

    from bb_ocr_amd import synth

    paths = []
    for k in range(n):
        p = os.path.join(d, f"page{k:03d}.jpg")
        if not os.path.exists(p):
            img, _ = synth.page(700 + k, width=1280, height=960, lines=20, colour=True)
            Image.fromarray(img).resize((5712, 4284), Image.BICUBIC).save(p, quality=92)
        paths.append(p)
    return paths


def timed(fn, items):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    out = [fn(x) for x in items]
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_preview.jsonl"))
    a = ap.parse_args()
    import bb_ocr_amd
    from bb_ocr_amd import weights
    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    d = a.dir or tempfile.mkdtemp(prefix="bench_preview_")
    os.makedirs(d, exist_ok=True)
    try:
        run(a, reader, d)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


def run(a, reader, d):
    import torch
    from PIL import Image

    from bb_ocr_amd.preprocess import (PAGE_YCBCR4, _png_data_url, _preview_jpeg_device, ocr_thumbnail_device, preview_device, preview_host,
                                       thumbnail_box_device)
    from bb_ocr_amd.reader import JpegPage, draft_scale, jpeg_plan

    paths = make_pages(d, a.pages)
    datas = [open(p, "rb").read() for p in paths]
    plans = [jpeg_plan(x) for x in datas]
    assert all(p.supported and (p.width, p.height) == (5712, 4284) for p in plans)
    rows = []

    def emit(**row):
        row["timing"] = "host wall clock around a device synchronise"
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- previews per second, device against host
    preview_device(reader, datas[0])                                      # warm-up (buffers, tables)
    preview_host(datas[0])
    for r in range(a.rounds):
        td, sd = timed(lambda x: preview_device(reader, x), datas)
        th, sh = timed(preview_host, datas)
        assert sd == sh
        emit(leg="preview_800", round=r, pages=len(datas), size=[5712, 4284], device_previews_per_s=round(len(datas) / td, 2),
             host_previews_per_s=round(len(datas) / th, 2), device_ms_per_page=round(td * 1e3 / len(datas), 1),
             host_ms_per_page=round(th * 1e3 / len(datas), 1))

    # ---- scaled decode against full-scale decode + thumbnail (device pixels only; nothing is downloaded)
    s = draft_scale(5712, 4284, 1600, 1600)
    assert s == 2

    def scaled(k):
        t, st = reader.decode_jpeg_batch([JpegPage(datas[k], plans[k])], padded=True, scale=s)
        assert st == [0]
        return thumbnail_box_device(reader, t[0], PAGE_YCBCR4, 600, 800, 5712 / s, 4284 / s)

    def full(k):
        t, st = reader.decode_jpeg_batch([JpegPage(datas[k], plans[k])], padded=True)
        assert st == [0]
        return ocr_thumbnail_device(reader, t[0], PAGE_YCBCR4, 800, 0)[0]

    def decode_only(scale):
        return lambda k: reader.decode_jpeg_batch([JpegPage(datas[k], plans[k])], padded=True, scale=scale)[1]

    idx = list(range(len(datas)))
    scaled(0), full(0)
    for r in range(a.rounds):
        ts, _ = timed(scaled, idx)
        tf, _ = timed(full, idx)
        t2, _ = timed(decode_only(s), idx)
        t1, _ = timed(decode_only(1), idx)
        emit(leg="decode_to_800", round=r, pages=len(idx), scale=s, scaled_decode_plus_box_ms=round(ts * 1e3 / len(idx), 2),
             full_decode_plus_thumbnail_ms=round(tf * 1e3 / len(idx), 2), scaled_decode_ms=round(t2 * 1e3 / len(idx), 2),
             full_decode_ms=round(t1 * 1e3 / len(idx), 2))
    # ---- the parts of one device preview (preview_device's own steps, one after the other)
    clock = time.perf_counter
    for r in range(a.rounds):
        parts = dict.fromkeys(("read_file", "plan", "icc_open", "device_pixels", "download", "png_base64"), 0.0)
        for p in paths:
            t0 = clock()
            data = open(p, "rb").read()
            t1 = clock()
            plan = jpeg_plan(data)
            t2 = clock()
            icc = Image.open(io.BytesIO(data)).info.get("icc_profile")
            t3 = clock()
            px = _preview_jpeg_device(reader, data, plan, 800)
            torch.cuda.synchronize()
            t4 = clock()
            host = px.cpu().numpy()
            t5 = clock()
            img = Image.fromarray(host)
            if icc:
                img.info["icc_profile"] = icc
            _png_data_url(img)
            t6 = clock()
            for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                parts[k] += dt
        emit(leg="preview_parts_ms_per_page", round=r, pages=len(paths), **{k: round(v * 1e3 / len(paths), 2) for k, v in parts.items()})
    trace_legs(a, reader, paths, datas, plans, emit)
    chroma_legs(a, reader, d, emit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


TRACE_KW = dict(use_preprocessing=True, edge_crop_percent=4.0, crop_for_ocr=True, crop_margin=32)


def trace_two_passes(reader, path, **kw):
    """trace_previews as it ran before the shared pass: the file decoded at the draft scale for the original's preview (preview_device)
    and again at full scale for the crop chain (ocr_page_crop -> imread_bgr_device) -- two runs of the entropy stages"""
    from bb_ocr_amd.extractor_batch import TRACE_KEYS, ocr_page_crop
    from bb_ocr_amd.preprocess import preview_device

    data = open(path, "rb").read()
    trace = {"original_b64": preview_device(reader, data)}
    pages = {}
    ocr_page_crop(reader, data, on_device=True, device_decode=True, pages=pages, **kw)
    for step, page in pages.items():
        trace[TRACE_KEYS[step]] = preview_device(reader, page)
    return trace


def trace_legs(a, reader, paths, datas, plans, emit):
    """(a) trace_previews per page with the shared entropy pass against the two-pass sequence it replaces: the whole trace (four PNG
    writes included) and the card's share of it alone -- one bbocr_jpeg_decode_scales call against bbocr_jpeg_decode_scaled + bbocr_jpeg_imread"""
    from bb_ocr_amd.extractor_batch import trace_previews
    from bb_ocr_amd.reader import JpegPage

    pages = [JpegPage(x, p) for x, p in zip(datas, plans)]

    def shared(k):
        return reader.decode_jpeg_scales_batch([pages[k]], (1, 2), imread=True)[1]

    def two(k):
        return reader.decode_jpeg_batch([pages[k]], padded=True, scale=2)[1], reader.imread_jpeg_batch([pages[k]])[1]

    idx = list(range(len(pages)))
    shared(0), two(0)
    assert trace_previews(reader, paths[:1], **TRACE_KW)[0] == trace_two_passes(reader, paths[0], **TRACE_KW)        # and the warm-up
    for r in range(a.rounds):
        c0 = reader.jpeg_counters()
        ts, _ = timed(lambda p: trace_previews(reader, [p], **TRACE_KW), paths)
        c1 = reader.jpeg_counters()
        tt, _ = timed(lambda p: trace_two_passes(reader, p, **TRACE_KW), paths)
        c2 = reader.jpeg_counters()
        ds, _ = timed(shared, idx)
        dt, _ = timed(two, idx)
        n = len(paths)
        emit(leg="trace_page", round=r, pages=n, size=[5712, 4284], shared_pass_ms_per_page=round(ts * 1e3 / n, 1),
             two_passes_ms_per_page=round(tt * 1e3 / n, 1), shared_pass_entropy_runs_per_page=(c1["entropy_runs"] - c0["entropy_runs"]) / n,
             two_passes_entropy_runs_per_page=(c2["entropy_runs"] - c1["entropy_runs"]) / n, shared_decode_ms=round(ds * 1e3 / n, 2),
             two_decodes_ms=round(dt * 1e3 / n, 2))


def chroma_legs(a, reader, d, emit):
    """(b) preview_device(device_decode="chroma") on 4:4:4 and 4:2:2 versions of the pages against preview_host (same strings, checked)"""
    from PIL import Image

    from bb_ocr_amd.preprocess import preview_device, preview_host
    from bb_ocr_amd.reader import jpeg_plan

    for name, sub in (("4:4:4", 0), ("4:2:2", 1)):
        datas = []
        for p in make_pages(d, a.pages):
            buf = io.BytesIO()
            Image.open(p).save(buf, "JPEG", quality=92, subsampling=sub)
            datas.append(buf.getvalue())
        assert all(jpeg_plan(x).chroma == sub + 1 for x in datas)
        info = {}
        assert preview_device(reader, datas[0], device_decode="chroma", info=info) == preview_host(datas[0]) and info["route"] == "device-jpeg"
        for r in range(a.rounds):
            td, sd = timed(lambda x: preview_device(reader, x, device_decode="chroma"), datas)
            th, sh = timed(preview_host, datas)
            assert sd == sh
            emit(leg="preview_800_chroma", sampling=name, round=r, pages=len(datas), size=[5712, 4284],
                 device_ms_per_page=round(td * 1e3 / len(datas), 1), host_ms_per_page=round(th * 1e3 / len(datas), 1))


if __name__ == "__main__":
    main()
