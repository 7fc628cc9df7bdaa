"""The trace previews' PNG file written on the device (png="device": Reader.encode_png, csrc/pngenc.hip) against Pillow's writer
(png="pillow", the default and the reference's bytes).

    python tools/bench_png.py [--pages 4] [--device-pages 64] [--rounds 3] [--dir DIR] [--out profiles/bench_png.jsonl]

Writes JSON lines; the two writers are measured alternately `--rounds` times in one process, so the "pillow" figure of a row is the
yardstick of its "device" figure:
  * leg "preview_800": preprocess.preview_device over bench_preview.py's 5712x4284 4:2:0 JPEG pages (decode at scale 2, thumbnail to 800
    pixels, PNG, base64) -- host wall time per preview and the PNG files' sizes;
  * leg "page_600x800": preview_device over `--device-pages` BGR pages of 600x800 already on the card (no resize: the page itself is
    written) -- host wall time per preview and the files' sizes;
  * leg "encode_600x800": the writer alone on those pages' RGB pixels -- Reader.encode_png between two HIP events recorded on the caller's
    stream (the call is synchronous, so the span covers its kernels, its two read-backs, the copy of the file to the host and the host
    framing) and its host wall time, against the wall time of Pillow's Image.save from a host array (Pillow has no device part).
Every preview of the device writer is decoded and compared with Pillow's: mode, size, pixels.
A directory the tool created itself is removed when it ends.
"""
import argparse
import base64
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_preview import make_pages, timed  # noqa: E402


def png_bytes(url):
    return base64.b64decode(url.split(",", 1)[1])


def same_image(a, b):
    import numpy as np
    from PIL import Image

    x, y = Image.open(io.BytesIO(png_bytes(a))), Image.open(io.BytesIO(png_bytes(b)))
    return x.mode == y.mode and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)) and x.info.get("icc_profile") == y.info.get("icc_profile")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--device-pages", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_png.jsonl"))
    a = ap.parse_args()
    import bb_ocr_amd
    from bb_ocr_amd import weights

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    d = a.dir or tempfile.mkdtemp(prefix="bench_png_")
    os.makedirs(d, exist_ok=True)
    try:
        rows = run(a, reader, d)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def run(a, reader, d):
    import numpy as np
    import torch
    from PIL import Image

    from bb_ocr_amd import synth
    from bb_ocr_amd.preprocess import PAGE_RGB, preview_device

    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def preview_leg(leg, items, timing, **extra):
        for png in ("pillow", "device"):
            preview_device(reader, items[0], png=png)                     # warm-up (buffers, tables)
        for r in range(max(3, a.rounds)):
            tp, sp = timed(lambda x: preview_device(reader, x, png="pillow"), items)
            td, sd = timed(lambda x: preview_device(reader, x, png="device"), items)
            assert all(same_image(x, y) for x, y in zip(sd, sp))
            emit(leg=leg, round=r, pages=len(items), pillow_ms_per_preview=round(tp * 1e3 / len(items), 2),
                 device_ms_per_preview=round(td * 1e3 / len(items), 2), pillow_previews_per_s=round(len(items) / tp, 2),
                 device_previews_per_s=round(len(items) / td, 2), pillow_png_bytes=sum(len(png_bytes(x)) for x in sp),
                 device_png_bytes=sum(len(png_bytes(x)) for x in sd), timing=timing, **extra)

    # ---- the whole preview of a 24-megapixel JPEG file
    datas = [open(p, "rb").read() for p in make_pages(d, a.pages)]
    preview_leg("preview_800", datas, "host wall clock around a device synchronise", size=[5712, 4284])

    # ---- pages already on the card
    pages = [np.ascontiguousarray(synth.page(900 + k, width=800, height=600, lines=14, colour=True)[0]) for k in range(a.device_pages)]
    bgr = [reader._to_dev(np.ascontiguousarray(p[:, :, ::-1])) for p in pages]
    preview_leg("page_600x800", bgr, "host wall clock around a device synchronise", size=[800, 600])

    # ---- the writer alone
    rgb = [reader._to_dev(p) for p in pages]

    def pillow_save(p):
        buf = io.BytesIO()
        Image.fromarray(p).save(buf, format="PNG")
        return buf.getvalue()

    def encode_events(t):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        data = reader.encode_png(t, PAGE_RGB)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), data

    reader.encode_png(rgb[0], PAGE_RGB), pillow_save(pages[0])
    for r in range(max(3, a.rounds)):
        tp, fp = timed(pillow_save, pages)
        td, fd = timed(encode_events, rgb)
        ev = sorted(x[0] for x in fd)
        assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(x[1]))), p) for x, p in zip(fd, pages))
        emit(leg="encode_600x800", round=r, pages=len(pages), pillow_save_ms=round(tp * 1e3 / len(pages), 2),
             device_call_wall_ms=round(td * 1e3 / len(pages), 3), device_call_event_ms_median=round(ev[len(ev) // 2], 3),
             device_call_event_ms_max=round(ev[-1], 3), pillow_png_bytes=sum(len(x) for x in fp), device_png_bytes=sum(len(x[1]) for x in fd),
             timing="HIP events on the caller's stream around the synchronous call; host wall clock for the *_wall_ms / *_save_ms figures")
    return rows


if __name__ == "__main__":
    main()
