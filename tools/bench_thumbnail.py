"""The extractor's OCR-input down-scaling (enhanced_extractor.py:486-512) on the device (csrc/thumb.hip) against the host path.

    python tools/bench_thumbnail.py [--pages 16] [--reps 20] [--dir DIR] [--device-only]

Generates its own 5712x4284 JPEG pages (synth.py pages up-scaled, quality 92) in DIR (default: a temporary directory) and prints JSON lines:
  * the device time of bbocr_ocr_thumbnail (cover rule: 1600 px, JPEG q90) for one 24-Mpixel RGB page and for one 55-Mpixel gray page
    (8568x6426, the size f2's 1.5x resize gives such a photograph), and the host time of the same step (_ocr_input_array, one core);
  * extract_texts pages/s on the directory with device_thumbnail False / True, with and without use_preprocessing + crop_for_ocr.
--device-only: the two device timings alone (for a separate `rocprofv3 --kernel-trace --stats` run).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pages(d, n):
    from PIL import Image

    from bb_ocr_amd import synth

    paths = []
    for k in range(n):
        p = os.path.join(d, f"page{k:03d}.jpg")
        if not os.path.exists(p):
            img, _ = synth.page(900 + k, width=1280, height=960, lines=20)
            Image.fromarray(img).resize((5712, 4284), Image.BICUBIC).save(p, quality=92)
        paths.append(p)
    return paths


def device_ms(reader, page_dev, reps):
    import torch

    from bb_ocr_amd.preprocess import ocr_input_device

    ocr_input_device(reader, page_dev, 0)                          # warm-up (tables, buffers)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        ocr_input_device(reader, page_dev, 0)
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, weights
    from bb_ocr_amd.preprocess import _imread_bgr

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    d = a.dir or tempfile.mkdtemp(prefix="bench_thumb_")
    os.makedirs(d, exist_ok=True)
    paths = make_pages(d, 1 if a.device_only else a.pages)
    bgr = _imread_bgr(paths[0])
    from PIL import Image

    gray = np.asarray(Image.fromarray(bgr[:, :, 1]).resize((8568, 6426), Image.BICUBIC))
    for name, host in (("rgb_24mpix", bgr), ("gray_55mpix", gray)):
        dev = reader._to_dev(host)
        row = dict(leg="device_step", page=name, shape=list(host.shape), device_ms=round(device_ms(reader, dev, a.reps), 3))
        if not a.device_only:
            t = time.perf_counter()
            extractor_batch._ocr_input_array(host, 0)
            row["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        print(json.dumps(row), flush=True)
    if a.device_only:
        return
    for crops in (False, True):
        kw = dict(use_preprocessing=True, crop_for_ocr=True) if crops else {}
        for dev in (False, True):
            extractor_batch.extract_texts(reader, paths[:2], device_thumbnail=dev, **kw)          # warm-up
            t = time.perf_counter()
            res = extractor_batch.extract_texts(reader, paths, device_thumbnail=dev, **kw)
            dt = time.perf_counter() - t
            print(json.dumps(dict(leg="extract_texts", crops=crops, device_thumbnail=dev, pages=len(paths), seconds=round(dt, 2),
                                  pages_per_s=round(len(paths) / dt, 2), chars=sum(len(v) for v in res.values()))), flush=True)


if __name__ == "__main__":
    main()
