"""The extractor's model-input image (enhanced_extractor.py:399-411) on the device (csrc/thumb.hip + csrc/jpegenc.hip:
preprocess.model_image_device, extractor_batch.encode_images_for_model) against ``preprocess.model_image_host`` (Pillow) on the same box,
in the same run.

    python tools/bench_model_image.py [--reps 5] [--dir DIR] [--out profiles/bench_model_image.jsonl]

Pages: the two committed photographs (tests/golden/photos) and a synthetic 5712x4284 page built in DIR (default: a temporary directory):
the first photograph up-scaled, JPEG quality 92, 4:2:0 -- the shape of the reference's iPhone photographs.  JSON lines, printed and
written to --out, one per page and rule ((2000, 88) and (3200, 95), enhanced_extractor.py:809-810); every device result is first checked
to equal the host's bytes:
  * host_ms                 model_image_host(path): Pillow's decode, thumbnail and JPEG save on one core;
  * device_from_file_ms     the file's bytes -> device decoder -> thumbnail -> encoder -> the JPEG's bytes (encode_images_for_model with
                            device_decode=True);
  * device_from_pixels_ms   thumbnail + encoder of the page already on the card (model_image_device);
  * encode_only_ms          Reader.encode_jpeg of the thumbnailed RGB page alone;
medians of --reps with their ranges, and images/s of the first two.
"""
import argparse
import base64
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHOTOS = [os.path.join(ROOT, "tests", "golden", "photos", n) for n in ("IMG_9684.JPG", "IMG_9685.JPG")]


def synthetic_page(d):
    from PIL import Image

    path = os.path.join(d, "page_5712x4284.jpg")
    if not os.path.exists(path):
        Image.open(PHOTOS[0]).convert("RGB").resize((5712, 4284), Image.BICUBIC).save(path, "JPEG", quality=92)
    return path


def median_ms(f, reps):
    import torch

    f()                                                           # warm-up (buffers, file cache)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 2), [round(min(ts), 2), round(max(ts), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_model_image.jsonl"))
    a = ap.parse_args()
    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, weights
    from bb_ocr_amd.preprocess import PAGE_RGB, PAGE_YCBCR4, model_image_device, model_image_host, ocr_thumbnail_device
    from bb_ocr_amd.reader import jpeg_page

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    d = a.dir or tempfile.mkdtemp(prefix="bench_model_image_")
    os.makedirs(d, exist_ok=True)
    rows = []
    for path in PHOTOS + [synthetic_page(d)]:
        page = jpeg_page(path)
        assert page is not None, path
        for max_dim, quality in ((2000, 88), (3200, 95)):
            rule = lambda i: (max_dim, quality)
            want = model_image_host(path, max_dim, quality)
            from_file = lambda: extractor_batch.encode_images_for_model(reader, [path], device_decode=True, rule=rule)
            assert base64.b64decode(from_file()[0]) == want, "the device file differs from Pillow's"
            ycc, status = reader.decode_jpeg_batch([page], padded=True)
            assert status[0] == 0
            from_pixels = lambda: model_image_device(reader, ycc[0], PAGE_YCBCR4, max_dim, quality)
            assert from_pixels() == want
            H, W = page.shape[:2]
            small = ocr_thumbnail_device(reader, ycc[0], PAGE_YCBCR4, max_dim, 0)[0] if max(H, W) > max_dim else None
            encode = (lambda: reader.encode_jpeg(small, PAGE_RGB, quality, components=3)) if small is not None else from_pixels
            host, host_range = median_ms(lambda: model_image_host(path, max_dim, quality), a.reps)
            t_file, r_file = median_ms(from_file, a.reps)
            t_px, r_px = median_ms(from_pixels, a.reps)
            t_enc, r_enc = median_ms(encode, a.reps)
            row = dict(leg="model_image", file=os.path.basename(path), file_bytes=os.path.getsize(path), shape=[H, W], max_dim=max_dim, quality=quality,
                       out_bytes=len(want), reps=a.reps, host_ms=host, host_range_ms=host_range, device_from_file_ms=t_file,
                       device_from_file_range_ms=r_file, device_from_pixels_ms=t_px, device_from_pixels_range_ms=r_px, encode_only_ms=t_enc,
                       encode_only_range_ms=r_enc, host_images_per_s=round(1e3 / host, 2), device_images_per_s=round(1e3 / t_file, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ycc, small
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
