"""``cv2.imread`` on the device (csrc/jpegdec.hip + csrc/orient.hip: preprocess.imread_bgr_device) against the host path
(preprocess._imread_bgr + upload), per page and through the extractor's crop settings.

    python tools/bench_imread.py [--pages 16] [--reps 5] [--runs 3] [--dir DIR] [--out profiles/bench_imread.jsonl] [--kernel-only]

Builds its own page in DIR (default: a temporary directory): tests/golden/photos/IMG_9684.JPG up-scaled to 5712x4284, JPEG quality 92,
4:2:0, one restart interval per MCU row, EXIF orientation 6 -- the shape of the reference's iPhone photographs -- plus a progressive and a
PNG copy of it for the two host-decode paths, and --pages copies of the first for the extractor legs.  JSON lines, printed and written to --out:
  * leg "imread": per page, host _imread_bgr + upload against imread_bgr_device, for each of its three paths (median of --reps);
  * leg "extract_texts": extract_texts(use_preprocessing=True, crop_for_ocr=True, device_thumbnail=True) on the pages with device_decode off
    and on, alternating, --runs runs each: medians and ranges of pages/s.
--kernel-only: for a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_imread.py --kernel-only` run: the decoded page
(YCBCR4) through page_orient -> BGR at orientations 1, 3, 6, 8 and through bbocr_op_ycc_to_rgb, 1 + --reps launches each, in that order.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHOTO = os.path.join(ROOT, "tests", "golden", "photos", "IMG_9684.JPG")


def make_pages(d, n):
    """-> (the n JPEG pages, the progressive copy, the PNG copy)"""
    from PIL import Image

    first = os.path.join(d, "page000.jpg")
    prog, png = os.path.join(d, "progressive.jpg"), os.path.join(d, "page.png")
    if not (os.path.exists(first) and os.path.exists(prog) and os.path.exists(png)):
        img = Image.open(PHOTO).convert("RGB").resize((5712, 4284), Image.BICUBIC)
        exif = Image.Exif()
        exif[0x0112] = 6
        img.save(first, "JPEG", quality=92, restart_marker_rows=1, exif=exif)
        img.save(prog, "JPEG", quality=92, progressive=True, exif=exif)
        img.save(png, "PNG", compress_level=1, exif=exif)
    data = open(first, "rb").read()
    paths = [first]
    for k in range(1, n):
        paths.append(os.path.join(d, f"page{k:03d}.jpg"))
        if not os.path.exists(paths[-1]):
            with open(paths[-1], "wb") as f:
                f.write(data)
    return paths, prog, png


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
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_imread.jsonl"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, weights
    from bb_ocr_amd.preprocess import PAGE_BGR, PAGE_YCBCR4, _imread_bgr, imread_bgr_device, orient_page_device
    from bb_ocr_amd.reader import decode_file_ycc, jpeg_plan

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    d = a.dir or tempfile.mkdtemp(prefix="bench_imread_")
    os.makedirs(d, exist_ok=True)
    paths, prog, png = make_pages(d, 1 if a.kernel_only else a.pages)
    plan = jpeg_plan(open(paths[0], "rb").read())
    assert plan.supported and plan.orientation == 6 and plan.segments == plan.mcu_rows and (plan.width, plan.height) == (5712, 4284)

    if a.kernel_only:
        ycc = decode_file_ycc(paths[0], padded=True)
        if ycc.shape[2] != 4:                                     # Pillow without the zero-copy export: pad here
            import numpy as np

            ycc = np.concatenate([ycc, np.full(ycc.shape[:2] + (1,), 255, np.uint8)], axis=2)
        dev = reader._to_dev(ycc)
        for o in (1, 3, 6, 8):
            for _ in range(1 + a.reps):
                orient_page_device(reader, dev, PAGE_YCBCR4, o, PAGE_BGR)
        for _ in range(1 + a.reps):
            reader.pages_from_ycc(dev[None])
        torch.cuda.synchronize()
        print(json.dumps(dict(leg="kernel_only", page=list(ycc.shape), order=["page_orient o=1", "o=3", "o=6", "o=8", "ycc_to_rgb_gray"],
                              launches_each=1 + a.reps)))
        return

    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for name, path in (("jpeg", paths[0]), ("ycc", prog), ("rgb", png)):
        got = imread_bgr_device(reader, path)
        assert got.imread_path == name and torch.equal(got, reader._to_dev(_imread_bgr(path)))
        del got
        host, host_range = median_ms(lambda: reader._to_dev(_imread_bgr(path)), a.reps)
        dev, dev_range = median_ms(lambda: imread_bgr_device(reader, path), a.reps)
        emit(dict(leg="imread", path=name, file=os.path.basename(path), file_bytes=os.path.getsize(path), shape=[5712, 4284, 3], orientation=6,
                  host_imread_upload_ms=host, host_range_ms=host_range, imread_bgr_device_ms=dev, device_range_ms=dev_range))

    kw = dict(use_preprocessing=True, crop_for_ocr=True, device_thumbnail=True)
    for flag in (False, True):
        extractor_batch.extract_texts(reader, paths[:2], device_decode=flag, **kw)          # warm-up
    rates = {False: [], True: []}
    chars = {}
    for _ in range(a.runs):
        for flag in (False, True):
            t = time.perf_counter()
            res = extractor_batch.extract_texts(reader, paths, device_decode=flag, **kw)
            rates[flag].append(len(paths) / (time.perf_counter() - t))
            chars[flag] = sum(len(v) for v in res.values())
    for flag in (False, True):
        r = rates[flag]
        emit(dict(leg="extract_texts", device_decode=flag, pages=len(paths), runs=a.runs, options=kw, pages_per_s_median=round(statistics.median(r), 2),
                  pages_per_s_range=[round(min(r), 2), round(max(r), 2)], chars=chars[flag]))
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
