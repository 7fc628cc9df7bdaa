"""Device text-region auto-crop (csrc/autocrop.hip) per page, after the device f2 pre-processing and the extractor's edge crop.

    python tools/bench_autocrop.py --cases DIR [--reps 10] [--cpu]

DIR/cases.json lists {"name", "percent", "margin"}; DIR/<name>.jpg is the photograph and, when present, DIR/<name>_auto_cropped.png the
800-px preview of the crop the reference extractor stored -- the device crop's thumbnail is compared with it (pixels equal, same size).
Prints one JSON line per page (f2 ms, auto-crop ms, box, preview agreement) and a summary line.  --cpu also times the numpy / scipy
restatement of tests/autocrop_ref.py on each page (that is not OpenCV's time: cv2 is not a dependency of this project).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image

    import bb_ocr_amd
    from bb_ocr_amd import weights
    from bb_ocr_amd.preprocess import _imread_bgr, auto_crop_box_device, central_edge_crop_box, preprocess_bgr_device

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    cases = json.load(open(os.path.join(a.cases, "cases.json")))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rows = []
    for c in cases:
        bgr = _imread_bgr(os.path.join(a.cases, c["name"] + ".jpg"))
        dev = reader._to_dev(bgr)
        f2 = preprocess_bgr_device(reader, dev)                       # warm-up (tables, buffers)
        t0, t1 = ev(), ev()
        t0.record()
        for _ in range(a.reps):
            f2 = preprocess_bgr_device(reader, dev)
        t1.record()
        t1.synchronize()
        f2_ms = t0.elapsed_time(t1) / a.reps
        b = central_edge_crop_box(f2.shape[0], f2.shape[1], c["percent"])
        view = f2[b[1]:b[3], b[0]:b[2]] if b else f2
        box = auto_crop_box_device(reader, view, c["margin"])        # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            box = auto_crop_box_device(reader, view, c["margin"])
        ac_ms = (time.perf_counter() - t) * 1e3 / a.reps
        row = dict(page=c["name"], f2_shape=list(f2.shape), view_shape=list(view.shape), f2_ms=round(f2_ms, 3), autocrop_ms=round(ac_ms, 3),
                   box=list(box) if box else None)
        host = view.contiguous().cpu().numpy()
        crop = host[box[1]:box[3], box[0]:box[2]] if box else host
        prev = os.path.join(a.cases, c["name"] + "_auto_cropped.png")
        if os.path.exists(prev):
            want = np.asarray(Image.open(prev).convert("L"))
            th = Image.fromarray(crop)
            th.thumbnail((800, 800))
            got = np.asarray(th)
            row["preview_size"] = [want.shape[1], want.shape[0]]
            row["thumb_size"] = [got.shape[1], got.shape[0]]
            row["preview_equal"] = float((got == want).mean()) if got.shape == want.shape else None
        if a.cpu:
            import autocrop_ref

            t = time.perf_counter()
            cbox, _ = autocrop_ref.auto_crop(host, c["margin"])
            row["cpu_restatement_s"] = round(time.perf_counter() - t, 2)
            row["cpu_box_equal"] = (cbox == box)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(summary=True, mean_autocrop_ms=round(float(np.mean([r["autocrop_ms"] for r in rows])), 3),
                          mean_f2_ms=round(float(np.mean([r["f2_ms"] for r in rows])), 3))))
    reader.close()


if __name__ == "__main__":
    main()
