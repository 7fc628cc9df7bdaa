"""Pages of mixed shapes: one device batch per SHAPE (the by-shape grouping of Reader.readtext_batched / extractor_batch.read_files)
against one `readtext_pages` call per mixed batch (their `mixed=True`), on the same pages already on the card.

    python tools/bench_mixed_pages.py [--pages 64] [--k 1,4,16,64] [--reps 5] [--precision fp16]

Workload: `--pages` synthetic pages of about 1280x960 in k distinct shapes (page i has shape i % k; each side differs from 1280 / 960 by a
few multiples of 8 pixels, on and off the detector's 32-pixel grid; k = 64: one shape per page).  Per k:
  (a) by shape: the pages of a shape stacked into one device batch, the batches streamed with two calls in flight (readtext_stream) --
      the device side of `readtext_batched(mixed=False)`, the parent behaviour; for k = 64 that is 64 one-page calls;
  (b) mixed: the page list cut by `mixed_batches` (page count, pixel budget), each batch one readtext_pages call, two in flight
      (readtext_pages_stream) -- the device side of `readtext_batched(mixed=True)`.
How to read the ratio: `readtext_batched` itself takes HOST arrays and uploads them, so it cannot read pages already on the card; the tool
runs the two device loops that it runs, on device pages.  The per-shape `torch.stack` of (a) is done once, outside the timed region (in
`readtext_batched` the upload produces the stacked batch, at no extra copy), so the ratio compares device calls only: no decode, no H2D,
no stacking on either side.
Both are warmed up on every shape, then timed alternately `--reps` times (host clock around calls that return synchronised); results are
compared (they must be equal).  stage_times come from one further serial pass of each path (summed over its calls).  Appends one JSON
line per k to profiles/bench_mixed_pages.jsonl and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes_for(k):
    """k distinct (H, W): 960 + 8 a, 1280 + 8 b with a, b in -4 .. 3, the plain shape first"""
    steps = (0, 1, -1, 2, -2, 3, -3, -4)
    grid = [(steps[i], steps[j]) for i, j in sorted(((i, j) for i in range(8) for j in range(8)), key=lambda t: (t[0] + t[1], t[0]))]   # both sides vary from k = 4 on
    return [(960 + 8 * a, 1280 + 8 * b) for a, b in grid[:k]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--k", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_pages.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import synth, weights
    from bb_ocr_amd.reader import mixed_batches

    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed_pages needs a GPU: nothing is measured without one")
    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)), precision=a.precision)
    max_pages = int(os.environ.get("BBOCR_MAX_DEVICE_BATCH", "64"))
    # one base page per index, a little larger than any shape: page i of every k is its top-left crop (made contiguous: "already on the card")
    base = [torch.from_numpy(synth.page(60_000 + i, width=1280 + 24, height=960 + 24)[0]).cuda() for i in range(a.pages)]
    keys = ("detector_net", "ccl_device", "box_geometry_host", "crops", "recognizer_net", "ctc", "contrast_retry", "total")
    for k in [int(v) for v in a.k.split(",")]:
        shapes = shapes_for(min(k, 64))
        pages = [base[i][:shapes[i % k][0], :shapes[i % k][1]].contiguous() for i in range(a.pages)]
        by_shape = {}
        for i, p in enumerate(pages):
            by_shape.setdefault(tuple(p.shape), []).append(i)
        groups = [idx[c:c + max_pages] for idx in by_shape.values() for c in range(0, len(idx), max_pages)]
        stacks = [torch.stack([pages[i] for i in g]) for g in groups]
        mixes = mixed_batches([p.shape[0] * p.shape[1] for p in pages], max_pages)
        torch.cuda.synchronize()

        def run_a(stream=True):
            out, times = [None] * len(pages), dict.fromkeys(keys, 0.0)
            results = reader.readtext_stream(iter(stacks)) if stream else None
            for g, s in zip(groups, stacks):
                res = next(results) if stream else reader.readtext_device(s)
                if not stream:
                    for key, v in reader.stage_times().items():
                        times[key] += v
                for i, r in zip(g, res):
                    out[i] = r
            return out, times

        def run_b(stream=True):
            out, times = [None] * len(pages), dict.fromkeys(keys, 0.0)
            lists = [[pages[i] for i in m] for m in mixes]
            results = reader.readtext_pages_stream(iter(lists)) if stream else None
            for m, l in zip(mixes, lists):
                res = next(results) if stream else reader.readtext_pages(l)
                if not stream:
                    for key, v in reader.stage_times().items():
                        times[key] += v
                for i, r in zip(m, res):
                    out[i] = r
            return out, times

        want, _ = run_a()                                   # warm-up of every shape on both paths (buffers, code objects) ...
        got, _ = run_b()
        equal = got == want                                 # ... and the check that faster is not different
        run_a()
        run_b()
        ta, tb = [], []
        for _ in range(a.reps):                             # alternating, so that drift of the shared host hits both alike
            t = time.perf_counter()
            run_a()
            ta.append(time.perf_counter() - t)
            t = time.perf_counter()
            run_b()
            tb.append(time.perf_counter() - t)
        _, st_a = run_a(stream=False)
        _, st_b = run_b(stream=False)
        rate = lambda ts: round(len(pages) / float(np.median(ts)), 1)
        row = dict(bench="mixed_pages", precision=a.precision, pages=len(pages), k=k, calls_by_shape=len(stacks), calls_mixed=len(mixes),
                   boxes=sum(len(r) for r in want), results_equal=bool(equal),
                   by_shape_pages_per_s=rate(ta), mixed_pages_per_s=rate(tb), ratio=round(float(np.median(ta)) / float(np.median(tb)), 3),
                   by_shape_s=[round(v, 4) for v in ta], mixed_s=[round(v, 4) for v in tb],
                   stage_ms_by_shape={key: round(v, 2) for key, v in st_a.items()}, stage_ms_mixed={key: round(v, 2) for key, v in st_b.items()})
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    reader.close()


if __name__ == "__main__":
    main()
