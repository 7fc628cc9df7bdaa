"""What decoder='wordbeamsearch' costs: `readtext_device` on 64-page 1280x960 batches with the word search on the device (route 6) at widths
5 and BBOCR_BEAM_DEVICE_MAX, against the host route (route 5) of the same build, with the `beamsearch` and `greedy` figures of the same run
as ceilings.

    python tools/bench_wordbeam.py [--pages 64] [--steps 5] [--warmup 2] [--precision fp16] [--label NAME] [--host-width 33] [--distractors 20000]

Workload: bench.py's pages and trained recogniser, as tools/bench_beam.py; the dictionary is the synthetic pages' own word list (both
capitalisations) plus `--distractors` random lower-case strings.  The library routes a pass by its width, its classes and its longest
sequence, and has no switch that would send a width-5 pass to the host, so the host legs are forced HERE, by `--host-width`: the narrowest
width the library gives to the host is BBOCR_BEAM_DEVICE_MAX + 1, and the host legs run at it.  They are therefore the host route's cost
at width 33, next to the device's at 32; the host route at width 5 is not measured by this tool.  Device and host legs alternate step by step.
Appends one JSON line per leg to profiles/bench_wordbeam.jsonl (`--out`) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--host-width", type=int, default=None)
    ap.add_argument("--distractors", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_wordbeam.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import _lib, synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench_wordbeam needs a GPU: nothing is measured without one")
    wmax = _lib.BEAM_DEVICE_MAX
    whost = a.host_width if a.host_width is not None else wmax + 1
    if whost <= wmax:
        raise SystemExit(f"--host-width must exceed {wmax}: narrower passes run on the device")
    rec = weights.load_npz_state(os.path.join(ROOT, "tests", "golden", "crnn_synth_fp16.npz"))
    pages = [synth.page(1234 + i, colour=bool(i & 1)) for i in range(a.pages)]
    rng = np.random.default_rng(1)
    words = sorted({w for _, boxes in pages for b in boxes for w in (b[4], b[4].lower(), b[4].capitalize())})
    words += ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 12)))) for _ in range(a.distractors)]
    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), rec), precision=a.precision, dictionary=words)
    rgb = torch.from_numpy(np.stack([p[0] for p in pages])).cuda()
    assert tuple(rgb.shape[1:]) == (960, 1280, 3), rgb.shape
    torch.cuda.synchronize()
    modes = {"greedy": dict(), "beam5": dict(decoder="beamsearch", beamWidth=5), f"beam{wmax}": dict(decoder="beamsearch", beamWidth=wmax),
             "word5_device": dict(decoder="wordbeamsearch", beamWidth=5), f"word{wmax}_device": dict(decoder="wordbeamsearch", beamWidth=wmax),
             f"word{whost}_host": dict(decoder="wordbeamsearch", beamWidth=whost)}
    keys = ("detector_net", "ccl_device", "box_geometry_host", "crops", "recognizer_net", "ctc", "contrast_retry", "total")
    ts = {m: [] for m in modes}
    stage = {m: dict.fromkeys(keys, 0.0) for m in modes}
    out, route = {}, {}
    for m, kw in modes.items():
        for _ in range(a.warmup):
            reader.readtext_device(rgb, **kw)
    for _ in range(a.steps):                       # the legs alternate: drift of the machine lands on all of them alike
        for m, kw in modes.items():
            t = time.perf_counter()
            out[m] = reader.readtext_device(rgb, **kw)
            ts[m].append(time.perf_counter() - t)
            route[m] = reader.last_ctc_route()
            for key, v in reader.stage_times().items():
                stage[m][key] += v / a.steps
    want = out["greedy"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for m, kw in modes.items():
        same_boxes = [[(b[0], b[2]) for b in p] for p in out[m]] == [[(b[0], b[2]) for b in p] for p in want]
        row = dict(bench="wordbeam", label=a.label, mode=m, beam_width=kw.get("beamWidth", 0), ctc_route=route[m], precision=a.precision, pages=a.pages,
                   dictionary=reader.dictionary_stats(), boxes=sum(len(p) for p in out[m]), boxes_and_confidences_equal_greedy=bool(same_boxes),
                   strings_differ_from_greedy=sum(b[1] != g[1] for p, q in zip(out[m], want) for b, g in zip(p, q)),
                   strings_differ_from_beam5=sum(b[1] != g[1] for p, q in zip(out[m], out["beam5"]) for b, g in zip(p, q)),
                   pages_per_s=round(a.pages / float(np.median(ts[m])), 1), step_s=[round(v, 4) for v in ts[m]],
                   stage_ms={key: round(v, 2) for key, v in stage[m].items()})
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    reader.close()


if __name__ == "__main__":
    main()
