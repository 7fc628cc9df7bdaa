"""What decoder='beamsearch' costs: `readtext_device` on 64-page 1280x960 batches with the greedy decoder (the ceiling), with beamsearch at
width 5 (readtext's default beamWidth) and at width BBOCR_BEAM_DEVICE_MAX (the widest beam the device search takes).

    python tools/bench_beam.py [--pages 64] [--steps 5] [--warmup 2] [--precision fp16] [--label NAME] [--one-step MODE]

Workload: bench.py's -- `--pages` synthetic pages of 1280x960 already on the card, the recogniser trained on them -- with one
`readtext_device` call per step (one call in flight: the stage times of a call are then that call's alone).  Per mode the batch is warmed up, then timed `--steps` times (host clock around calls that
return synchronised); the rate is pages / median step.  The strings of the beam modes are compared with the greedy ones (boxes and
confidences must be equal, strings may differ).  Appends one JSON line per mode to profiles/bench_beam.jsonl and prints it; `--label`
names the build in the line (A/B runs of two libraries on one machine: BBOCR_LIB_PATH selects the library).
`--one-step MODE` (greedy | beam5 | beammax) runs the warm-up and then ONE step of that mode and writes nothing: the step to put under a
memory-copy trace when the bytes of its device-to-host copies are the question.
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
    ap.add_argument("--one-step", default=None, choices=("greedy", "beam5", "beammax"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_beam.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import _lib, synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench_beam needs a GPU: nothing is measured without one")
    wmax = getattr(_lib, "BEAM_DEVICE_MAX", 32)              # a build from before the device search: the same width, on its host path
    modes = {"greedy": dict(), "beam5": dict(decoder="beamsearch", beamWidth=5), "beammax": dict(decoder="beamsearch", beamWidth=wmax)}
    # bench.py's weights: the recogniser trained on these pages.  What a beam search costs depends on how many classes pass the candidate
    # threshold per step; random recogniser weights would make nearly all 97 pass at every step, which no trained model does
    rec = weights.load_npz_state(os.path.join(ROOT, "tests", "golden", "crnn_synth_fp16.npz"))
    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), rec), precision=a.precision)
    rgb = torch.from_numpy(np.stack([synth.page(1234 + i, colour=bool(i & 1))[0] for i in range(a.pages)])).cuda()
    assert tuple(rgb.shape[1:]) == (960, 1280, 3), rgb.shape
    torch.cuda.synchronize()
    if a.one_step:
        for _ in range(a.warmup):
            reader.readtext_device(rgb, **modes[a.one_step])
        torch.cuda.synchronize()
        out = reader.readtext_device(rgb, **modes[a.one_step])
        print(json.dumps(dict(bench="beam_one_step", mode=a.one_step, boxes=sum(len(p) for p in out))), flush=True)
        reader.close()
        return
    keys = ("detector_net", "ccl_device", "box_geometry_host", "crops", "recognizer_net", "ctc", "contrast_retry", "total")
    want = None
    for mode, kw in modes.items():
        for _ in range(a.warmup):
            out = reader.readtext_device(rgb, **kw)
        ts, stage = [], dict.fromkeys(keys, 0.0)
        for _ in range(a.steps):
            t = time.perf_counter()
            out = reader.readtext_device(rgb, **kw)
            ts.append(time.perf_counter() - t)
            for key, v in reader.stage_times().items():
                stage[key] += v / a.steps
        if want is None:
            want = out
        same_boxes = [[(b[0], b[2]) for b in p] for p in out] == [[(b[0], b[2]) for b in p] for p in want]
        changed = sum(b[1] != g[1] for p, q in zip(out, want) for b, g in zip(p, q))
        row = dict(bench="beam", label=a.label, mode=mode, beam_width=kw.get("beamWidth", 0), precision=a.precision, pages=a.pages,
                   boxes=sum(len(p) for p in out), boxes_and_confidences_equal_greedy=bool(same_boxes), strings_changed_by_the_search=changed,
                   pages_per_s=round(a.pages / float(np.median(ts)), 1), step_s=[round(v, 4) for v in ts],
                   stage_ms={key: round(v, 2) for key, v in stage.items()})
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    reader.close()


if __name__ == "__main__":
    main()
