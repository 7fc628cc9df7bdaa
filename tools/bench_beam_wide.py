"""What decoder='beamsearch' costs on recognisers of more than 128 classes, with the search on the card (Reader(beam_wide=True), route 4)
and on the host (route 1, which reads the probabilities back): `readtext_device` on 64-page 1280x960 batches at 352, 2,200 and 6,719 classes,
widths 5 and BBOCR_BEAM_DEVICE_MAX, with the greedy rate of the same run as the ceiling.

    python tools/bench_beam_wide.py [--pages 64] [--steps 4] [--warmup 1] [--precision fp16] [--label NAME] [--classes 352,2200,6719]
                                    [--widths 5,32] [--only host|device]

Workload: bench.py's -- `--pages` synthetic pages of 1280x960 already on the card and the recogniser trained on them, its 97 Prediction rows
scattered into C classes (tools/bench_wide_classes.py's model: blank at 0, every other class zero weights and bias -30), so it reads the
same text and the passes have the same rows whatever C is.  One `readtext_device` call per step (one call in flight: the stage times are
that call's alone), host clock around calls that return synchronised.  Following measuring-on-mi355x, what is compared is ALTERNATED: per
(C, width) the device route and the host route take turns step by step in one process, after `--warmup` untimed steps each, and every
figure is the median with its minimum and maximum.  `--only device` (or `host`) times that route alone, step after step: a host-route
step leaves the card idle for hundreds of milliseconds, and the device-route step that follows it in the alternation runs slower than one
that follows another device-route step; the rows of such a run carry `alone: true`.

A build from before the option (`--label parent` with BBOCR_LIB_PATH naming its library) has the host route only; it is measured in a
process of its own, and processes of the two builds are alternated on one card by the caller (three times each).

Appends one JSON line per (C, mode) to profiles/bench_beam_wide.jsonl: pages/s, the stage time `ctc` (ms per step), the route the call
reported and, for the device route, the number of sequences per step that overflowed the candidate list and were searched on the host.
The device route's strings, boxes and confidences are compared with the host route's: they must be equal.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_wide_classes import spread, wide_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--classes", default="352,2200,6719")
    ap.add_argument("--widths", default="5,32")
    ap.add_argument("--only", default=None, choices=("host", "device"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_beam_wide.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import _lib, synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_wide needs a GPU: nothing is measured without one")
    # a build from before the option exports none of its entry points (a Reader without the option goes through bbocr_create): host route only
    probe = C.CDLL(_lib.LIB_PATH)
    has_option = hasattr(probe, "bbocr_op_ctc_beam_wide")
    if not has_option:
        for name in ("bbocr_create_v2", "bbocr_op_ctc_beam_wide", "bbocr_host_ctc_route", "bbocr_last_ctc_host_sequences"):
            _lib.PROTOTYPES.pop(name, None)
    rec = weights.load_npz_state(os.path.join(ROOT, "tests", "golden", "crnn_synth_fp16.npz"))
    craft = weights.designed_craft_state(0)
    rgb = torch.from_numpy(np.stack([synth.page(1234 + i, colour=bool(i & 1))[0] for i in range(a.pages)])).cuda()
    assert tuple(rgb.shape[1:]) == (960, 1280, 3), rgb.shape
    torch.cuda.synchronize()

    def step(reader, kw):
        t = time.perf_counter()
        out = reader.readtext_device(rgb, **kw)
        dt = time.perf_counter() - t
        return out, dt, reader.stage_times()["ctc"], reader.last_ctc_route(), (reader.last_ctc_host_sequences() if has_option else 0)

    def record(row):
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for Cn in [int(v) for v in a.classes.split(",")]:
        state, chars = wide_model(rec, Cn)
        readers = {"host": bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=(craft, state), precision=a.precision)}
        if has_option:
            readers["device"] = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=(craft, state), precision=a.precision, beam_wide=True)
        base = dict(bench="beam_wide", label=a.label, classes=Cn, precision=a.precision, pages=a.pages, alone=a.only is not None)
        # the ceiling: greedy (the fused kernel), on the reader every build has
        for _ in range(a.warmup):
            step(readers["host"], {})
        runs = [step(readers["host"], {}) for _ in range(a.steps)]
        greedy = runs[-1][0]
        record(dict(base, mode="greedy", beam_width=0, route=runs[-1][3], boxes=sum(len(p) for p in greedy),
                    pages_per_s=spread([a.pages / r[1] for r in runs]), ctc_ms=spread([r[2] for r in runs])))
        for w in [int(v) for v in a.widths.split(",")]:
            kw = dict(decoder="beamsearch", beamWidth=w)
            want = step(readers["host"], kw)[0] if a.only == "device" else None        # the host route's results, to compare with
            timed = {name: r for name, r in readers.items() if a.only in (None, name)}
            for r in timed.values():
                for _ in range(a.warmup):
                    step(r, kw)
            runs = {name: [] for name in timed}
            for _ in range(a.steps):                           # host, device, host, device, ...
                for name, r in timed.items():
                    runs[name].append(step(r, kw))
            for name, rr in runs.items():
                out = rr[-1][0]
                record(dict(base, mode=name, beam_width=w, route=rr[-1][3], boxes=sum(len(p) for p in out),
                            equal_to_the_host_route=bool(out == (want if want is not None else runs["host"][-1][0])),
                            strings_changed_by_the_search=sum(b[1] != g[1] for p, q in zip(out, greedy) for b, g in zip(p, q)),
                            sequences_searched_on_the_host_per_step=(max(r[4] for r in rr) if name == "device" else None),
                            pages_per_s=spread([a.pages / r[1] for r in rr]), ctc_ms=spread([r[2] for r in rr])))
        for r in readers.values():
            r.close()


if __name__ == "__main__":
    main()
