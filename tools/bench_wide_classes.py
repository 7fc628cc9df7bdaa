"""What a recogniser of more than 128 classes costs: the recognition stage of `readtext_device` on 64-page 1280x960 batches at 97 classes
(english_g2: the no-regression reading, to be taken with this build and with its parent's) and at 352, 2,200 and 6,719 classes, and the two
routes through Prediction + CTC -- fused (pred_ctc_kernel) and unfused (the conv plan + ctc_rows_wide_kernel) -- alternated in one process.

    python tools/bench_wide_classes.py [--pages 64] [--steps 5] [--warmup 2] [--rows 32768] [--reps 7] [--precision fp16] [--label NAME]
                                       [--widths 97,352,2200,6719]

Workload: bench.py's -- `--pages` synthetic pages of 1280x960 already on the card and the recogniser trained on them.  A wide model is
that recogniser with its 97 Prediction rows scattered into C classes (blank at 0, every other class zero weights and bias -30), so it reads
the same text and the passes have the same rows whatever C is.  Following measuring-on-mi355x: every figure is taken after `--warmup`
untimed repetitions; things that are compared are ALTERNATED in one process (A B A B ...), never run block after block; and each figure
is reported as median with its minimum and maximum, so that a difference can be held against the spread.

Rows of profiles/bench_wide_classes.jsonl (appended, one JSON object per line):
  bench = "wide_readtext": per width, `readtext_device` per step -- pages/s and the stage times `recognizer_net` + `ctc` (ms per step), the
      widths alternated step by step.  `--widths 97` runs on a build from before the feature too (the parent's reading: check this file out
      beside it, `--label parent`).
  bench = "wide_routes": per width > 128, `--rows` rows of the second BiLSTM stage's output (uniform +-1) through bbocr_op_pred_ctc (fused) and
      through bbocr_op_pred + bbocr_op_ctc_rows (unfused), alternated `--reps` times: host wall time around calls that return
      synchronised, ns per row; both include one device-to-device copy of x resp. of the logits that a recognition pass does not make, and the
      unfused route a second synchronised call.  The kernels' own times: `rocprofv3 --kernel-trace --stats -- python tools/bench_wide_classes.py
      --routes-only --widths C` (one width per run: the stats are per kernel name) -> profiles/wide_classes_kernel_stats.csv.
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


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def wide_model(rec, Cn, seed=5):
    from bb_ocr_amd.reader import CHARSET

    pos = np.sort(np.random.default_rng(seed).choice(np.arange(1, Cn), size=96, replace=False))
    state = dict(rec)
    w = np.zeros((Cn, 256), np.float32)
    b = np.full(Cn, -30.0, np.float32)
    w[0], b[0] = rec["Prediction.weight"][0], rec["Prediction.bias"][0]
    w[pos], b[pos] = rec["Prediction.weight"][1:], rec["Prediction.bias"][1:]
    state["Prediction.weight"], state["Prediction.bias"] = w, b
    chars = [chr(0x4E00 + k) for k in range(Cn - 1)]
    for p, ch in zip(pos, CHARSET):
        chars[p - 1] = ch
    return state, chars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--widths", default="97,352,2200,6719")
    ap.add_argument("--routes-only", action="store_true", help="skip the readtext rows: only the stage entry points run (the run to put under a "
                    "kernel trace, where Prediction's conv kernel must not be mixed with the other GEMMs of a recognition pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_wide_classes.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_classes needs a GPU: nothing is measured without one")
    widths = [int(v) for v in a.widths.split(",")]
    rec = weights.load_npz_state(os.path.join(ROOT, "tests", "golden", "crnn_synth_fp16.npz"))
    craft = weights.designed_craft_state(0)
    readers = {}
    for Cn in widths:
        if Cn == 97:
            readers[Cn] = bb_ocr_amd.Reader(["en"], gpu=True, weights=(craft, rec), precision=a.precision)
        else:
            state, chars = wide_model(rec, Cn)
            readers[Cn] = bb_ocr_amd.Reader(["xx"], gpu=True, character=chars, weights=(craft, state), precision=a.precision)
    rgb = torch.from_numpy(np.stack([synth.page(1234 + i, colour=bool(i & 1))[0] for i in range(a.pages)])).cuda()
    torch.cuda.synchronize()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    # ---- the recognition stage inside readtext_device, the widths alternated step by step
    texts = {}
    for Cn, r in ({} if a.routes_only else readers).items():
        for _ in range(a.warmup):
            texts[Cn] = r.readtext_device(rgb)
    ts = {Cn: [] for Cn in widths}
    st = {Cn: {"recognizer_net": [], "ctc": []} for Cn in widths}
    for _ in range(0 if a.routes_only else a.steps):
        for Cn, r in readers.items():
            t = time.perf_counter()
            r.readtext_device(rgb)
            ts[Cn].append(time.perf_counter() - t)
            times = r.stage_times()
            for key in st[Cn]:
                st[Cn][key].append(times[key])
    base = texts.get(widths[0])
    for Cn in ([] if a.routes_only else widths):
        same = [[(b[0], b[1]) for b in p] for p in texts[Cn]] == [[(b[0], b[1]) for b in p] for p in base]
        emit(dict(bench="wide_readtext", label=a.label, classes=Cn, precision=a.precision, pages=a.pages, boxes=sum(len(p) for p in texts[Cn]),
                  boxes_and_strings_equal_first_width=bool(same), pages_per_s=round(a.pages / float(np.median(ts[Cn])), 1), step_s=spread(ts[Cn]),
                  recognizer_net_ms=spread(st[Cn]["recognizer_net"]), ctc_ms=spread(st[Cn]["ctc"])))

    # ---- the two routes through Prediction + CTC on the same rows, alternated
    for Cn, r in readers.items():
        if Cn <= 128:
            continue
        lib, h = r._lib, r._h
        cs = (Cn + 15) // 16 * 16
        rows = min(a.rows, ((1 << 30) // (cs * 4)) // 256 * 256)
        dt = torch.bfloat16 if a.precision == "bf16" else torch.float16
        x = (torch.rand((rows, 256), device="cuda") * 2 - 1).to(dt)
        logits = torch.empty((rows, cs), dtype=torch.float32, device="cuda")
        idx = torch.empty(rows, dtype=torch.int32, device="cuda")
        pmax = torch.empty(rows, dtype=torch.float32, device="cuda")
        oidx = torch.empty(rows, dtype=torch.int32, device="cuda")
        T = 64                                                   # sequences of 64 steps, as crops of 256 pixel columns give: the collapse's serial
        nseq = rows // T                                         # product runs over T steps, not over all rows
        cout = torch.empty((nseq, 4), dtype=torch.int32, device="cuda")
        seq = (C.c_int * (2 * nseq))(*[v for i in range(nseq) for v in (i * T, T)])
        p = lambda t: C.c_void_p(t.data_ptr())

        def fused():
            r._check(lib.bbocr_op_pred_ctc(h, p(x), rows, None, 0, p(idx), p(pmax)))

        def unfused():
            r._check(lib.bbocr_op_pred(h, p(x), rows, p(logits)))
            r._check(lib.bbocr_op_ctc_rows(h, p(logits), rows, Cn, cs, None, seq, nseq, None, p(idx), p(pmax), p(oidx), p(cout)))

        for _ in range(a.warmup):
            fused()
            unfused()
        tf, tu = [], []
        for _ in range(a.reps):
            for fn, acc in ((fused, tf), (unfused, tu)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t) * 1e9 / rows)
        fused()
        i1 = idx.clone()
        unfused()
        emit(dict(bench="wide_routes", label=a.label, classes=Cn, precision=a.precision, rows=rows, fused_ns_per_row=spread(tf),
                  unfused_ns_per_row=spread(tu), rows_with_another_class=int((i1 != idx).sum().item())))
    for r in readers.values():
        r.close()


if __name__ == "__main__":
    main()
