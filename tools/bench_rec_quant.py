"""What the recogniser's rec_quant mode costs and how closely it follows the CPU arithmetic it restates.

    python tools/bench_rec_quant.py [--pages 64] [--a4-pages 16] [--steps 3] [--rounds 3] [--cpu-pages 64] [--label NAME]

Timing: `readtext_device` of an `exact_rec` Reader without and with the switch, on `--pages` synthetic pages of 1280x960 and on `--a4-pages`
A4 pages (2480x3504, bench.py's two workloads, the recogniser trained on them), one call in flight.  The two readers are ALTERNATED `--rounds`
times on one card (warm-up call, then `--steps` timed calls each); per reader and workload: pages / median step and the stage times, of
which `recognizer_net` holds the sequence stage.
Distances (`--cpu-pages` of the 1280x960 pages, 0 = skip; the CPU models need ~5 s per page): the crops of those pages through
bbocr_crnn_logits of both readers against torch's dynamically quantised oracle.nets.CRNN and against the fp32 one on the CPU -- rms over all
logits, arg-max differences at the time steps the margin rule of tests/quant_cases.py calls decidable -- and the number of boxes whose text
differs between the quantised CPU model and the fp32 one: how much the mode matters on these pages.
Appends JSON lines to profiles/bench_rec_quant.jsonl and prints them.  Nothing here is a gate.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_logits(r, xs, W):
    import torch

    g = np.rint((np.stack(xs) * 0.5 + 0.5) * 255.0).astype(np.int16) + 1           # exact-mode crops: the codes 1 + grey level
    dev = torch.from_numpy(g).contiguous().cuda()
    out = torch.zeros((len(xs), W // 4 - 1, 112), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r._check(r._lib.bbocr_crnn_logits(r._h, C.c_void_p(dev.data_ptr()), len(xs), W, C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()[:, :, :97]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--a4-pages", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cpu-pages", type=int, default=64)
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rec_quant.jsonl"))
    a = ap.parse_args()
    import torch

    import bb_ocr_amd
    from bb_ocr_amd import synth, weights

    if not torch.cuda.is_available():
        raise SystemExit("bench_rec_quant needs a GPU: nothing is measured without one")
    states = (weights.designed_craft_state(0), weights.load_npz_state(os.path.join(ROOT, "tests", "golden", "crnn_synth_fp16.npz")))
    readers = {"exact_rec": bb_ocr_amd.Reader(["en"], gpu=True, weights=states, precision="exact_rec", rec_quant=False),
               "exact_rec+rec_quant": bb_ocr_amd.Reader(["en"], gpu=True, weights=states, precision="exact_rec", rec_quant=True)}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    p1 = [synth.page(1234 + i, colour=bool(i & 1))[0] for i in range(max(a.pages, a.cpu_pages))]
    workloads = {"1280x960": p1[:a.pages],
                 "a4": [synth.page(5000 + i, width=2480, height=3504, lines=110, line_pitch=31, colour=bool(i & 1))[0] for i in range(a.a4_pages)]}
    for wl, host in workloads.items():
        if not host:
            continue
        rgb = torch.from_numpy(np.stack(host)).cuda()
        ts = {k: [] for k in readers}
        stage = {k: {} for k in readers}
        outs = {}
        for _ in range(a.rounds):
            for name, r in readers.items():
                outs[name] = r.readtext_device(rgb)
                for _ in range(a.steps):
                    t = time.perf_counter()
                    r.readtext_device(rgb)
                    ts[name].append(time.perf_counter() - t)
                    for key, v in r.stage_times().items():
                        stage[name][key] = stage[name].get(key, 0.0) + v / (a.steps * a.rounds)
        base, quant = outs["exact_rec"], outs["exact_rec+rec_quant"]
        for name in readers:
            emit(dict(bench="rec_quant", label=a.label, workload=wl, mode=name, pages=len(host), boxes=sum(len(p) for p in outs[name]),
                      boxes_equal_exact_rec=[[b[0] for b in p] for p in outs[name]] == [[b[0] for b in p] for p in base],
                      texts_differing_from_exact_rec=sum(b[1] != g[1] for p, q in zip(outs[name], base) for b, g in zip(p, q)),
                      pages_per_s=round(len(host) / float(np.median(ts[name])), 1), step_s=[round(v, 4) for v in ts[name]],
                      stage_ms={k: round(v, 2) for k, v in stage[name].items()}))
        del rgb
    if a.cpu_pages > 0:
        import quant_cases as QC
        from oracle import pipeline, recog

        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        o = pipeline.OracleReader({k: torch.from_numpy(v) for k, v in states[0].items()}, {k: torch.from_numpy(v) for k, v in states[1].items()})
        qmodel = QC.quantize_dynamic(o.recognizer)
        acc = {k: dict(sq_q=0.0, sq_f=0.0, bad=0) for k in readers}
        n = steps = excluded = boxes = text_differs = 0
        for img in p1[:a.cpu_pages]:
            by_w = {}
            for W, x in QC.page_crops(o, img):
                by_w.setdefault(W, []).append(x)
            for W, xs in sorted(by_w.items()):
                want_q = np.stack([QC.logits(qmodel, x) for x in xs])
                want_f = np.stack([QC.logits(o.recognizer, x) for x in xs])
                boxes += len(xs)
                text_differs += sum(recog.predict_from_logits(q[None])[0][0] != recog.predict_from_logits(f[None])[0][0] for q, f in zip(want_q, want_f))
                decidable = QC.margins(want_q) > QC.ARGMAX_TOL
                steps += decidable.size
                excluded += int((~decidable).sum())
                n += want_q.size
                for name, r in readers.items():
                    got = device_logits(r, xs, W)
                    acc[name]["sq_q"] += float(((got - want_q) ** 2).sum())
                    acc[name]["sq_f"] += float(((got - want_f) ** 2).sum())
                    acc[name]["bad"] += int(((got.argmax(-1) != want_q.argmax(-1)) & decidable).sum())
        for name, v in acc.items():
            emit(dict(bench="rec_quant_distance", label=a.label, mode=name, pages=a.cpu_pages, boxes=boxes, time_steps=steps,
                      rms_device_vs_quantised_cpu=float(np.sqrt(v["sq_q"] / n)), rms_device_vs_fp32_cpu=float(np.sqrt(v["sq_f"] / n)),
                      argmax_tol=QC.ARGMAX_TOL, ref_max_measured_cpu=QC.REF_MAX_MEASURED, steps_below_the_margin=excluded,
                      decidable_argmax_differences_from_quantised_cpu=v["bad"],
                      boxes_whose_text_differs_between_quantised_and_fp32_cpu=text_differs))
    for r in readers.values():
        r.close()


if __name__ == "__main__":
    main()
