"""CCITT TIFF files decoded on the device (tiff_decode="fax": bbocr_tiff_decode_fax, csrc/tiff_fax.h) against the host path they replace:
Pillow's decode (libtiff) on one core (reader.decode_file) plus the upload -- bench_tiff_decode.py's yardstick.

    python tools/bench_tiff_fax.py [--pages 64] [--files 256] [--rounds 3] [--no-a4] [--out profiles/bench_tiff_fax.jsonl]

Writes JSON lines.  Every figure is a host wall time around a device synchronise; the two sides of a row are measured alternately
`--rounds` times in one process, so the host figure of a row is the yardstick of its device figure.  The pages are 1-bit text pages
(synth.page's ink mask) of 1280x960 and of 2480x3504 (A4 at 300 dpi), each written by Pillow as Group 4 in its own strips ("g4"), as
Group 4 in ONE strip ("g4_one_strip") and as Group 3 2-D in its own strips ("g3_2d").
  * legs "decode64_<class>_<size>": `--pages` files per call -- one decode_tiff_pages call against decode_file of every file + one upload of
    the batch;
  * legs "decode1_<class>_<size>": one such file alone;
  * legs "read_files_<class>_1280x960": a directory of `--files` files through extractor_batch.read_files with tiff_decode="fax" and off,
    after one untimed pass of each side over the whole directory;
  * leg "fax_ns_per_code": the 1280x960 Group 4 page in ONE strip decoded alone -- one wavefront -- over the strip's code count (mode
    codes and run code words, counted by tests/tiff_fax_ref.py's decoder): the strip kernel's time per code (an upper bound: the upload
    and the output launch are inside it).
Every device decode is compared with the host's planes.
"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CLASSES = ("g4", "g4_one_strip", "g3_2d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-a4", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_tiff_fax.jsonl"))
    a = ap.parse_args()
    import torch
    from PIL import Image, TiffImagePlugin

    import bb_ocr_amd
    import tiff_fax_ref as F
    from bb_ocr_amd import extractor_batch, synth, weights
    from bb_ocr_amd.reader import decode_file, tiff_page

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def tiff(mask, cls):
        old = TiffImagePlugin.STRIP_SIZE
        if cls == "g4_one_strip":
            TiffImagePlugin.STRIP_SIZE = 1 << 30
        try:
            b = io.BytesIO()
            Image.fromarray(mask).save(b, "TIFF", compression="group3" if cls == "g3_2d" else "group4", tiffinfo={292: 1} if cls == "g3_2d" else {})
        finally:
            TiffImagePlugin.STRIP_SIZE = old
        return b.getvalue()

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def host(files):
        planes = [decode_file(f) for f in files]
        return reader._to_dev([p[0] for p in planes]), reader._to_dev([p[1] for p in planes])

    def device(files):
        planes, status = reader.decode_tiff_pages([tiff_page(f, fax=True) for f in files])
        assert not any(status), status
        return torch.stack([p[0] for p in planes]), torch.stack([p[1] for p in planes])

    def leg(name, files, **extra):
        h, d = host(files), device(files)                                # warm-up, and the comparison
        assert torch.equal(h[0], d[0]) and torch.equal(h[1], d[1]), name
        del h, d
        out = []
        for r in range(max(3, a.rounds)):
            th, _ = wall(lambda: host(files))
            td, _ = wall(lambda: device(files))
            out.append(td)
            emit(leg=name, round=r, files=len(files), file_bytes=sum(len(f) for f in files), strips=F.fax_plan(files[0])[0]["strips"] * len(files),
                 host_ms_per_file=round(th / len(files), 3), device_ms_per_file=round(td / len(files), 3),
                 timing="host wall clock around a device synchronise", **extra)
        return min(out)

    def mask(k, width, height, lines):
        return ~(synth.page(500 + k, width=width, height=height, lines=lines, colour=True)[0][..., 1] < 128)

    sizes = [("1280x960", 1280, 960, 20, a.pages)] + ([] if a.no_a4 else [("2480x3504", 2480, 3504, 70, 8)])
    d = tempfile.mkdtemp(prefix="bench_tiff_fax_")
    try:
        for tag, width, height, lines, distinct in sizes:
            masks = [mask(k, width, height, lines) for k in range(distinct)]
            for cls in CLASSES:
                files = [tiff(masks[k % distinct], cls) for k in range(a.pages)]
                leg("decode64_%s_%s" % (cls, tag), files, size=[width, height])
                leg("decode1_%s_%s" % (cls, tag), files[:1], size=[width, height])
                if tag != "1280x960":
                    continue
                paths = []
                for k in range(a.files):
                    paths.append(os.path.join(d, "%s%04d.tiff" % (cls, k)))
                    with open(paths[-1], "wb") as f:
                        f.write(files[k % len(files)])
                off = extractor_batch.read_files(reader, paths, tiff_decode=False)      # untimed: both sides once over the whole directory
                assert repr(extractor_batch.read_files(reader, paths, tiff_decode="fax")) == repr(off)
                for r in range(max(3, a.rounds)):
                    t_off, _ = wall(lambda: extractor_batch.read_files(reader, paths, tiff_decode=False))
                    t_on, _ = wall(lambda: extractor_batch.read_files(reader, paths, tiff_decode="fax"))
                    emit(leg="read_files_%s_%s" % (cls, tag), round=r, files=len(paths), host_pages_per_s=round(len(paths) / t_off * 1e3, 1),
                         device_pages_per_s=round(len(paths) / t_on * 1e3, 1),
                         timing="host wall clock around a device synchronise; one untimed pass first")
                for p in paths:
                    os.remove(p)
                if cls == "g4_one_strip":
                    pl, fax, strips = F.fax_walk(files[0])
                    assert pl["strips"] == 1
                    codes = []
                    F.decode_strip(files[0][strips[0][0]:sum(strips[0])], width, height, 4, codes=codes)
                    best = leg("fax_one_strip", files[:1], size=[width, height], codes=len(codes))
                    emit(leg="fax_ns_per_code", codes=len(codes), device_ms=round(best, 3), ns_per_code=round(best * 1e6 / len(codes), 1),
                         note="one wavefront, one strip; upload and output launch included")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
