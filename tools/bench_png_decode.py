"""PNG files decoded on the device (png_decode=True: Reader.decode_png_batch, csrc/pngdec.hip) against the host path they replace:
Pillow's decode on one core (reader.decode_file) plus the upload.

    python tools/bench_png_decode.py [--pages 64] [--files 256] [--rounds 3] [--no-photo] [--out profiles/bench_png_decode.jsonl]

Writes JSON lines.  Every figure is a host wall time around a device synchronise; the two sides of a row are measured alternately
`--rounds` times in one process, so the host figure of a row is the yardstick of its device figure.
  * legs "decode64_<kind>": `--pages` files of 1280x960 per call -- clean RGB (the text mask over flat paper and ink, no noise), noisy RGB
    (synth.page: N(0,4) on the paper and chroma noise), the noisy page as mode L, the text mask at 1 bit -- one decode_png_batch call
    against decode_file of every file + one upload of the batch;
  * legs "decode1_<kind>": one such file alone;
  * leg "photo": one 5712x4284 RGB file;
  * legs "read_files_noisy_rgb" / "read_files_clean_rgb": a directory of `--files` such files through extractor_batch.read_files with
    png_decode on and off, after one untimed pass of each side over the whole directory.
Inflate is serial per stream and one wavefront decodes one file: the batch legs have the parallelism, the single-file legs do not.
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
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-photo", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_png_decode.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, synth, weights
    from bb_ocr_amd.reader import PngPage, decode_file, png_plan

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def png(arr):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, "PNG")
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
        (rgb, gray), status = reader.decode_png_batch([PngPage(f, png_plan(f)) for f in files])
        assert not any(status), status
        return rgb, gray

    def leg(name, files, **extra):
        h, d = host(files), device(files)                                # warm-up, and the comparison
        assert torch.equal(h[0], d[0]) and torch.equal(h[1], d[1]), name
        del h, d
        for r in range(max(3, a.rounds)):
            th, _ = wall(lambda: host(files))
            td, _ = wall(lambda: device(files))
            emit(leg=name, round=r, files=len(files), file_bytes=sum(len(f) for f in files), host_ms_per_file=round(th / len(files), 3),
                 device_ms_per_file=round(td / len(files), 3), timing="host wall clock around a device synchronise", **extra)

    def kinds(k):
        # synth.page IS the noisy page: N(0,4) on the paper, +-10 on the ink, chroma noise on red and blue.  The clean page is its text
        # mask over flat paper and flat ink (a pre-processed scan): no noise at all.
        noisy = synth.page(500 + k, width=1280, height=960, lines=20, colour=True)[0]
        ink = noisy[..., 1] < 128
        clean = np.where(ink[..., None], np.array([30, 30, 40], np.uint8), np.array([235, 233, 228], np.uint8)).astype(np.uint8)
        return {"clean_rgb": png(clean), "noisy_rgb": png(noisy), "noisy_L": png(noisy[..., 1]), "text_1bit": png(~ink)}

    pages = [kinds(k) for k in range(a.pages)]
    for kind in ("clean_rgb", "noisy_rgb", "noisy_L", "text_1bit"):
        leg("decode64_" + kind, [p[kind] for p in pages], size=[1280, 960])
    for kind in ("clean_rgb", "noisy_rgb", "noisy_L", "text_1bit"):
        leg("decode1_" + kind, [pages[0][kind]], size=[1280, 960])
    if not a.no_photo:
        photo = np.asarray(Image.fromarray(synth.page(700, width=1280, height=960, lines=20, colour=True)[0]).resize((5712, 4284), Image.BICUBIC))
        leg("photo", [png(photo)], size=[5712, 4284])

    d = tempfile.mkdtemp(prefix="bench_png_decode_")
    try:
        for kind in ("noisy_rgb", "clean_rgb"):
            paths = []
            for k in range(a.files):
                paths.append(os.path.join(d, "%s%04d.png" % (kind, k)))
                with open(paths[-1], "wb") as f:
                    f.write(pages[k % len(pages)][kind])
            off = extractor_batch.read_files(reader, paths, png_decode=False)          # untimed: both sides once over the whole directory
            assert repr(extractor_batch.read_files(reader, paths, png_decode=True)) == repr(off)
            for r in range(max(3, a.rounds)):
                t_off, _ = wall(lambda: extractor_batch.read_files(reader, paths, png_decode=False))
                t_on, _ = wall(lambda: extractor_batch.read_files(reader, paths, png_decode=True))
                emit(leg="read_files_" + kind, round=r, files=len(paths), host_pages_per_s=round(len(paths) / t_off * 1e3, 1),
                     device_pages_per_s=round(len(paths) / t_on * 1e3, 1), timing="host wall clock around a device synchronise; one untimed pass first")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
