"""GIF and BMP files decoded on the device (gif_decode=True / bmp_decode=True: Reader.decode_gif_pages, csrc/gifdec.hip;
Reader.decode_bmp_pages, csrc/bmpdec.hip) against the host path they replace: Pillow's decode on one core (reader.decode_file) plus the
upload -- bench_tiff_decode.py's yardstick and page classes.

    python tools/bench_gif_bmp_decode.py [--pages 64] [--files 256] [--rounds 3] [--out profiles/bench_gif_bmp_decode.jsonl]

Writes JSON lines.  Every figure is a host wall time around a device synchronise; the two sides of a row are measured alternately
`--rounds` times in one process, so the host figure of a row is the yardstick of its device figure.  The files are Pillow's own.
  * legs "decode64_gif_<kind>": `--pages` files of 1280x960 per call -- the clean text page (mode P), the noisy page as mode L, the text
    mask at 1 bit -- one decode_gif_pages call against decode_file of every file + the upload of every page; "decode64_bmp_<kind>": clean
    and noisy RGB, noisy L, the 1-bit text mask;
  * legs "decode1_<format>_<kind>": one such file alone;
  * legs "read_files_<format>_<kind>": a directory of `--files` such files through extractor_batch.read_files with the option on and off,
    after one untimed pass of each side over the whole directory;
  * legs "gif_launches_<kind>": the five launches' times of one 64-file call and of one file alone (bbocr_gif_decode_timed: events on the
    stream), with the files' code and piece counts -- whether the scan or the slowest piece bounds a page -- and "gif_ns_per_code": the
    lengths and the decode launch of ONE noisy file over the codes of its LONGEST piece (each piece is one wavefront's serial walk, all
    pieces run side by side: the launch lasts as long as the longest piece).
Every device decode is compared with the host's planes.
"""
import argparse
import ctypes as C
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def pieces_of(payload, m):
    """[(data codes, how it ends)] of a payload, by one serial walk with incremental widths (tests/gif_decode_ref.py's scan is the rule)"""
    clear, nbits = 1 << m, 8 * len(payload)
    out, bit, k, width, nxt = [], 0, 0, m + 1, (1 << m) + 2
    while True:
        if bit + width > nbits:
            out.append((k, 2))
            return out
        code = (int.from_bytes(payload[bit >> 3:(bit >> 3) + 3], "little") >> (bit & 7)) & ((1 << width) - 1)
        bit += width
        if code == clear or code == clear + 1:
            out.append((k, 0 if code == clear else 1))
            if code != clear:
                return out
            k, width, nxt = 0, m + 1, clear + 2
            continue
        if k and nxt < 4096:
            nxt += 1
            if nxt == 1 << width and width < 12:
                width += 1
        k += 1


KINDS = {"gif": ("clean_P", "noisy_L", "text_1bit"), "bmp": ("clean_rgb", "noisy_rgb", "noisy_L", "text_1bit")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gif_bmp_decode.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    import bb_ocr_amd
    import gif_decode_ref as R
    from bb_ocr_amd import extractor_batch, synth, weights
    from bb_ocr_amd.reader import BmpPage, GifPage, bmp_plan, decode_file, gif_plan

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def written(arr, fmt):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, fmt.upper())
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

    def device(files, fmt):
        if fmt == "gif":
            planes, status = reader.decode_gif_pages([GifPage(f, gif_plan(f)) for f in files])
        else:
            planes, status = reader.decode_bmp_pages([BmpPage(f, bmp_plan(f)) for f in files])
        assert not any(status), status
        return planes

    def leg(name, files, fmt, **extra):
        h, d = host(files), device(files, fmt)                           # warm-up, and the comparison
        assert all(torch.equal(h[0][k], d[k][0]) and torch.equal(h[1][k], d[k][1]) for k in range(len(files))), name
        del h, d
        for r in range(max(3, a.rounds)):
            th, _ = wall(lambda: host(files))
            td, _ = wall(lambda: device(files, fmt))
            emit(leg=name, round=r, files=len(files), file_bytes=sum(len(f) for f in files), host_ms_per_file=round(th / len(files), 3),
                 device_ms_per_file=round(td / len(files), 3), timing="host wall clock around a device synchronise", **extra)

    def launches(name, files, pieces):
        pages = [GifPage(f, gif_plan(f)) for f in files]
        out = [(torch.empty(p.shape, dtype=torch.uint8, device=reader.device), torch.empty(p.shape[:2], dtype=torch.uint8, device=reader.device)) for p in pages]
        n = len(pages)
        fs, sizes = reader._jpeg_files(pages)
        status, ms = (C.c_int * n)(), (C.c_float * 5)()
        best = None
        for r in range(max(3, a.rounds) + 1):                            # (the first round is the warm-up)
            torch.cuda.synchronize()
            rc = reader._lib.bbocr_gif_decode_timed(reader._h, fs, sizes, n, (C.c_void_p * n)(*[x.data_ptr() for x, _ in out]),
                                                    (C.c_longlong * n)(*[3 * p.shape[1] for p in pages]), (C.c_void_p * n)(*[g.data_ptr() for _, g in out]),
                                                    (C.c_longlong * n)(*[p.shape[1] for p in pages]), status, ms)
            assert rc == 0 and not any(status)
            if r:
                emit(leg=name, round=r - 1, files=n, scan_ms=round(ms[0], 4), lengths_ms=round(ms[1], 4), offsets_ms=round(ms[2], 4), decode_ms=round(ms[3], 4),
                     output_ms=round(ms[4], 4), codes_first_file=sum(c for c, _ in pieces) + len(pieces), pieces_first_file=len(pieces),
                     longest_piece_codes_first_file=max(c for c, _ in pieces), timing="events on the decode stream around each launch")
                best = list(ms) if best is None else [min(x, y) for x, y in zip(best, ms)]
        return best

    def arrays(k):
        # synth.page IS the noisy page: N(0,4) on the paper, +-10 on the ink, chroma noise on red and blue.  The clean page is its text
        # mask over flat paper and flat ink (a pre-processed scan): no noise at all.
        noisy = synth.page(500 + k, width=1280, height=960, lines=20, colour=True)[0]
        ink = noisy[..., 1] < 128
        clean = np.where(ink[..., None], np.array([30, 30, 40], np.uint8), np.array([235, 233, 228], np.uint8)).astype(np.uint8)
        return {"clean_rgb": clean, "clean_P": clean, "noisy_rgb": noisy, "noisy_L": np.ascontiguousarray(noisy[..., 1]), "text_1bit": ~ink}

    pages = [arrays(k) for k in range(a.pages)]
    d = tempfile.mkdtemp(prefix="bench_gif_bmp_decode_")
    try:
        for fmt in ("gif", "bmp"):
            files = {kind: [written(p[kind], fmt) for p in pages] for kind in KINDS[fmt]}
            for kind in KINDS[fmt]:
                leg("decode64_%s_%s" % (fmt, kind), files[kind], fmt, size=[1280, 960])
            for kind in KINDS[fmt]:
                leg("decode1_%s_%s" % (fmt, kind), files[kind][:1], fmt, size=[1280, 960])
            if fmt == "gif":
                for kind in KINDS[fmt]:
                    pl = R.plan(files[kind][0])
                    pieces = pieces_of(pl["payload"], pl["min_code"])
                    launches("gif_launches64_" + kind, files[kind], pieces)
                    best = launches("gif_launches1_" + kind, files[kind][:1], pieces)
                    if kind == "noisy_L":
                        longest = max(c for c, _ in pieces)
                        emit(leg="gif_ns_per_code", longest_piece_codes=longest, pieces=len(pieces), lengths_ns_per_code=round(best[1] * 1e6 / longest, 1),
                             decode_ns_per_code=round(best[3] * 1e6 / longest, 1), scan_ns_per_code=round(best[0] * 1e6 / (sum(c for c, _ in pieces) + len(pieces)), 2),
                             note="one file: the lengths and the decode launch last as long as their longest piece's serial walk; the scan walks every code, 64 per step")
            for kind in (("noisy_L", "clean_P") if fmt == "gif" else ("noisy_rgb", "clean_rgb")):
                paths = []
                for k in range(a.files):
                    paths.append(os.path.join(d, "%s_%s%04d.%s" % (fmt, kind, k, fmt)))
                    with open(paths[-1], "wb") as f:
                        f.write(files[kind][k % len(pages)])
                on, off = {fmt + "_decode": True}, {fmt + "_decode": False}
                ref = extractor_batch.read_files(reader, paths, **off)      # untimed: both sides once over the whole directory
                assert repr(extractor_batch.read_files(reader, paths, **on)) == repr(ref)
                for r in range(max(3, a.rounds)):
                    t_off, _ = wall(lambda: extractor_batch.read_files(reader, paths, **off))
                    t_on, _ = wall(lambda: extractor_batch.read_files(reader, paths, **on))
                    emit(leg="read_files_%s_%s" % (fmt, kind), round=r, files=len(paths), host_pages_per_s=round(len(paths) / t_off * 1e3, 1),
                         device_pages_per_s=round(len(paths) / t_on * 1e3, 1),
                         timing="host wall clock around a device synchronise; one untimed pass first")
                for p in paths:
                    os.remove(p)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
