"""TIFF files decoded on the device (tiff_decode=True: Reader.decode_tiff_batch, csrc/tiffdec.hip) against the host path they replace:
Pillow's decode on one core (reader.decode_file) plus the upload -- bench_png_decode.py's yardstick and page classes.

    python tools/bench_tiff_decode.py [--pages 64] [--files 256] [--rounds 3] [--no-photo] [--out profiles/bench_tiff_decode.jsonl]

Writes JSON lines.  Every figure is a host wall time around a device synchronise; the two sides of a row are measured alternately
`--rounds` times in one process, so the host figure of a row is the yardstick of its device figure.  The files are Pillow's own: strips
of about 64 KB of pixels (libtiff's default) for PackBits, LZW and Deflate, ONE strip for uncompressed files (Pillow's raw writer).
Per codec (raw, packbits, tiff_lzw, tiff_adobe_deflate):
  * legs "decode64_<codec>_<kind>": `--pages` files of 1280x960 per call -- clean RGB (the text mask over flat paper and ink), noisy RGB
    (synth.page), the noisy page as mode L, the text mask at 1 bit -- one decode_tiff_batch call against decode_file of every file + one
    upload of the batch;
  * legs "decode1_<codec>_<kind>": one such file alone;
  * leg "photo_<codec>": one 5712x4284 RGB file;
  * legs "read_files_<codec>_noisy_rgb" / "..._clean_rgb": a directory of `--files` such files through extractor_batch.read_files with
    tiff_decode on and off, after one untimed pass of each side over the whole directory.
  * leg "lzw_one_strip": the noisy L page as ONE LZW strip -- one wavefront decodes it alone, so its time over the strip's code count is
    the LZW kernel's time per code (an upper bound: the upload and the output launch are inside it).
Every device decode is compared with the host's planes.
"""
import argparse
import io
import json
import os
import shutil
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODECS = ("raw", "packbits", "tiff_lzw", "tiff_adobe_deflate")
KINDS = ("clean_rgb", "noisy_rgb", "noisy_L", "text_1bit")


def lzw_code_count(strip):
    """the codes of one LZW strip up to its EOI: the width is a function of the entry count, so no string is needed to count them"""
    bitpos, next_free, behind_clear, count = 0, 258, True, 0
    nbits = 8 * len(strip)
    strip = bytes(strip) + b"\0\0"
    while True:
        w = 9 if next_free < 511 else (10 if next_free < 1023 else (11 if next_free < 2047 else 12))
        if bitpos + w > nbits:
            return count
        byte, shift = divmod(bitpos, 8)
        code = (int.from_bytes(strip[byte:byte + 3], "big") >> (24 - shift - w)) & ((1 << w) - 1)
        bitpos += w
        count += 1
        if code == 257:
            return count
        if code == 256:
            next_free, behind_clear = 258, True
        else:
            if not behind_clear and next_free < 4096:
                next_free += 1
            behind_clear = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-photo", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_tiff_decode.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image, TiffImagePlugin

    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, synth, weights
    from bb_ocr_amd.reader import TiffPage, decode_file, tiff_plan

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def tiff(arr, codec):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, "TIFF", compression=codec)
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
        (rgb, gray), status = reader.decode_tiff_batch([TiffPage(f, tiff_plan(f)) for f in files])
        assert not any(status), status
        return rgb, gray

    def leg(name, files, **extra):
        h, d = host(files), device(files)                                # warm-up, and the comparison
        assert torch.equal(h[0], d[0]) and torch.equal(h[1], d[1]), name
        del h, d
        out = []
        for r in range(max(3, a.rounds)):
            th, _ = wall(lambda: host(files))
            td, _ = wall(lambda: device(files))
            out.append(td)
            emit(leg=name, round=r, files=len(files), file_bytes=sum(len(f) for f in files), strips=sum(tiff_plan(f).strips for f in files),
                 host_ms_per_file=round(th / len(files), 3), device_ms_per_file=round(td / len(files), 3),
                 timing="host wall clock around a device synchronise", **extra)
        return min(out)

    def arrays(k):
        # synth.page IS the noisy page: N(0,4) on the paper, +-10 on the ink, chroma noise on red and blue.  The clean page is its text
        # mask over flat paper and flat ink (a pre-processed scan): no noise at all.
        noisy = synth.page(500 + k, width=1280, height=960, lines=20, colour=True)[0]
        ink = noisy[..., 1] < 128
        clean = np.where(ink[..., None], np.array([30, 30, 40], np.uint8), np.array([235, 233, 228], np.uint8)).astype(np.uint8)
        return {"clean_rgb": clean, "noisy_rgb": noisy, "noisy_L": np.ascontiguousarray(noisy[..., 1]), "text_1bit": ~ink}

    pages = [arrays(k) for k in range(a.pages)]
    photo = None
    if not a.no_photo:
        photo = np.asarray(Image.fromarray(synth.page(700, width=1280, height=960, lines=20, colour=True)[0]).resize((5712, 4284), Image.BICUBIC))
    d = tempfile.mkdtemp(prefix="bench_tiff_decode_")
    try:
        for codec in CODECS:
            files = {kind: [tiff(p[kind], codec) for p in pages] for kind in KINDS}
            for kind in KINDS:
                leg("decode64_%s_%s" % (codec, kind), files[kind], size=[1280, 960])
            for kind in KINDS:
                leg("decode1_%s_%s" % (codec, kind), files[kind][:1], size=[1280, 960])
            if photo is not None:
                leg("photo_" + codec, [tiff(photo, codec)], size=[5712, 4284])
            for kind in ("noisy_rgb", "clean_rgb"):
                paths = []
                for k in range(a.files):
                    paths.append(os.path.join(d, "%s_%s%04d.tiff" % (codec, kind, k)))
                    with open(paths[-1], "wb") as f:
                        f.write(files[kind][k % len(pages)])
                off = extractor_batch.read_files(reader, paths, tiff_decode=False)      # untimed: both sides once over the whole directory
                assert repr(extractor_batch.read_files(reader, paths, tiff_decode=True)) == repr(off)
                for r in range(max(3, a.rounds)):
                    t_off, _ = wall(lambda: extractor_batch.read_files(reader, paths, tiff_decode=False))
                    t_on, _ = wall(lambda: extractor_batch.read_files(reader, paths, tiff_decode=True))
                    emit(leg="read_files_%s_%s" % (codec, kind), round=r, files=len(paths), host_pages_per_s=round(len(paths) / t_off * 1e3, 1),
                         device_pages_per_s=round(len(paths) / t_on * 1e3, 1),
                         timing="host wall clock around a device synchronise; one untimed pass first")
                for p in paths:
                    os.remove(p)
        old = TiffImagePlugin.STRIP_SIZE
        TiffImagePlugin.STRIP_SIZE = 1 << 30
        try:
            one = tiff(pages[0]["noisy_L"], "tiff_lzw")
        finally:
            TiffImagePlugin.STRIP_SIZE = old
        plan = tiff_plan(one)
        assert plan.strips == 1
        off0 = struct.unpack_from("<I", one, 4)[0]                       # the one strip's place: the inline LONGs of tags 273 and 279
        tags = {struct.unpack_from("<H", one, off0 + 2 + 12 * e)[0]: struct.unpack_from("<I", one, off0 + 2 + 12 * e + 8)[0]
                for e in range(struct.unpack_from("<H", one, off0)[0])}
        codes = lzw_code_count(one[tags[273]:tags[273] + tags[279]])
        best = leg("lzw_one_strip", [one], size=[1280, 960], codes=codes)
        emit(leg="lzw_ns_per_code", codes=codes, device_ms=round(best, 3), ns_per_code=round(best * 1e6 / codes, 1),
             note="one wavefront, one strip; upload and output launch included")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
