"""Baseline JPEG decoding on the device (csrc/jpegdec.hip) against the host's libjpeg-turbo (Pillow), on one box.

    python tools/jpeg_decode_bench.py [--reps 10] [--extract 1024] [--photos 16] [--out profiles/bench_jpeg_decode.jsonl] [--device-only]
                                      [--label NAME] [--progressive-only]

Prints JSON lines and appends them to --out; `--label` names the build in every line (A/B runs of two libraries on one machine:
BBOCR_LIB_PATH selects the library):
  * plan        bbocr_host_jpeg_plan per file (the only host work per file: one pass over the markers and the scan's FF bytes);
  * decode64    one bbocr_jpeg_decode call for a 64-page batch of 1280x960 quality-90 synthetic pages, ms per page, against
                decode_file_ycc of the same files on one core;
  * photo       one 5712x4284 photograph, the same two ways;
  * decode64_444 / decode64_422 / decode64_440   the 64-page batch saved 4:4:4 and 4:2:2, and 64 copies of one page's lossless transposition
                (4:4:0, built by tests/jpeg_chroma_ref.make_440: Pillow writes no such file) -- the files ``device_decode="chroma"`` adds --
                one bbocr_jpeg_decode call against what they cost without it: decode_file_ycc on one core plus the upload of the triples;
  * decode64_prog420 / decode64_prog444 / decode1_prog / photo_prog   the files ``device_decode="progressive"`` adds: the 64-page batch saved
                progressive as 4:2:0 and as 4:4:4, one such page alone, and tests/golden/photos/IMG_9684.JPG saved progressive -- one
                bbocr_jpeg_decode_progressive call against Pillow's decode on one core plus the upload of the triples, the two alternated
                in one process (best of --reps each); --progressive-only runs these rows alone;
  * extract     extract_texts over --extract pages (extractor_bench.py's page set) with device_decode off / on, alternating, each twice;
  * photos      extract_texts(device_thumbnail=True) over --photos 5712x4284 pages with device_decode off / on.
--device-only: the decode64 and photo device legs alone (for a separate `rocprofv3 --kernel-trace --stats` run).
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--extract", type=int, default=1024)
    ap.add_argument("--photos", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_jpeg_decode.jsonl"))
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--label", default="in-tree")
    ap.add_argument("--progressive-only", action="store_true")
    a = ap.parse_args()
    import torch
    from PIL import Image

    import bb_ocr_amd
    from bb_ocr_amd import extractor_batch, synth, weights
    from bb_ocr_amd.reader import decode_file_ycc, jpeg_page, jpeg_plan

    rows = []

    def emit(**row):
        row["build"] = a.label
        print(json.dumps(row), flush=True)
        rows.append(row)

    def jpeg(img, **kw):
        buf = io.BytesIO()
        img.save(buf, "JPEG", **kw)
        return buf.getvalue()

    reader = bb_ocr_amd.Reader(["en"], gpu=True, weights=(weights.designed_craft_state(0), weights.synthetic_crnn_state(0)))
    pages = [jpeg(Image.fromarray(synth.page(1234 + i)[0]), quality=90) for i in range(64)]
    photo = jpeg(Image.fromarray(synth.page(900, width=1280, height=960, lines=20)[0]).resize((5712, 4284), Image.BICUBIC), quality=92)

    def device_ms(datas):
        batch = [jpeg_page(d, chroma=True) for d in datas]
        _, status = reader.decode_jpeg_batch(batch, padded=True)                 # warm-up: buffers grow here
        assert not any(status)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            reader.decode_jpeg_batch(batch, padded=True)
        return (time.perf_counter() - t) * 1e3 / a.reps

    def host_ms(datas):
        t = time.perf_counter()
        for d in datas:
            assert decode_file_ycc(d, padded=True) is not None
        return (time.perf_counter() - t) * 1e3

    def host_upload_ms(datas):
        torch.cuda.synchronize()
        t = time.perf_counter()
        reader._to_dev([decode_file_ycc(d, padded=True) for d in datas])
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def progressive_rows():
        imgs = [Image.fromarray(synth.page(1234 + i)[0]) for i in range(64)]
        golden = Image.open(os.path.join(ROOT, "tests", "golden", "photos", "IMG_9684.JPG"))
        p420 = [jpeg(im, quality=90, progressive=True) for im in imgs]
        legs = (("decode64_prog420", p420), ("decode64_prog444", [jpeg(im, quality=90, progressive=True, subsampling=0) for im in imgs]),
                ("decode1_prog", p420[:1]), ("photo_prog", [jpeg(golden, quality=90, progressive=True)]))
        for name, datas in legs:
            batch = [jpeg_page(d, chroma=True, progressive=True) for d in datas]
            assert all(p is not None and p.progressive for p in batch)
            _, status = reader.decode_jpeg_batch(batch, padded=True)             # warm-up: buffers grow here
            assert not any(status)
            dev, host = [], []
            for _ in range(a.reps):                                              # alternated: both see the same machine
                torch.cuda.synchronize()
                t = time.perf_counter()
                reader.decode_jpeg_batch(batch, padded=True)
                dev.append((time.perf_counter() - t) * 1e3)
                host.append(host_upload_ms(datas))
            emit(leg=name, files=len(datas), kbytes_per_file=round(sum(map(len, datas)) / len(datas) / 1024, 1), reps=a.reps,
                 size="%dx%d" % (batch[0].shape[1], batch[0].shape[0]), device_ms_per_page=round(min(dev) / len(datas), 3),
                 device_ms_per_page_mean=round(sum(dev) / len(dev) / len(datas), 3),
                 host_decode_upload_ms_per_page=round(min(host) / len(datas), 3),
                 host_decode_upload_ms_per_page_mean=round(sum(host) / len(host) / len(datas), 3))

    def write_rows():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")

    if a.progressive_only:
        progressive_rows()
        write_rows()
        return
    for name, datas in (("decode64", pages), ("photo", [photo])):
        row = dict(leg=name, files=len(datas), kbytes_per_file=round(sum(map(len, datas)) / len(datas) / 1024, 1),
                   device_ms_per_page=round(device_ms(datas) / len(datas), 3))
        if not a.device_only:
            row["host_one_core_ms_per_page"] = round(min(host_ms(datas) for _ in range(3)) / len(datas), 3)
            t = time.perf_counter()
            for d in datas:
                jpeg_plan(d)
            row["plan_ms_per_file"] = round((time.perf_counter() - t) * 1e3 / len(datas), 4)
        emit(**row)
    if not a.device_only:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from jpeg_chroma_ref import make_440

        imgs = [Image.fromarray(synth.page(1234 + i)[0]) for i in range(64)]
        classes = (("decode64_444", [jpeg(im, quality=90, subsampling=0) for im in imgs]),
                   ("decode64_422", [jpeg(im, quality=90, subsampling=1) for im in imgs]),
                   ("decode64_440", [make_440(jpeg(imgs[0].transpose(Image.TRANSPOSE), quality=90, subsampling=1))] * 64))
        for name, datas in classes:
            assert all(jpeg_plan(d).chroma and not jpeg_plan(d).supported for d in datas)
            emit(leg=name, files=len(datas), kbytes_per_file=round(sum(map(len, datas)) / len(datas) / 1024, 1),
                 device_ms_per_page=round(device_ms(datas) / len(datas), 3),
                 host_decode_upload_ms_per_page=round(min(host_upload_ms(datas) for _ in range(3)) / len(datas), 3))
        progressive_rows()
        with tempfile.TemporaryDirectory() as d:
            if a.extract > 0:
                uniq = [Image.fromarray(synth.page(1234 + i)[0]) for i in range(8)]
                paths = []
                for i in range(a.extract):
                    paths.append(os.path.join(d, f"page_{i:04d}.jpg"))
                    uniq[i % 8].save(paths[-1], quality=92)
                for dev in (False, True):
                    extractor_batch.extract_texts(reader, paths[:64], device_decode=dev)   # warm-up
                bb_ocr_amd.freeze_gc()
                ref = None
                for dev in (False, True, False, True):
                    t = time.perf_counter()
                    texts = extractor_batch.extract_texts(reader, paths, device_decode=dev)
                    dt = time.perf_counter() - t
                    ref = ref or texts
                    emit(leg="extract", device_decode=dev, pages=len(paths), seconds=round(dt, 3), pages_per_s=round(len(paths) / dt, 1),
                         texts_equal_first_run=texts == ref)
            if a.photos > 0:
                paths = []
                for k in range(a.photos):
                    paths.append(os.path.join(d, f"photo{k:03d}.jpg"))
                    Image.fromarray(synth.page(900 + k, width=1280, height=960, lines=20)[0]).resize((5712, 4284), Image.BICUBIC).save(paths[-1], quality=92)
                ref = None
                for dev in (False, True, False, True):
                    extractor_batch.extract_texts(reader, paths[:2], device_thumbnail=True, device_decode=dev)
                    t = time.perf_counter()
                    texts = extractor_batch.extract_texts(reader, paths, device_thumbnail=True, device_decode=dev)
                    dt = time.perf_counter() - t
                    ref = ref or texts
                    emit(leg="photos", device_thumbnail=True, device_decode=dev, pages=len(paths), seconds=round(dt, 2),
                         pages_per_s=round(len(paths) / dt, 2), texts_equal_first_run=texts == ref)
    write_rows()


if __name__ == "__main__":
    main()
