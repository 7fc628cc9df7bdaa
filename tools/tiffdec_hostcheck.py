"""Build tools/tiffdec_hostcheck.cpp -- the strip decoders the device TIFF decoder runs (csrc/tiff_codecs.h, csrc/png_inflate.h) under their
serial host drivers, and the IFD walk of bbocr_host_tiff_plan (csrc/tiff_parse.h), as a stand-alone host program -- with
-fsanitize=address,undefined and run it ONCE over the files of tests/tiff_decode_ref.py: Pillow's matrix, the hand-built files, the
hand-written code streams, the damage list and the files the plan refuses.  The run must end clean; every sound file must decode to the
restatement's stream with status 0, every damaged one must end in a status with its sound strips exact, every refused one in the
restatement's reason.  No GPU; nothing is loaded into python.

    python tools/tiffdec_hostcheck.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sound_strips(R, f):
    """-> (the stream with the damaged strips left zero, whether any strip is damaged)"""
    pl, strips, _ = R.walk(f)
    rb, rows, H = pl["row_bytes"], pl["rows_per_strip"], pl["height"]
    out, bad = bytearray(), False
    for s, (o, c) in enumerate(strips):
        need = min(rows, H - s * rows) * rb
        try:
            out += R.decode_strip(pl["compression"], f[o:o + c], need)
        except R.Damaged:
            out += bytes(need)
            bad = True
    return bytes(out), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++")
    args = ap.parse_args()
    import tiff_decode_ref as R

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tiffdec_hostcheck")
        subprocess.run([args.cxx, "-std=c++20", "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "tiffdec_hostcheck.cpp"), "-o", exe], check=True)
        good = list(R.matrix()) + R.handbuilt() + R.handwritten_files()
        bad = R.damaged()
        refused = [(n, f) for n, f, _ in R.refusals()]
        files = good + bad + refused
        paths = []
        for i, (_, f) in enumerate(files):
            paths.append(os.path.join(d, "f%04d.tif" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        r = subprocess.run([exe] + paths, capture_output=True, text=True)
        failures = 0
        if r.returncode != 0 or "Sanitizer" in r.stderr or "runtime error" in r.stderr:
            failures += 1
            print(r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(paths) or failures, (len(lines), len(paths))
        flagged = 0
        for i, line in enumerate(lines):
            name, f = files[i]
            words = line.split()
            reason, status = int(words[-5]), int(words[-3])
            pl = R.plan(f)
            ok = reason == pl["reason"]
            if ok and pl["supported"]:
                got = open(paths[i] + ".raw", "rb").read()
                want, damaged = sound_strips(R, f)
                flagged += status != 0
                ok = got == want and (status != 0) == damaged and damaged == (i >= len(good))
            elif ok:
                ok = i >= len(good) + len(bad)
            if not ok:
                failures += 1
                print("MISMATCH", name, line)
        print(f"{len(good)} files decoded and compared, {len(bad)} damaged files ({flagged} of them ended in a status), {len(refused)} refused "
              f"files, {failures} failures")
        return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
