"""Build tools/pngdec_hostcheck.cpp -- the inflate the device PNG decoder runs (csrc/png_inflate.h) under its serial host driver, and the
chunk walk of bbocr_host_png_plan (csrc/png_parse.h), as a stand-alone host program -- with -fsanitize=address,undefined and run it ONCE
over the files of tests/png_decode_ref.py: the matrix, the hand-written deflate streams, the damage list and the files the plan refuses.
The run must end clean; every undamaged file must inflate to the restatement's bytes with status 0, every damaged one must end in a status
(or, where the stream is sound and the scanlines are not, in the bytes zlib gives), every refused one in the restatement's reason.  No
GPU; nothing is loaded into python.

    python tools/pngdec_hostcheck.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++")
    args = ap.parse_args()
    import png_decode_ref as R
    import test_png_decode_cpu as T

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pngdec_hostcheck")
        subprocess.run([args.cxx, "-std=c++20", "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "pngdec_hostcheck.cpp"), "-o", exe], check=True)
        good = list(R.matrix()) + [(n, R.wrap_stream(z, len(data))) for n, z, data in R.handwritten()]
        bad = [(n, R.wrap_stream(z, length, 3)) for n, z, length in R.damaged()]
        refused = [(n, f) for n, f, _ in T.refusals()]
        files = good + bad + refused
        paths = []
        for i, (_, f) in enumerate(files):
            paths.append(os.path.join(d, "f%04d.png" % i))
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
            reason, status, produced = int(words[-5]), int(words[-3]), int(words[-1])
            pl, idat, _ = R.walk(f)
            ok = reason == pl["reason"]
            if ok and pl["supported"]:
                got = open(paths[i] + ".raw", "rb").read()
                want_len = pl["height"] * (1 + pl["row_bytes"])
                try:
                    o = zlib.decompressobj()
                    want = o.decompress(b"".join(idat))
                    sound = o.eof and len(want) == want_len
                except zlib.error:
                    want, sound = None, False
                if i < len(good):
                    ok = sound and status == 0 and got == want
                else:
                    flagged += status != 0
                    ok = (status != 0) == (not sound) and (not sound or got == want) and len(got) == produced <= want_len
            if not ok:
                failures += 1
                print("MISMATCH", name, line)
        print(f"{len(good)} files inflated and compared, {len(bad)} damaged files ({flagged} of them ended in a status), {len(refused)} refused files, "
              f"{failures} failures")
        return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
