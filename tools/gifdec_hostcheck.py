"""Build tools/gifdec_hostcheck.cpp -- what the device GIF decoder runs (csrc/gif_lzw.h: the piece scan, the lengths pass, the offsets, the
decode of every piece) under its serial host drivers, and the walk of bbocr_host_gif_plan (csrc/gif_parse.h), as a stand-alone host
program -- with -fsanitize=address,undefined and run it ONCE over the files of tests/gif_decode_ref.py: Pillow's matrix, the hand-built
files, the hand-written code streams, the damage list and the files the plan refuses.  The run must end clean; every sound file must give
the restatement's piece table and index stream with status 0, every damaged one the restatement's status bits, every refused one the
restatement's reason.  The files of tests/bmp_decode_ref.py go through the walk of bbocr_host_bmp_plan (csrc/bmp_parse.h) in the same run:
every reason must be the restatement's, and every byte the BMP kernel would read is read from an exact-size copy of the file.  No GPU;
nothing is loaded into python.

    python tools/gifdec_hostcheck.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++")
    args = ap.parse_args()
    import numpy as np

    import bmp_decode_ref as B
    import gif_decode_ref as R

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gifdec_hostcheck")
        subprocess.run([args.cxx, "-std=c++20", "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "gifdec_hostcheck.cpp"), "-o", exe], check=True)
        good = R.matrix() + R.handbuilt() + R.handwritten_files()
        bad = R.damaged()
        refused = [(n, f) for n, f, _ in R.refusals()]
        files = good + bad + refused
        paths = []
        for i, (_, f) in enumerate(files):
            paths.append(os.path.join(d, "f%04d.gif" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        bmps = B.matrix() + B.handbuilt() + [(n, f) for n, f, _ in B.refusals()]
        bmp_paths = []
        for i, (_, f) in enumerate(bmps):
            bmp_paths.append(os.path.join(d, "b%04d.bmp" % i))
            with open(bmp_paths[-1], "wb") as fh:
                fh.write(f)
        r = subprocess.run([exe] + paths + bmp_paths, capture_output=True, text=True)
        failures = 0
        if r.returncode != 0 or "Sanitizer" in r.stderr or "runtime error" in r.stderr:
            failures += 1
            print(r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(paths) + len(bmp_paths) or failures, (len(lines), len(paths), len(bmp_paths))
        lines, bmp_lines = lines[:len(paths)], lines[len(paths):]
        for (name, f), line in zip(bmps, bmp_lines):
            pl = B.plan(f)
            want = 0
            if pl["supported"]:
                want = (sum(f[pl["table_offset"]:pl["table_offset"] + pl["table_entry"] * pl["colors"]])
                        + sum(f[pl["data_offset"]:pl["data_offset"] + pl["row_stride"] * pl["height"]])) & 0xFFFFFFFF
            if int(line.split()[-7]) != pl["reason"] or int(line.split()[-1]) != want:
                failures += 1
                print("MISMATCH", name, line)
        flagged = 0
        for i, line in enumerate(lines):
            name, f = files[i]
            words = line.split()
            reason, status, pieces, total = int(words[-7]), int(words[-5]), int(words[-3]), int(words[-1])
            pl = R.plan(f)
            ok = reason == pl["reason"]
            if ok and pl["supported"]:
                want = R.decode(f)
                st = want["stages"]
                table = np.fromfile(paths[i] + ".pieces", np.uint32).reshape(-1, 4)
                flagged += status != 0
                ok = (status == want["status"] and pieces == len(st["pieces"]) and total == st["total"]
                      and [(int(a) | (int(b) << 32), int(c), int(e)) for a, b, c, e in table] == st["pieces"] and (status != 0) == (i >= len(good)))
                if ok and status == 0:
                    ok = open(paths[i] + ".raw", "rb").read() == want["stage2"]
            elif ok:
                ok = i >= len(good) + len(bad)
            if not ok:
                failures += 1
                print("MISMATCH", name, line)
        print(f"{len(good)} files decoded and compared, {len(bad)} damaged files ({flagged} of them ended in a status), {len(refused)} refused "
              f"files, {len(bmps)} BMP files planned and read, {failures} failures")
        return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
