"""Build tools/jpegprog_hostcheck.cpp -- the progressive scan decoder the device runs (csrc/jpegprog.h) and its host side (csrc/jpeg_parse.h),
as a stand-alone host program -- with -fsanitize=address,undefined and run it over the files of tests/test_jpeg_progressive_cpu.py: the
matrix, the written scripts, the end-of-band file, and copies with damaged bytes inside a scan of each kind (DC first, AC first, DC
refinement, AC refinement).  Every run must end clean; the coefficients of every undamaged file must equal the restatement's
(tests/jpeg_progressive_ref.py).  No GPU; nothing is loaded into python.

    python tools/jpegprog_hostcheck.py [--cxx /opt/rocm/llvm/bin/clang++] [--sizes 3]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def kind_of(scan):
    return ("dc" if scan["ss"] == 0 else "ac") + ("_first" if scan["ah"] == 0 else "_refine")


def damaged(data, plan):
    """{scan kind: a copy with up to 64 bytes inside the first scan of that kind overwritten} (no byte becomes FF: the markers stay)"""
    out = {}
    for s in plan["scans"]:
        k = kind_of(s)
        if k in out or s["bytes"] < 2:
            continue
        a = s["offset"] + s["bytes"] // 3
        n = min(64, s["offset"] + s["bytes"] - a)
        bad = bytearray(data)
        bad[a:a + n] = bytes((i * 37 + 11 + data[a + i]) & 0x7F for i in range(n))
        out[k] = bytes(bad)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++")
    ap.add_argument("--rocm", default="/opt/rocm")
    ap.add_argument("--sizes", type=int, default=5, help="how many of the matrix's sizes to run")
    args = ap.parse_args()
    import jpeg_progressive_ref as P
    import test_jpeg_progressive_cpu as T

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jpegprog_hostcheck")
        subprocess.run([args.cxx, "-std=c++20", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(args.rocm, "include"), "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "jpegprog_hostcheck.cpp"),
                        "-o", exe], check=True)
        good = [(n, f) for size in T.SIZES[:args.sizes] for n, _, f in T.matrix(size)]
        good += [(n, T.written(n)) for n in T.WRITTEN] + [("flat_eob", T.flat_eob_file())]
        bad = []
        for n, f in good[::7] + good[-5:]:
            bad += [(n + "-damaged-" + k, b) for k, b in damaged(f, P.parse(f)).items()]
        kinds = {n.rsplit("-", 1)[1] for n, _ in bad}
        assert kinds == {"dc_first", "ac_first", "dc_refine", "ac_refine"}, kinds
        paths = []
        for i, (n, f) in enumerate(good + bad):
            paths.append(os.path.join(d, "f%04d.jpg" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        failures = 0
        lines = []
        for k in range(0, len(paths), 200):
            r = subprocess.run([exe] + paths[k:k + 200], capture_output=True, text=True)
            lines += r.stdout.splitlines()
            if r.returncode != 0 or "Sanitizer" in r.stderr or "runtime error" in r.stderr:
                failures += 1
                print(r.stderr[-4000:])
        assert len(lines) == len(paths), (len(lines), len(paths))
        flagged = 0
        for i, (n, f) in enumerate(good + bad):
            words = lines[i].split()
            if i < len(good):
                got = np.fromfile(paths[i] + ".coef", np.int16).reshape(-1, 64)
                want = P.decode_coefficients(f, P.parse(f))
                if words[-3:] != ["0", "status", "0"] or not np.array_equal(got, want):
                    failures += 1
                    print("MISMATCH", n, lines[i])
            else:                                                     # the error paths too: a status exactly where the restatement gives up
                plan = P.parse(f)
                if not plan["supported"]:                             # the damage reached a marker: both plans refuse, for one reason
                    ok = words[-2:] == ["reason", str(plan["reason"])]
                else:
                    status = words[-3:] != ["0", "status", "0"]
                    flagged += status
                    try:
                        P.decode_coefficients(f, plan)
                        raised = False
                    except ValueError:
                        raised = True
                    ok = status == raised
                if not ok:
                    failures += 1
                    print("STATUS MISMATCH", n, lines[i])
        print(f"{len(good)} files decoded and compared, {len(bad)} damaged copies ({flagged} of them ended in a status), {failures} failures")
        return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
