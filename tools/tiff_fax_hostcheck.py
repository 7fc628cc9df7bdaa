"""Build tools/tiff_fax_hostcheck.cpp -- the CCITT strip decoder the device TIFF decoder runs (csrc/tiff_fax.h) under its serial policy, and
the lenient IFD walk of bbocr_host_tiff_fax_plan (csrc/tiff_parse.h), as a stand-alone host program -- with -fsanitize=address,undefined
and run it ONCE over the files of tests/tiff_fax_ref.py: the designed pages in all their variants, the hand-built files, the hand-written
streams, Pillow's own files, the damage list and the files the fax plan refuses.  The run must end clean; every sound file must decode to
the restatement's stream with status 0, every damaged one must end in a status with its sound strips exact, every refused one in the
restatement's reasons.  No GPU; nothing is loaded into python.

    python tools/tiff_fax_hostcheck.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import io
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sound_strips(F, f):
    """-> (the stream with the damaged strips left zero, whether any strip is damaged)"""
    pl, fax, strips = F.fax_walk(f)
    rb, rows, H = pl["row_bytes"], pl["rows_per_strip"], pl["height"]
    out, bad = bytearray(), False
    for s, (o, c) in enumerate(strips):
        n = min(rows, H - s * rows)
        try:
            out += F.decode_strip(f[o:o + c], pl["width"], n, fax["scheme"], fax["t4_options"], fax["fill_order"])
        except F.Damaged:
            out += bytes(n * rb)
            bad = True
    return bytes(out), bad


def pillow_files(F):
    from PIL import Image

    page = F.text_page(200, 60, 3)
    out = []
    for comp in ("tiff_ccitt", "group3", "group4"):
        for info in ({}, {292: 1}, {292: 4}, {292: 5}, {266: 2}):
            if comp == "group3" or 292 not in info:
                b = io.BytesIO()
                Image.fromarray(page == 0).save(b, "TIFF", compression=comp, tiffinfo=info)
                out.append(("pillow-%s-%s" % (comp, info), b.getvalue()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="/opt/rocm/llvm/bin/clang++")
    args = ap.parse_args()
    import tiff_fax_ref as F

    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tiff_fax_hostcheck")
        subprocess.run([args.cxx, "-std=c++20", "-I", os.path.join(ROOT, "include"), "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "tiff_fax_hostcheck.cpp"), "-o", exe], check=True)
        good = F.designed_files() + F.handbuilt() + F.handwritten_files() + pillow_files(F)
        bad = F.damaged()
        refused = [(n, f) for n, f, _, _ in F.fax_refusals()]
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
            reason, fax_reason, scheme, status = int(words[-9]), int(words[-7]), int(words[-5]), int(words[-3])
            pl, fax = F.fax_plan(f)
            ok = (reason, fax_reason, scheme) == (pl["reason"], fax["reason"], fax["scheme"])
            if ok and pl["supported"]:
                got = open(paths[i] + ".raw", "rb").read()
                want, damaged = sound_strips(F, f)
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
