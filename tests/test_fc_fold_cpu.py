"""CPU: the fold of fc6 -> fc7 -> upconv1's 1x1 into one dilated conv (bb-ocr_amd/csrc/fc_fold.h) as tools/fc_fold_hostcheck.cpp runs it -- a
stand-alone host program with its own main, no HIP, nothing loaded into python.

The program builds small random chains (Cin 8, mids 12 and 10, Cout 6, 5 skip channels, BatchNorm with non-trivial running statistics,
dilation 2, images 7 x 9 and 3 x 2), compares the folded dilated conv + 1x1 with the layer-by-layer chain in double (1e-12 of the largest
pre-activation), shows that four named mistakes are seen by that comparison, and checks the float instantiation the library uses.  It is built
and run twice: plainly, and once under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISTAKES = ["W7 b6 left out of b'", "BN scale on the Ws block only", "Wy and Ws columns swapped", "taps transposed"]


def _cxx():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no host C++ compiler on this box")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fc_fold") / f"fc_fold_hostcheck_{request.param}")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cc = subprocess.run([_cxx(), "-std=c++20", "-pthread"] + flags + [os.path.join(ROOT, "tools", "fc_fold_hostcheck.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert cc.returncode == 0, cc.stdout.decode()[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r


def test_hostcheck_ends_clean(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "0 failures" and all(l.startswith("ok ") for l in lines[:-1]), run.stdout


@pytest.mark.parametrize("shape", ["7 x 9", "3 x 2"])
def test_fold_equals_the_chain_in_double(run, shape):
    got = [l for l in run.stdout.splitlines() if "against the chain in double" in l and l.split(":")[0].endswith(shape)]
    assert len(got) == 2 and all(l.startswith("ok ") for l in got), got          # over a pool and on one thread
    assert all(float(l.rsplit(":", 1)[1]) <= 1e-12 for l in got), got


@pytest.mark.parametrize("shape", ["7 x 9", "3 x 2"])
@pytest.mark.parametrize("mistake", MISTAKES)
def test_mistake_is_seen(run, mistake, shape):
    got = [l for l in run.stdout.splitlines() if f"mistake seen (> 1e-6): {mistake}, {shape}:" in l]
    assert len(got) == 1 and got[0].startswith("ok "), (got, run.stdout)
    assert float(got[0].rsplit(":", 1)[1]) > 1e-6


def test_float_fold_is_the_double_fold_rounded_once(run):
    got = [l for l in run.stdout.splitlines() if "float fold == double fold rounded once" in l]
    assert len(got) == 1 and got[0].startswith("ok ") and float(got[0].rsplit(":", 1)[1]) == 0.0, got
