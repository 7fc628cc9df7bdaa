"""No GPU: the projection shim of tests/test_gpu_seq_proj.py compiles against the library's internal headers (as
test_stage_ref_cpu.py::test_stage_shim_compiles does for stage_shim.hip), so a signature that drifts is caught where there is no card."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seq_proj_shim_compiles(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    cc = subprocess.run([hipcc, "-O2", "-std=c++20", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "bb-ocr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                         "-c", os.path.join(ROOT, "tools", "micro", "seq_proj_shim.hip"), "-o", str(tmp_path / "seq_proj_shim.o")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert cc.returncode == 0, cc.stdout.decode()[-2000:]
