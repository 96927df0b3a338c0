"""Plan invariants of the skinny-M decode GEMM for MXFP4 weights (CPU): ``csrc/tests/skinny_w4_plan_check.cpp``
is a stand-alone host program, built here with the ordinary host compiler and no sanitizer, that walks
``gemm_skinny_plan(SkinnyFormat::MXFP4, N, K)`` over every N up to 8300 and every K % 32 == 0 up to 10240:
the tiles-per-wave thresholds, ``waves <=`` full register sets, and workgroups that cover the tiles exactly."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_mxfp4_plan_invariants(tmp_path):
    exe = str(tmp_path / "skinny_w4_plan_check")
    r = subprocess.run([CXX, "-O1", "-std=c++17", "-I" + os.path.join(REPO, "csrc", "include"), os.path.join(REPO, "csrc", "tests", "skinny_w4_plan_check.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mxfp4 plan checks passed" in r.stdout
