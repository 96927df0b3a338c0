"""Register-spill guard for the FP8 weight-only skinny-M GEMM kernel (CPU: hipcc cross-compiles gfx950
here), by the recipe of ``test_skinny_resources.py``. The kernel holds two register sets of W bytes and
twice the 16-bit kernel's x fragments per set, plus the converted W of the MFMA pair in flight; a
spill to scratch would add memory traffic to the path that is bound by it. Every kernel of the file
must compile with ScratchSize 0 under the build's own flags, and the file holds exactly the
instantiations its dispatch declares: 2 activation dtypes (bf16, fp16) x 3 configurations (1, 2 or 4
W tiles per wave) = 6 kernels. Only resource usage is looked at."""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "csrc/gemm/gemm_skinny_w8.hip"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_scratch(tmp_path):
    from cs336_systems._native import build

    path = os.path.join(REPO, SRC)
    head = open(path).read(4096)
    flags = ["-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(REPO, "csrc", "include"),
             "-I" + os.path.join(REPO, "csrc", "flash_attn"), "--offload-arch=gfx950", "-munsafe-fp-atomics"]
    if "cs336-build: agpr-accumulators" not in head:
        flags += list(build.VGPR_FORM)
    if "cs336-build: no-slp" in head:
        flags += ["-fno-slp-vectorize"]
    r = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                        str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert names and len(names) == len(scratch)
    assert sum("gemm_skinny_w8_kernel" in n for n in names) == 6 and len(names) == 6, names
    spills = [(n, s) for n, s in zip(names, scratch) if s]
    assert not spills, spills
