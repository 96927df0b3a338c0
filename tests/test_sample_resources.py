"""Register-spill guard for the fused sampler (CPU: hipcc cross-compiles gfx950 here), by the recipe of
``test_decode_kv8_resources.py``: a thread keeps its 8 elements of a tile, their weights and the
running sums in registers, at 1024 threads per workgroup (at most 128 registers each). Every kernel
of ``csrc/ops/sample.hip`` must compile with ScratchSize 0 under the build's own flags. The
instantiation count is pinned: ``sample_logits`` and ``sample_advance`` share one kernel per dtype."""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = {"csrc/ops/sample.hip": {"sample_kernel": 3}}  # 3 logits dtypes


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(SOURCES))
def test_no_scratch(src, tmp_path):
    from cs336_systems._native import build

    path = os.path.join(REPO, src)
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
    for kernel, count in SOURCES[src].items():
        assert sum(kernel in n for n in names) == count, kernel
    assert len(names) == sum(SOURCES[src].values())  # ... and nothing else
    spills = [(n, s) for n, s in zip(names, scratch) if s]
    assert not spills, spills
