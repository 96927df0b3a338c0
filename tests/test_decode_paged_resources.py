"""Register-spill guard for the paged decode-attention and append kernels (CPU: hipcc cross-compiles
gfx950 here), by the recipe of ``test_decode_resources.py``: ``fa_decode_paged.hip`` is compiled with
the build's own flags, must hold 12 attention kernels (3 dtypes x 4 head dims) and 3 append kernels,
and every one of them must have ScratchSize 0."""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "csrc/flash_attn/fa_decode_paged.hip"


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
    assert sum("fa_decode_paged_kernel" in n for n in names) == 12
    assert sum("kv_append_rope_paged_kernel" in n for n in names) == 3
    spills = [(n, s) for n, s in zip(names, scratch) if s]
    assert not spills, spills
