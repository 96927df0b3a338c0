"""Register-spill guard for the multi-token decode-attention and chunk-append kernels (CPU: hipcc
cross-compiles gfx950 here), by the recipe of ``test_decode_resources.py``. The query-tile kernel keeps
the K / V rows, QT query slices and QT output slices in registers; a spill to scratch would put extra
memory traffic into the path that is limited by it. Every kernel of the file must compile with
ScratchSize 0 under the build's own flags; there is no exceptions list."""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "csrc/flash_attn/fa_decode_chunk.hip"


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
    # 3 dtypes x 4 head dims x query tiles {1, 4, 8} of the chunk kernel, 3 x 4 merge kernels, 3
    # dtypes of the append kernel
    assert sum("fa_decode_chunk_kernel" in n for n in names) == 36
    assert sum("fa_decode_chunk_merge_kernel" in n for n in names) == 12
    assert sum("kv_append_rope_chunk_kernel" in n for n in names) == 3
    assert len(names) == 51
    spills = [(n, s) for n, s in zip(names, scratch) if s]
    assert not spills, spills
