"""Register-spill guard for the FP8 KV cache kernels (CPU: hipcc cross-compiles gfx950 here), by the
recipe of ``test_decode_resources.py``: the attention kernels keep their packed K / V rows, the row
scales, the query slices and the output slices in registers, and the append / quantize kernels a row
slice per lane. Every kernel of the two files must compile with ScratchSize 0 under the build's own
flags; there is no exceptions list. The instantiation counts are pinned: the merge kernels are not
among them (the partials are merged by ``fa_decode.hip`` / ``fa_decode_chunk.hip``'s own)."""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# kernel name -> instantiations: 3 q / x dtypes x 4 head dims (the chunk kernel has one query tile)
SOURCES = {
    "csrc/flash_attn/fa_decode_kv8.hip": {"fa_decode_kv8_kernel": 12, "kv_append_rope_kv8_kernel": 12,
                                         "kv_quantize_rows_kernel": 12},
    "csrc/flash_attn/fa_decode_chunk_kv8.hip": {"fa_decode_chunk_kv8_kernel": 12},
}


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
    assert len(names) == sum(SOURCES[src].values())  # ... and nothing else, a copied merge kernel included
    spills = [(n, s) for n, s in zip(names, scratch) if s]
    assert not spills, spills
