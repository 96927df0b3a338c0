"""Register guard for the skinny-M GEMM kernel, 16-bit and FP8 weights (CPU: hipcc cross-compiles gfx950
here), by the recipe of ``test_decode_resources.py``: the kernel is bound by the W stream and keeps two
register sets of W / x fragments in flight (in FP8 twice the x fragments per set, plus the converted W
of the MFMA pair), so a spill to scratch would add memory traffic to exactly the path that is limited
by it. Every kernel of the file must compile with ScratchSize 0 under the build's own flags, and the
file holds exactly the instantiations its dispatch declares: 2 weight formats x 2 activation dtypes
(bf16, fp16) x 3 configurations (1, 2 or 4 W tiles per wave) = 12 kernels of the one template. Per
(format, tiles per wave) the VGPR count may not rise above, nor the occupancy fall below, what the two
separate kernels had before they became one template. The file is compiled once; ``test_no_scratch``
looks at the whole file and the 16-bit format, ``test_no_scratch_fp8`` at the FP8 format. Only resource
usage is looked at."""

import functools
import os
import re
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "csrc/gemm/gemm_skinny.hip"

# (format policy in the kernel's template arguments, TN) -> (most VGPRs, least waves per SIMD); bf16 = fp16
LIMITS = {("W16", 4): (192, 2), ("W16", 2): (118, 4), ("W16", 1): (142, 3),
          ("W8", 4): (238, 2), ("W8", 2): (154, 3), ("W8", 1): (214, 2)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@functools.lru_cache(maxsize=None)
def _usage():
    """(mangled name, scratch bytes per lane, VGPRs, waves per SIMD) of every kernel of the file"""
    from cs336_systems._native import build

    path = os.path.join(REPO, SRC)
    head = open(path).read(4096)
    flags = ["-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(REPO, "csrc", "include"),
             "-I" + os.path.join(REPO, "csrc", "flash_attn"), "--offload-arch=gfx950", "-munsafe-fp-atomics"]
    if "cs336-build: agpr-accumulators" not in head:
        flags += list(build.VGPR_FORM)
    if "cs336-build: no-slp" in head:
        flags += ["-fno-slp-vectorize"]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                            os.path.join(tmp, "k.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert names and len(names) == len(scratch) == len(vgprs) == len(occ)
    return tuple(zip(names, scratch, vgprs, occ))


def _key(name):
    # mangled: gemm_skinny_kernelI <policy W16 / W8> I <BF16 / F16> E E Li<TN>E Li<U>E Li<MAXW>E
    m = re.search(r"gemm_skinny_kernelI\w*?\d(W16|W8)I\w*?(BF16|F16)EEELi(\d+)E", name)
    assert m, name
    return m.group(1), m.group(2), int(m.group(3))


def _check_format(fmt):
    mine = [(_key(n), s, v, o) for n, s, v, o in _usage() if _key(n)[0] == fmt]
    assert sorted(k for k, *_ in mine) == sorted((fmt, t, tn) for t in ("BF16", "F16") for tn in (1, 2, 4)), mine
    spills = [(k, s) for k, s, _, _ in mine if s]
    assert not spills, spills
    over = [(k, v, o) for k, _, v, o in mine if v > LIMITS[fmt, k[2]][0] or o < LIMITS[fmt, k[2]][1]]
    assert not over, over


def test_no_scratch():
    names = [n for n, *_ in _usage()]
    assert sum("gemm_skinny_kernel" in n for n in names) == 12 and len(names) == 12, names
    spills = [(n, s) for n, s, _, _ in _usage() if s]
    assert not spills, spills
    _check_format("W16")


def test_no_scratch_fp8():
    _check_format("W8")
