"""Register guard for the MXFP4 format of the skinny-M GEMM kernel (CPU: hipcc cross-compiles gfx950 here), by
the recipe of ``test_skinny_resources.py``. The kernel is bound by the W stream and keeps two register sets of
W / x fragments and block-scale bytes in flight, so a spill to scratch would add memory traffic to exactly
the path that is limited by it. ``csrc/gemm/gemm_skinny_w4.hip`` must hold exactly its 6 kernels -- the W4
policy of the one template x 2 activation dtypes (bf16, fp16) x 3 configurations (1, 2 or 4 W tiles per
wave) -- each with ScratchSize 0 under the build's own flags. There is no predecessor to compare with: the
VGPR and occupancy figures of the first build are the limits (TN 4: 195 VGPRs, 2 waves per SIMD; TN 2: 134,
3; TN 1: 191, 2; bf16 = fp16). Only resource usage is looked at."""

import functools
import os
import re
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "csrc/gemm/gemm_skinny_w4.hip"

# TN -> (most VGPRs, least waves per SIMD); bf16 = fp16
LIMITS = {4: (195, 2), 2: (134, 3), 1: (191, 2)}
# TN -> (U, MAXW) of the configuration, as the plan (csrc/gemm/skinny_plan.h) has them for this format
CONFIG = {4: (2, 4), 2: (2, 8), 1: (4, 8)}

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
    # mangled: gemm_skinny_kernelI <policy W4> I <BF16 / F16> E E Li<TN>E Li<U>E Li<MAXW>E
    m = re.search(r"gemm_skinny_kernelI\w*?\d(W\d+)I\w*?(BF16|F16)EEELi(\d+)ELi(\d+)ELi(\d+)E", name)
    assert m, name
    return m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))


def test_exactly_the_six_mxfp4_kernels():
    keys = sorted(_key(n) for n, *_ in _usage())
    want = sorted(("W4", t, tn, *CONFIG[tn]) for t in ("BF16", "F16") for tn in (1, 2, 4))
    assert keys == want, keys


def test_no_scratch_and_register_limits():
    spills = [(n, s) for n, s, _, _ in _usage() if s]
    assert not spills, spills
    over = [(_key(n), v, o) for n, _, v, o in _usage() if v > LIMITS[_key(n)[2]][0] or o < LIMITS[_key(n)[2]][1]]
    assert not over, over
