"""Register guard for the weight-only FP8 / MXFP4 GEMM for 17..128 rows (CPU: hipcc cross-compiles gfx950
here), by the recipe of ``test_skinny_w4_resources.py``. ``csrc/gemm/gemm_wq.hip`` must hold exactly the
kernels of its plan (``csrc/gemm/gemm_wq_plan.h``): per format and activation dtype, one per (MB, tiles per
workgroup) pair from the format's floor (MB / 2 tiles for e4m3, MB for MXFP4) up to 8 tiles -- 9 + 6 pairs x 2
dtypes = 30 -- each with ScratchSize 0 under the build's own flags: the accumulators, two W register sets,
the converted operands and the staged x slab all live in registers. The VGPR and occupancy figures of the
first build are the limits (bf16 = fp16). Only resource usage is looked at."""

import re

from . import test_skinny_w4_resources as recipe

pytestmark = recipe.pytestmark

SRC = "csrc/gemm/gemm_wq.hip"
# (format, MB, TN, RW) -> (most VGPRs, least waves per SIMD); tiles per workgroup = TN x RW
LIMITS = {
    ("W8", 2, 1, 1): (246, 2), ("W8", 2, 1, 2): (138, 3), ("W8", 2, 2, 2): (176, 2), ("W8", 2, 2, 4): (152, 3),
    ("W8", 4, 1, 2): (128, 4), ("W8", 4, 2, 2): (157, 3), ("W8", 4, 2, 4): (134, 3),
    ("W8", 8, 2, 2): (208, 2), ("W8", 8, 2, 4): (170, 2),
    ("W4", 2, 1, 2): (133, 3), ("W4", 2, 2, 2): (166, 3), ("W4", 2, 2, 4): (142, 3),
    ("W4", 4, 2, 2): (169, 2), ("W4", 4, 2, 4): (125, 4),
    ("W4", 8, 2, 4): (256, 1),  # plus 18 AGPRs: the one kernel at one wave per SIMD
}


def _usage(monkeypatch):
    monkeypatch.setattr(recipe, "SRC", SRC)
    return recipe._usage.__wrapped__()


def _key(name):
    # mangled: gemm_wq_kernelI <policy W8 / W4> I <BF16 / F16> E E Li<MB>E Li<TN>E Li<RW>E
    m = re.search(r"gemm_wq_kernelI\w*?\d(W\d)I\w*?(BF16|F16)EEELi(\d+)ELi(\d+)ELi(\d+)E", name)
    assert m, name
    return m.group(2), (m.group(1), int(m.group(3)), int(m.group(4)), int(m.group(5)))


def test_exactly_the_planned_kernels_without_scratch_within_the_register_limits(monkeypatch):
    usage = _usage(monkeypatch)
    assert sorted(_key(n) for n, *_ in usage) == sorted((t, k) for t in ("BF16", "F16") for k in LIMITS)
    spills = [(n, s) for n, s, _, _ in usage if s]
    assert not spills, spills
    over = [(_key(n), v, o) for n, _, v, o in usage if v > LIMITS[_key(n)[1]][0] or o < LIMITS[_key(n)[1]][1]]
    assert not over, over
