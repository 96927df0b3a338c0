"""Resource guard for the weight-only FP8 / MXFP4 tile GEMM above 128 rows (CPU: hipcc cross-compiles gfx950
here), by the recipe of ``test_skinny_w4_resources.py``. ``csrc/gemm/gemm_wqt.hip`` must hold exactly the
kernels of its plan (``csrc/gemm/gemm_wqt_plan.h``): per format and activation dtype one per tile, (128, 128),
(128, 64) and (64, 64), plus one reduce kernel per dtype; each with ScratchSize 0 and within the plan's
register budget (144 VGPRs, 3 waves per SIMD), and the launch's LDS, two buffers of both operands' k-tile,
within the 64 KB that lets two workgroups share a CU. Only resource usage is looked at."""

import re

from . import test_skinny_w4_resources as recipe

pytestmark = recipe.pytestmark

SRC = "csrc/gemm/gemm_wqt.hip"
TILES = [(128, 128), (128, 64), (64, 64)]
MAX_VGPRS, MIN_WAVES, MAX_LDS = 144, 3, 65536


def _key(name):
    # mangled: gemm_wqt_kernelI <policy W8 / W4> I <BF16 / F16> E E Li<BM>E Li<BN>E, or wqt_reduce_kernelI <BF16 / F16> E
    m = re.search(r"gemm_wqt_kernelI\w*?\d(W\d)I\w*?(BF16|F16)EEELi(\d+)ELi(\d+)E", name)
    if m:
        return m.group(1), m.group(2), int(m.group(3)), int(m.group(4))
    m = re.search(r"wqt_reduce_kernelI\w*?(BF16|F16)E", name)
    assert m, name
    return ("reduce", m.group(1))


def test_exactly_the_planned_kernels_without_scratch_within_the_budget(monkeypatch):
    monkeypatch.setattr(recipe, "SRC", SRC)
    usage = recipe._usage.__wrapped__()
    want = [(f, t, bm, bn) for f in ("W8", "W4") for t in ("BF16", "F16") for bm, bn in TILES]
    want += [("reduce", t) for t in ("BF16", "F16")]
    assert sorted(_key(n) for n, *_ in usage) == sorted(want)
    spills = [(n, s) for n, s, _, _ in usage if s]
    assert not spills, spills
    over = [(_key(n), v, o) for n, _, v, o in usage if v > MAX_VGPRS or o < MIN_WAVES]
    assert not over, over
    # dynamic LDS of a launch: 2 buffers x (BM + BN) rows x 64 k x 2 bytes (wqt_lds_bytes)
    assert all(2 * (bm + bn) * 64 * 2 <= MAX_LDS for bm, bn in TILES)
