"""gemm8w's K-tile pipeline (csrc/gemm/gemm8w.hip: A fragments read one phase ahead into a second
set, the LDS-DMA of a K-tile issued from four points), checked bit for bit.

Operands are integer-valued bf16 in [-4, 4]; with at most 320 tokens every partial sum is an
integer below 2^14, so fp32 accumulation is exact in any order and the result must *equal*
``a.float().t() @ b.float()``. One mis-staged fragment, one read ahead of its DMA or one restage
ahead of a region's last read fails that, where a relative-norm bound need not. The shapes are the
smallest that reach every prologue, tail and stage-parity path: 1 to 5 K-tiles, splits of 1, 2 and 3
K-tiles, a padded row tile, several tiles, both tile widths (FN 5: N % 320 == 0, FN 4: N % 256 == 0)
and both store forms."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cs():
    from cs336_systems import ops

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load_ext(), ops.load_error()
    return torch.ops.cs336


def _ints(rows, cols, seed, guard=0):
    """Integer-valued bf16 (rows, cols) in [-4, 4]; guard > 0: a row-slice of a buffer with that many
    NaN rows before and after it."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randint(-4, 5, (rows, cols), device="cuda", generator=g).to(torch.bfloat16)
    if not guard:
        return v
    buf = torch.full((rows + 2 * guard, cols), float("nan"), device="cuda", dtype=torch.bfloat16)
    buf[guard: guard + rows] = v
    return buf[guard: guard + rows]


def _run(cs, a, b, trans, splits, out=None, accumulate=False):
    M, N = a.shape[1], b.shape[1]
    shape = (N, M) if trans else (M, N)
    if splits > 1:
        slabs = torch.full((splits, *shape), float("nan"), device="cuda")
        cs.gemm8w(a, b, slabs, splits, trans, False, 0)
        got = slabs.sum(0)
    else:
        got = torch.full(shape, float("nan"), device="cuda") if out is None else out
        cs.gemm8w(a, b, got, 1, trans, accumulate, 0)
    return got.t() if trans else got


CASES = [
    # K, M, N, trans, splits
    (64, 256, 320, False, 1), (64, 256, 320, True, 1),  # one K-tile: no read-ahead target
    (128, 256, 320, False, 1), (128, 256, 320, True, 1),  # the last two K-tiles: no restage,
    (192, 256, 320, False, 1), (192, 256, 320, True, 1),  # both stage parities
    (256, 256, 320, False, 1), (320, 256, 320, False, 1),  # steady state
    (192, 256, 320, False, 3),  # one K-tile per split
    (320, 256, 320, False, 2),  # uneven 2 + 3 split
    (320, 256, 320, False, 4),  # splits of 1 and 2 K-tiles
    (128, 264, 320, False, 1),  # padded row tile
    (128, 320, 320, False, 1),  # padded tile with 64 valid rows: wave group 1 all padding
    (192, 512, 640, False, 1),  # several tiles
    (192, 256, 256, False, 1), (192, 256, 256, True, 1),  # FN 4
    (192, 256, 512, False, 1), (192, 256, 512, True, 1),  # FN 4, two column tiles
]


@pytest.mark.parametrize("K,M,N,trans,splits", CASES)
def test_gemm8w_phases_exact(K, M, N, trans, splits):
    cs = _cs()
    a, b = _ints(K, M, seed=K + M), _ints(K, N, seed=K + N + 1)
    ref = a.float().t() @ b.float()
    got = _run(cs, a, b, trans, splits)
    assert torch.equal(got, ref), int((got != ref).sum())


def test_gemm8w_phases_accumulate():
    """accumulate=True onto an integer-valued out."""
    cs = _cs()
    K, M, N = 128, 256, 320
    a, b = _ints(K, M, seed=11), _ints(K, N, seed=12)
    g = torch.Generator(device="cuda").manual_seed(13)
    out0 = torch.randint(-64, 65, (M, N), device="cuda", generator=g).float()
    ref = a.float().t() @ b.float() + out0
    got = _run(cs, a, b, False, 1, out=out0.clone(), accumulate=True)
    assert torch.equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("splits", [1, 3])
def test_gemm8w_phases_nan_guards(splits):
    """Operands are row-slices of larger NaN-filled buffers and out is pre-filled with NaN: a read or
    DMA outside the operand (or, with splits, outside a split's own rows: those are other integers)
    poisons or changes the result, and an unwritten element stays NaN."""
    cs = _cs()
    K, M, N = 192, 256, 320
    a, b = _ints(K, M, seed=21, guard=64), _ints(K, N, seed=22, guard=64)
    ref = a.float().t() @ b.float()
    got = _run(cs, a, b, False, splits)
    assert torch.equal(got, ref), int((got != ref).sum())
