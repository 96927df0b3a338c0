"""The diagnostic stamp buffer of gemm8 and gemm8w (the op ``gemm8_stamps``; csrc/gemm/gemm_common.h,
``PhaseStamps``): setting it, and taking it away again, never changes a result, the shipped build
never writes to it, and a build with -DCS336_G8_STAMP (loaded through ``CS336_LIB``) writes the row
layout that ``analyse`` in scripts/gemm8w_stamps.py reads.

One tile of each kernel with three k-tiles, the smallest shape that runs prologue, steady-state and
last-tile code: gemm8 M 256, N 320, K 192 (epi 0); gemm8w 192 token rows, M 256, N 320. Each is one
workgroup, so the (5, 8) buffer has gemm8's own row, its four per-phase rows behind it, and room for
gemm8w's four rows (which start at row 0: the buffer is zeroed between the two kernels)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, K = 256, 320, 192
BLOCKS = 1


def _cs():
    from cs336_systems import ops

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load_ext(), ops.load_error()
    return torch.ops.cs336


def test_stamp_buffer_leaves_results_alone_and_rows_parse():
    cs = _cs()
    g = torch.Generator(device="cuda").manual_seed(7)

    def rnd(r, c):
        return (torch.rand(r, c, device="cuda", generator=g) * 2 - 1).bfloat16()

    a, b = rnd(M, K), rnd(N, K)  # gemm8: c = a @ b.T
    dy, x = rnd(K, M), rnd(K, N)  # gemm8w: dw = dy.T @ x over K token rows

    def run8():
        c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        cs.gemm8(a, b, c, 0, 0, None, None, 0)
        return c

    def run8w():
        dw = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32)
        cs.gemm8w(dy, x, dw, 1, False, False, 0)
        return dw

    cs.gemm8_stamps(None)
    ref8, ref8w = run8(), run8w()
    assert bool(torch.isfinite(ref8).all()) and bool(torch.isfinite(ref8w).all())

    buf = torch.zeros(5 * BLOCKS, 8, dtype=torch.int64, device="cuda")
    try:
        built = cs.gemm8_stamps(buf)
        with8 = run8()
        rows8 = buf.clone()
        buf.zero_()
        with8w = run8w()
        rows8w = buf.clone()
    finally:
        cs.gemm8_stamps(None)
    buf.zero_()
    after8, after8w = run8(), run8w()
    torch.cuda.synchronize()

    assert torch.equal(with8, ref8) and torch.equal(after8, ref8)
    assert torch.equal(with8w, ref8w) and torch.equal(after8w, ref8w)
    assert not bool(buf.any()), "a launch after gemm8_stamps(None) wrote stamps"
    if not built:
        assert not bool(rows8.any()) and not bool(rows8w.any()), "the shipped build wrote stamps"
        return
    # gemm8: one row per workgroup (four s_memtime, two s_memrealtime, HW_ID, XCC_ID) ...
    assert bool((rows8[:BLOCKS, :6] != 0).all()), rows8[:BLOCKS].tolist()
    # ... and behind those, at level 2 only, the per-phase rows in gemm8w's layout
    ph8 = rows8[BLOCKS:].view(BLOCKS, 4, 8)
    if bool(ph8.any()):
        _check_phase_rows(ph8)
    _check_phase_rows(rows8w[: 4 * BLOCKS].view(BLOCKS, 4, 8))
    assert not bool(rows8w[4 * BLOCKS:].any())


def _check_phase_rows(st):
    """st: (workgroups, 4, 8), per wave group g rows 2g (work[4], wait[4]) and 2g + 1 (mma[4], stamped
    k-tiles, k-tiles, HW_ID, XCC_ID); two phases are in use."""
    for g in (0, 1):
        first, second = st[:, 2 * g], st[:, 2 * g + 1]
        assert bool((first[:, [0, 1, 4, 5]] > 0).all()) and bool((second[:, :2] > 0).all()), st.tolist()
        assert bool((second[:, 4] == K // 64).all()), st.tolist()  # all three k-tiles are stamped
        assert bool((second[:, 5] == K // 64).all()), st.tolist()
