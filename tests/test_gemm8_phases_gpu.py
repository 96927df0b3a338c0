"""gemm8's K-tile pipeline (csrc/gemm/gemm8.hip: two phases per K-tile split by rows, the LDS-DMA of
a K-tile issued in two parts with counted waits), checked bit for bit.

Operands are integer-valued bf16 in [-4, 4]; with K <= 320 every partial sum is an integer below
2^13, so fp32 accumulation is exact in any order and the bf16 result must *equal*
``(a.float() @ b.float().t()).bfloat16()``. One mis-staged fragment, one read ahead of its DMA or one
restage ahead of a region's last read fails that, where a relative-norm bound need not. The shapes
are the smallest that reach every prologue, tail and stage-parity path: 1 to 5 K-tiles (no next
K-tile, no K-tile after next, both stage parities, steady state), one and several tiles of both tile
widths (FN 5: N % 320 == 0, FN 4: N % 256 == 0), the K and N tails, and every epilogue kind.

Every operand is a slice of a larger NaN-filled buffer (guard rows before and after, guard columns
left and right) and the output is a slice of a NaN-filled buffer: a read or DMA outside the operand
poisons the result, an unwritten element stays NaN and a store outside the output shows in its
guard columns."""

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8


def _cs():
    from cs336_systems import ops

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load_ext(), ops.load_error()
    return torch.ops.cs336


def _guarded(v):
    """v as a slice of a NaN-filled buffer with GUARD rows / columns on every side."""
    rows, cols = v.shape
    buf = torch.full((rows + 2 * GUARD, cols + 2 * GUARD), float("nan"), device="cuda", dtype=v.dtype)
    view = buf[GUARD: GUARD + rows, GUARD: GUARD + cols]
    view.copy_(v)
    return buf, view


def _ints(rows, cols, seed):
    """Integer-valued bf16 (rows, cols) in [-4, 4] inside NaN guards."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return _guarded(torch.randint(-4, 5, (rows, cols), device="cuda", generator=g).to(torch.bfloat16))[1]


def _out(rows, cols):
    """(buffer, view): a NaN-filled output inside NaN guard columns."""
    buf = torch.full((rows, cols + 2 * GUARD), float("nan"), device="cuda", dtype=torch.bfloat16)
    return buf, buf[:, GUARD: GUARD + cols]


def _guards_untouched(buf, cols):
    return bool(torch.isnan(buf[:, :GUARD]).all()) and bool(torch.isnan(buf[:, GUARD + cols:]).all())


def _exact(a, b):
    return (a.float() @ b.float().t()).bfloat16()


KS = [64, 128, 192, 256, 320]  # 1 to 5 K-tiles
MN = [(M, N) for M in (256, 512) for N in (320, 640, 256, 512)]  # FN 5: 320, 640; FN 4: 256, 512
TAILS = [
    # M, N, K
    (256, 320, 72), (256, 320, 200),  # K tails: 2 and 4 K-tiles, the last one 8 wide
    (512, 640, 200),
    (256, 328, 128), (512, 328, 192),  # N tail: a second column tile 8 wide (FN 4)
    (256, 600, 128),  # N tail at FN 5: a second column tile 280 wide
    (256, 328, 72), (256, 328, 200),  # both
]


@pytest.mark.parametrize("M,N", MN)
@pytest.mark.parametrize("K", KS)
def test_gemm8_phases_exact(K, M, N):
    cs = _cs()
    a, b = _ints(M, K, seed=K + M), _ints(N, K, seed=K + N + 1)
    cbuf, c = _out(M, N)
    cs.gemm8(a, b, c, 0, 0, None, None, 0)
    ref = _exact(a, b)
    assert torch.equal(c, ref), int((c != ref).sum())
    assert _guards_untouched(cbuf, N)


@pytest.mark.parametrize("M,N,K", TAILS)
def test_gemm8_phases_tails_exact(M, N, K):
    cs = _cs()
    a, b = _ints(M, K, seed=K + M + 2), _ints(N, K, seed=K + N + 3)
    cbuf, c = _out(M, N)
    cs.gemm8(a, b, c, 0, 0, None, None, 0)
    ref = _exact(a, b)
    assert torch.equal(c, ref), int((c != ref).sum())
    assert _guards_untouched(cbuf, N)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


@pytest.mark.parametrize("half", [160, 128])  # FN 5 / FN 4
@pytest.mark.parametrize("K", [128, 320])
def test_gemm8_phases_swiglu_forward(K, half):
    """EPI 1: the stored y = [a|b] is the exact product; h = silu(a)·b of the stored a, b to the
    tolerance of tests/test_gemm8_gpu.py."""
    cs = _cs()
    M = 256
    x, w13 = _ints(M, K, seed=K + 5), _ints(2 * half, K, seed=K + half)
    ybuf, y = _out(M, 2 * half)
    hbuf, h = _out(M, half)
    cs.gemm8(x, w13, y, 1, 0, h, None, half)
    ref = _exact(x, w13)
    assert torch.equal(y, ref), int((y != ref).sum())
    yb = ref.float()
    hr = torch.nn.functional.silu(yb[:, :half]) * yb[:, half:]
    assert _rel(h, hr) < 5e-3
    assert _guards_untouched(ybuf, 2 * half) and _guards_untouched(hbuf, half)


@pytest.mark.parametrize("half", [320, 256])  # FN 5 / FN 4 (EPI 2: N = half)
@pytest.mark.parametrize("K", [128, 320])
def test_gemm8_phases_swiglu_backward(K, half):
    """EPI 2: [da|db] from dh = dY·W2 (never stored) and the saved a, b, to the tolerance of
    tests/test_gemm8_gpu.py."""
    cs = _cs()
    M = 256
    dy, w2t = _ints(M, K, seed=K + 7), _ints(half, K, seed=K + half + 8)
    g = torch.Generator(device="cuda").manual_seed(9)
    y = _guarded(((torch.rand(M, 2 * half, device="cuda", generator=g) * 2 - 1) * 3).to(torch.bfloat16))[1]
    dbuf, dab = _out(M, 2 * half)
    cs.gemm8(dy, w2t, dab, 2, 0, None, y, half)
    dh = dy.float() @ w2t.float().t()
    a, b = y.float()[:, :half], y.float()[:, half:]
    s = torch.sigmoid(a)
    da = dh * b * s * (1 + a * (1 - s))
    db = dh * a * s
    assert _rel(dab[:, :half], da) < 5e-3
    assert _rel(dab[:, half:], db) < 5e-3
    assert _guards_untouched(dbuf, 2 * half)


@pytest.mark.parametrize("N,rope_cols", [(640, 320), (512, 256)])  # FN 5 / FN 4
@pytest.mark.parametrize("K", [128, 320])
def test_gemm8_phases_rope_exact(K, N, rope_cols):
    """EPI 3 with cos/sin tables holding only 0 and +-1 (quarter turns): the rotation of the
    bf16-rounded product is exact, so the output must equal the rotated exact product."""
    cs = _cs()
    M, dh, seq = 256, 64, 64
    a, b = _ints(M, K, seed=K + 11), _ints(N, K, seed=K + N + 12)
    g = torch.Generator(device="cuda").manual_seed(13)
    turn = torch.randint(0, 4, (seq, dh // 2), device="cuda", generator=g)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0], device="cuda")[turn].contiguous()
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0], device="cuda")[turn].contiguous()
    cbuf, c = _out(M, N)
    cs.gemm8_rope(a, b, c, cos, sin, None, seq, rope_cols, dh)
    ref = _exact(a, b).float()
    pos = torch.arange(M, device="cuda") % seq
    qk = ref[:, :rope_cols].reshape(M, -1, dh // 2, 2)
    cc, ss = cos[pos][:, None, :], sin[pos][:, None, :]
    x0, x1 = qk[..., 0], qk[..., 1]
    rot = torch.stack((cc * x0 - ss * x1, ss * x0 + cc * x1), dim=-1).reshape(M, rope_cols)
    ref = torch.cat((rot, ref[:, rope_cols:]), dim=1).bfloat16()
    assert torch.equal(c, ref), int((c != ref).sum())
    assert _guards_untouched(cbuf, N)
