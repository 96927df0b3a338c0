"""The skinny-M GEMM kernel (``csrc/gemm/gemm_skinny.hip``, ``cs336::gemm_skinny``) against an fp64
oracle, with the one comparison rule of ``test_kernel_edges_gpu.py`` (``check``, ``k = 4``):
``ref64 = x.double() @ w.double().T`` and the same product in plain fp32, both from the rounded 16-bit
inputs.

Shapes are the smallest at which the code takes another path: M 1 / 3 / 16 (one row, a partial and a
full MFMA tile of batch rows); N 1 / 15 / 16 / 17 / 48 (less than, exactly and more than one 16-row W
tile, several workgroups) and the vocabulary head's 50257 (not a multiple of 4: scalar stores); K 8 (a
single 16-B load), 40 and 1608 (not multiples of the 32-k MFMA block nor of a register set), 64, 1600.
``PATHS`` adds the shapes that engage the rest of the dispatch: a K long enough that all 8 waves of a
workgroup own several register sets (the in-workgroup K split and the ping-pong loop), and W tall
enough for the 2- and 4-tiles-per-wave kernels (N >= 4096 / 8192), each with a short and a long K.

Measured ``max (|got - ref64| - u*|ref64|) / E32`` on an MI355X: at most 0.16 over every case here (0 in
most: the error stays within the one rounding to the output type), so the rule's ``k = 4`` holds
everywhere and no case has a margin of its own."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext, gemm

from .test_kernel_edges_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
MS = (1, 3, 16)
NS = (1, 15, 16, 17, 48)
KS = (8, 40, 64, 1600, 1608)
PATHS = [(48, 8232), (4100, 1608), (4100, 4104), (8200, 1608), (8200, 4104)]


def _hip():
    return _ext.ops()


def _inputs(M, N, K, dt, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w = torch.randn(N, K, device=DEV, generator=g).to(dt)
    return x, w


def _refs(x, w):
    return x.double() @ w.double().t(), x.float() @ w.float().t()


def _run(x, w, out=None):
    out = torch.empty(x.shape[0], w.shape[0], device=DEV, dtype=x.dtype) if out is None else out
    _hip().gemm_skinny(x, w, out)
    return out


def _check(x, w, got, tag):
    ref64, ref32 = _refs(x, w)
    r = check(got, ref64, ref32, x.dtype, f"gemm_skinny.{tag}")
    print(f"gemm_skinny.{tag} M {x.shape[0]} N {w.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_small_shapes(dt, K):
    for M in MS:
        for N in NS:
            x, w = _inputs(M, N, K, dt)
            _check(x, w, _run(x, w), "small")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_vocabulary_head(dt):
    for M in MS:
        x, w = _inputs(M, 50257, 64, dt)
        _check(x, w, _run(x, w), "vocab")


@pytest.mark.parametrize("N,K", PATHS)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_dispatch_paths(dt, N, K):
    for M in (3, 16):
        x, w = _inputs(M, N, K, dt)
        _check(x, w, _run(x, w), "paths")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_views(dt):
    M, N, K = 3, 48, 1608
    x, w = _inputs(M, N, K, dt)
    ref = _run(x, w)
    xb = torch.zeros(2 * M, K, device=DEV, dtype=dt)
    xb[::2] = x
    wg = torch.randn(3 * N, K, device=DEV).to(dt)  # the grouped QKV layout: w is its middle row block
    wg[N:2 * N] = w
    ob = torch.zeros(M, N + 16, device=DEV, dtype=dt)
    out = ob[:, 8:8 + N]
    _run(xb[::2], wg[N:2 * N], out)
    assert torch.equal(out, ref)
    assert not ob[:, :8].any() and not ob[:, 8 + N:].any()
    _check(x, w, out, "views")
    # an odd column offset: out rows are not 8-B aligned, the kernel stores element by element
    out = ob[:, 3:3 + N]
    _run(x, w, out)
    assert torch.equal(out, ref)
    # ops.skinny_linear and the routed mm_nt give the same bits, with leading dims restored
    assert torch.equal(ops.skinny_linear(x.view(M, 1, K), w), ref.view(M, 1, N))
    with gemm.skinny_decode():
        assert torch.equal(gemm.mm_nt(x, w), ref)


@pytest.mark.parametrize("dt,M,N,K", [(BF16, 3, 17, 1608), (F16, 16, 50257, 64)])
def test_nan_poisoning(dt, M, N, K):
    """All three operands are cut out of larger NaN-filled buffers: a W row >= N, a batch row >= M or
    a k >= K that leaked into a stored value, or a store outside ``out``, shows without any fault."""
    x, w = _inputs(M, N, K, dt, seed=1)
    nan = float("nan")
    xb = torch.full((M + 2, K + 16), nan, device=DEV, dtype=dt)
    wb = torch.full((N + 2, K + 16), nan, device=DEV, dtype=dt)
    ob = torch.full((M + 2, N + 16), nan, device=DEV, dtype=dt)
    xb[1:M + 1, 8:8 + K] = x
    wb[1:N + 1, 8:8 + K] = w
    before = ob.clone().view(torch.int16)
    out = ob[1:M + 1, 4:4 + N]
    _run(xb[1:M + 1, 8:8 + K], wb[1:N + 1, 8:8 + K], out)
    assert torch.isfinite(out).all()
    _check(x, w, out, "poisoned")
    after = ob.view(torch.int16).clone()
    after[1:M + 1, 4:4 + N] = before[1:M + 1, 4:4 + N]
    assert torch.equal(after, before)  # the bytes around out are untouched


@pytest.mark.parametrize("dt", [BF16, F16])
def test_bitwise_reproducible(dt):
    for M, N, K in [(16, 48, 8232), (3, 8200, 1608), (1, 50257, 64)]:
        x, w = _inputs(M, N, K, dt, seed=2)
        assert torch.equal(_run(x, w), _run(x, w))


def test_unsupported_inputs_raise_and_skinny_linear_falls_back():
    def raises(x, w, out=None):
        out = torch.empty(x.shape[0], w.shape[0], device=DEV, dtype=x.dtype) if out is None else out
        with pytest.raises(RuntimeError):
            _hip().gemm_skinny(x, w, out)

    x, w = _inputs(17, 32, 64, BF16)  # M = 17
    raises(x, w)
    assert torch.equal(ops.skinny_linear(x, w), gemm.mm_nt(x, w))
    x, w = _inputs(4, 32, 12, BF16)  # K % 8 != 0
    raises(x, w)
    assert torch.equal(ops.skinny_linear(x, w), gemm.mm_nt(x, w))
    x, w = _inputs(4, 32, 64, BF16)
    raises(x.float(), w.float())  # fp32
    assert torch.equal(ops.skinny_linear(x.float(), w.float()), gemm.mm_nt(x.float(), w.float()))
    xb = torch.zeros(4, 72, device=DEV, dtype=BF16)
    xm = xb[:, 4:68]  # rows start 8 bytes off a 16-byte boundary
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 8
    raises(xm, w)
    assert torch.equal(ops.skinny_linear(xm, w), gemm.mm_nt(xm, w))
    raises(x, w.to(F16))  # mismatched dtypes
    raises(x, w, torch.empty(4, 32, device=DEV, dtype=F16))
    with pytest.raises(RuntimeError):  # ... which the existing path refuses as well
        gemm.mm_nt(x, w.to(F16))
    with pytest.raises(RuntimeError):
        ops.skinny_linear(x, w.to(F16))
    raises(x, w, torch.empty(4, 31, device=DEV, dtype=BF16))  # out shape
    ok = _hip().gemm_skinny_ok
    assert ok(1, 1, 8, 2) and ok(16, 50257, 1600, 2)
    assert not ok(17, 32, 64, 2) and not ok(0, 32, 64, 2) and not ok(4, 32, 12, 2) and not ok(4, 32, 64, 4)
    assert not ok(4, 1 << 30, 64, 2) and not ok(4, 32, 1 << 30, 2)


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        x = torch.empty(3, 64, device=DEV, dtype=BF16)
        w = torch.empty(50257, 64, device=DEV, dtype=BF16)
        out = torch.empty(3, 50257, device=DEV, dtype=BF16)
        assert torch.ops.cs336.gemm_skinny(x, w, out) is None
        y = gemm.skinny_mm(x, w)
        assert y.shape == (3, 50257) and y.dtype == BF16
