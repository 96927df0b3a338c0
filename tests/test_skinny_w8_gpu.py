"""The FP8 weight-only skinny-M GEMM kernel (the e4m3 weight format of ``csrc/gemm/gemm_skinny.hip``,
``cs336::gemm_skinny_w8``)
against an fp64 oracle, with the one comparison rule of ``test_kernel_edges_gpu.py`` (``check``, ``k = 4``):
``ref64 = (x.double() @ wq.double().T) * scale.double()`` and the same in plain fp32. Both come from
the QUANTIZED operands, so the quantization error is not in the comparison; against the 16-bit kernel
the only differences are an exact conversion and one fp32 multiply, so no case has a margin of its own.

Inputs: ``x`` randn in bf16 / fp16; ``wq, scale = quantize_fp8_rows(randn rows * 2^e)`` with a per-row
``e`` in -6 .. 6.

Shapes: M 1 / 3 / 16 (one row, a partial and a full MFMA tile of batch rows); N 1 / 15 / 16 / 17 / 48
(below, at and above one 16-row W tile; several workgroups) and the vocabulary head's 50257 (not a
multiple of 4: scalar stores); K 16 (a single 16-B W load), 48 (not a multiple of the 64-k block), 64
(one block), 1600 (a multiple), 1616 (a tail). ``PATHS``: the plan keeps the 16-bit kernel's N
thresholds (2 / 4 tiles per wave from 256 / 512 tiles), so the shapes are those of
``test_skinny_gemm_gpu.py`` with K moved to multiples of 16: (48, 8240) gives all 8 waves of a workgroup
several register sets (16 sets of 512 k and a 48-k tail), the others reach the 2- and 4-tile kernels
with a short and a long K.

Measured ``max (|got - ref64| - u*|ref64|) / E32`` on an MI355X per group: small 0.000, vocab 0.010,
paths 0.237, views 0.000, poisoned 0.001, fallback 0.000 (0: the error stayed within the one rounding to
the output type). The rule's ``k = 4`` holds everywhere and no case has a margin of its own.

The fallback group includes 17 rows, which ``ops.skinny_linear_fp8`` runs through the existing GEMM with
an fp32 result. With that GEMM's 16-bit result and the scale applied afterwards (two roundings) 27 of
544 elements missed the rule, by up to a whole bf16 ulp (ratio 3955): the reason the path rounds once."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext, gemm

from .test_kernel_edges_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
MS = (1, 3, 16)
NS = (1, 15, 16, 17, 48)
KS = (16, 48, 64, 1600, 1616)
PATHS = [(48, 8240), (4100, 1616), (4100, 4112), (8200, 1616), (8200, 4112)]


def _hip():
    return _ext.ops()


def _inputs(M, N, K, dt, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    e = torch.randint(-6, 7, (N, 1), device=DEV, generator=g)
    wq, scale = ops.quantize_fp8_rows(torch.randn(N, K, device=DEV, generator=g) * torch.exp2(e.float()))
    return x, wq, scale


def _refs(x, wq, scale):
    return (x.double() @ wq.double().t()) * scale.double(), (x.float() @ wq.float().t()) * scale


def _run(x, wq, scale, out=None):
    out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
    _hip().gemm_skinny_w8(x, wq, scale, out)
    return out


def _check(x, wq, scale, got, tag):
    ref64, ref32 = _refs(x, wq, scale)
    r = check(got, ref64, ref32, x.dtype, f"gemm_skinny_w8.{tag}")
    print(f"gemm_skinny_w8.{tag} M {x.shape[0]} N {wq.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_small_shapes(dt, K):
    for M in MS:
        for N in NS:
            x, wq, s = _inputs(M, N, K, dt)
            _check(x, wq, s, _run(x, wq, s), "small")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_vocabulary_head(dt):
    for M in MS:
        x, wq, s = _inputs(M, 50257, 64, dt)
        _check(x, wq, s, _run(x, wq, s), "vocab")


@pytest.mark.parametrize("N,K", PATHS)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_dispatch_paths(dt, N, K):
    for M in (3, 16):
        x, wq, s = _inputs(M, N, K, dt)
        _check(x, wq, s, _run(x, wq, s), "paths")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_views(dt):
    M, N, K = 3, 48, 1616
    x, wq, s = _inputs(M, N, K, dt)
    ref = _run(x, wq, s)
    xb = torch.zeros(2 * M, K, device=DEV, dtype=dt)
    xb[::2] = x
    wg = torch.full((3 * N, K), 0x38, device=DEV, dtype=torch.uint8)  # the grouped QKV layout (0x38 is 1.0)
    wg[N:2 * N] = wq.view(torch.uint8)
    wg = wg.view(F8)
    sg = torch.ones(3 * N, device=DEV)
    sg[N:2 * N] = s
    ob = torch.zeros(M, N + 16, device=DEV, dtype=dt)
    out = ob[:, 4:4 + N]  # 8 bytes into a row: the 4-column stores
    assert out.data_ptr() % 16 == 8
    _run(xb[::2], wg[N:2 * N], sg[N:2 * N], out)
    assert torch.equal(out, ref)
    assert not ob[:, :4].any() and not ob[:, 4 + N:].any()
    _check(x, wq, s, out, "views")
    # an odd column offset: out rows are not 8-B aligned, the kernel stores element by element
    ob.zero_()
    out = ob[:, 3:3 + N]
    _run(x, wq, s, out)
    assert torch.equal(out, ref)
    assert not ob[:, :3].any() and not ob[:, 3 + N:].any()
    # the uint8 view of wq and ops.skinny_linear_fp8 (leading dims restored) give the same bits
    assert torch.equal(_run(x, wq.view(torch.uint8), s), ref)
    assert torch.equal(ops.skinny_linear_fp8(x.view(M, 1, K), wq, s), ref.view(M, 1, N))


@pytest.mark.parametrize("dt,M,N,K", [(BF16, 3, 17, 1616), (F16, 16, 50257, 64)])
def test_nan_poisoning(dt, M, N, K):
    """All operands are cut out of larger poisoned buffers (NaN; byte 0x7f, the e4m3 NaN, around ``wq``):
    a W row >= N, a batch row >= M, a scale >= N or a k >= K that leaked into a stored value, or a
    store outside ``out``, shows without any fault."""
    x, wq, s = _inputs(M, N, K, dt, seed=1)
    nan = float("nan")
    xb = torch.full((M + 2, K + 16), nan, device=DEV, dtype=dt)
    wb = torch.full((N + 2, K + 32), 0x7F, device=DEV, dtype=torch.uint8)
    sb = torch.full((N + 2,), nan, device=DEV)
    ob = torch.full((M + 2, N + 16), nan, device=DEV, dtype=dt)
    xb[1:M + 1, 8:8 + K] = x
    wb[1:N + 1, 16:16 + K] = wq.view(torch.uint8)
    wb = wb.view(F8)
    sb[1:N + 1] = s
    before = ob.clone().view(torch.int16)
    out = ob[1:M + 1, 4:4 + N]
    _run(xb[1:M + 1, 8:8 + K], wb[1:N + 1, 16:16 + K], sb[1:N + 1], out)
    assert torch.isfinite(out).all()
    _check(x, wq, s, out, "poisoned")
    after = ob.view(torch.int16).clone()
    after[1:M + 1, 4:4 + N] = before[1:M + 1, 4:4 + N]
    assert torch.equal(after, before)  # the bytes around out are untouched


@pytest.mark.parametrize("dt", [BF16, F16])
def test_bitwise_reproducible(dt):
    for M, N, K in [(16, 48, 8240), (3, 8200, 1616), (1, 50257, 64)]:
        x, wq, s = _inputs(M, N, K, dt, seed=2)
        assert torch.equal(_run(x, wq, s), _run(x, wq, s))


def test_unsupported_inputs_raise_and_skinny_linear_fp8_falls_back():
    def raises(x, wq, s, out=None):
        out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
        with pytest.raises(RuntimeError):
            _hip().gemm_skinny_w8(x, wq, s, out)

    def falls_back(x, wq, s):
        got = ops.skinny_linear_fp8(x, wq, s)
        assert got.dtype == x.dtype and got.shape == (x.shape[0], wq.shape[0])
        if x.dtype in (BF16, F16):
            ref64, ref32 = _refs(x, wq, s)
            r = check(got, ref64, ref32, x.dtype, "gemm_skinny_w8.fallback")
            print(f"gemm_skinny_w8.fallback M {x.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")
        else:
            assert torch.equal(got, ops.skinny_linear_fp8_ref(x, wq, s))

    x, wq, s = _inputs(17, 32, 64, BF16)  # M = 17: the existing GEMM on the converted weight, then the scale
    raises(x, wq, s)
    falls_back(x, wq, s)
    x, wq, s = _inputs(4, 32, 24, BF16)  # K % 16 != 0
    raises(x, wq, s)
    falls_back(x, wq, s)
    x, wq, s = _inputs(4, 32, 64, BF16)
    raises(x.float(), wq, s)  # fp32 x
    falls_back(x.float(), wq, s)
    raises(x, wq, s, torch.empty(4, 32, device=DEV, dtype=F16))  # x / out dtype mismatch
    raises(x, wq, s[:31])  # scale of the wrong length
    raises(x, wq, s.double())  # ... or dtype
    raises(x, wq, torch.ones(64, device=DEV)[::2])  # ... or not contiguous
    raises(x, wq.to(BF16), s)  # wq must be e4m3 (or its uint8 view)
    raises(x, wq, s, torch.empty(4, 31, device=DEV, dtype=BF16))  # out shape
    xb = torch.zeros(4, 72, device=DEV, dtype=BF16)
    xm = xb[:, 4:68]  # rows start 8 bytes off a 16-byte boundary
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 8
    raises(xm, wq, s)
    falls_back(xm, wq, s)
    ok = _hip().gemm_skinny_w8_ok
    assert ok(1, 1, 16, 2) and ok(16, 50257, 1600, 2)
    assert not ok(17, 32, 64, 2) and not ok(0, 32, 64, 2) and not ok(4, 32, 24, 2) and not ok(4, 32, 8, 2)
    assert not ok(4, 32, 64, 4) and not ok(4, 1 << 30, 64, 2) and not ok(4, 32, 1 << 30, 2)


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        x = torch.empty(3, 64, device=DEV, dtype=BF16)
        wq = torch.empty(50257, 64, device=DEV, dtype=F8)
        s = torch.empty(50257, device=DEV, dtype=torch.float32)
        out = torch.empty(3, 50257, device=DEV, dtype=BF16)
        assert torch.ops.cs336.gemm_skinny_w8(x, wq, s, out) is None
        y = gemm.skinny_w8_mm(x, wq, s)
        assert y.shape == (3, 50257) and y.dtype == BF16
