"""The MXFP4 weight-only skinny-M GEMM kernel (``csrc/gemm/gemm_skinny_w4.hip``, ``cs336::gemm_skinny_w4``)
against an fp64 oracle, with the one comparison rule of ``test_kernel_edges_gpu.py`` (``check``, ``k = 4``):
``ref64 = x.double() @ dq.double().T`` and the same in plain fp32, ``dq = dequantize_mxfp4_rows(wq, scale)``.
Both come from the DEQUANTIZED operands, so the quantization error is not in the comparison; against the
16-bit kernel the only difference is an exact conversion, so no case has a margin of its own.

Inputs: ``x`` randn in bf16 / fp16; ``wq, scale = quantize_mxfp4_rows(randn rows * 2^e)`` with a per-row ``e``
in -6 .. 6.

Shapes: M 1 / 3 / 16 (one row, a partial and a full MFMA tile of batch rows); N 1 / 15 / 16 / 17 / 48 (below,
at and above one 16-row W tile; several workgroups) and the vocabulary head's 50257 (not a multiple of 4:
scalar stores); K 32 (a single 16-B W load), 96 (below the 128-k block), 128 (one block), 1600 (a tail of 64),
1632 (a tail of 96). ``PATHS``, from the plan as it is (``csrc/gemm/skinny_plan.h``: 1 / 2 / 4 W tiles per wave
below 256 / from 256 / from 512 tiles, a register set of 4 / 2 / 2 k-blocks of 128 k): (48, 8288) gives all 8
waves of a 1-tile workgroup two register sets each (16 sets of 512 k) and a 96-k tail; (4100, .) and (8200, .)
reach the 2- and 4-tile kernels with a short K (1632: 6 sets of 256 k, 6 and 4 waves, a tail) and a long one
(4128: 16 sets, 8 and 4 waves, a 32-k tail).

``test_the_map_bit_for_bit`` is the check that the hardware conversion means what the format says: one-hot
``x`` rows read single weights out of the kernel, which must equal ``dequantize_mxfp4_rows`` exactly for every
code, under scale exponents -23 .. 13, at every k of a 128-k block -- nibble order, byte selects, the
k-to-lane map and the scale-to-block map.

Measured ``max (|got - ref64| - u*|ref64|) / E32`` on an MI355X per group: small 0.000, vocab 0.016, paths
0.068, views 0.000, poisoned 0.002, fallback 0.000 (0: the error stayed within the one rounding to the output
type). The rule's ``k = 4`` holds everywhere and no case has a margin of its own; the one-hot map came out
exact in bf16 and in fp16, subnormal fp16 products (down to 2^-24) included."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext, gemm

from .test_kernel_edges_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, U8 = torch.bfloat16, torch.float16, torch.uint8
MS = (1, 3, 16)
NS = (1, 15, 16, 17, 48)
KS = (32, 96, 128, 1600, 1632)
PATHS = [(48, 8288), (4100, 1632), (4100, 4128), (8200, 1632), (8200, 4128)]


def _hip():
    return _ext.ops()


def _inputs(M, N, K, dt, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    e = torch.randint(-6, 7, (N, 1), device=DEV, generator=g)
    wq, scale = ops.quantize_mxfp4_rows(torch.randn(N, K, device=DEV, generator=g) * torch.exp2(e.float()))
    return x, wq, scale


def _refs(x, wq, scale):
    return (x.double() @ ops.dequantize_mxfp4_rows(wq, scale, torch.float64).t(),
            x.float() @ ops.dequantize_mxfp4_rows(wq, scale, torch.float32).t())


def _run(x, wq, scale, out=None):
    out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
    _hip().gemm_skinny_w4(x, wq, scale, out)
    return out


def _check(x, wq, scale, got, tag):
    ref64, ref32 = _refs(x, wq, scale)
    r = check(got, ref64, ref32, x.dtype, f"gemm_skinny_w4.{tag}", k=4)
    print(f"gemm_skinny_w4.{tag} M {x.shape[0]} N {wq.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")


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
        x, wq, s = _inputs(M, 50257, 128, dt)
        _check(x, wq, s, _run(x, wq, s), "vocab")


@pytest.mark.parametrize("N,K", PATHS)
@pytest.mark.parametrize("dt", [BF16, F16])
def test_dispatch_paths(dt, N, K):
    for M in (3, 16):
        x, wq, s = _inputs(M, N, K, dt)
        _check(x, wq, s, _run(x, wq, s), "paths")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_the_map_bit_for_bit(dt):
    N, K = 17, 128
    g = torch.Generator(device=DEV).manual_seed(11)
    codes = torch.randint(0, 16, (N, K), device=DEV, generator=g).to(U8)
    codes[0, :16] = torch.arange(16, device=DEV, dtype=U8)  # every code is there whatever the draw
    codes[16, 112:] = torch.arange(16, device=DEV, dtype=U8).flip(0)
    wq = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    # 68 blocks over the 37 scale exponents -23 .. 13, each at least once, in no order the layout could mirror
    scale = ((torch.arange(N * 4, device=DEV) * 23 + 5) % 37 + 104).to(U8).view(N, 4)
    assert set(scale.flatten().tolist()) == set(range(104, 141)) and set(codes.flatten().tolist()) == set(range(16))
    dq = ops.dequantize_mxfp4_rows(wq, scale, torch.float64)
    assert torch.equal(dq, ops.dequantize_mxfp4_rows(wq, scale, dt).double())  # exact in the activation type
    for c in range(8):  # 16 k per call: batch row i reads k = 16 c + i
        x = torch.zeros(16, K, device=DEV, dtype=dt)
        x[torch.arange(16), 16 * c + torch.arange(16)] = 1.0
        got = _run(x, wq, scale).double()
        want = dq[:, 16 * c:16 * c + 16].t()
        bad = (got != want).nonzero()
        assert not len(bad), (c, bad[:8].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@pytest.mark.parametrize("dt", [BF16, F16])
def test_views(dt):
    M, N, K = 3, 48, 1632
    x, wq, s = _inputs(M, N, K, dt)
    ref = _run(x, wq, s)
    xb = torch.zeros(2 * M, K, device=DEV, dtype=dt)
    xb[::2] = x
    wg = torch.full((3 * N, K // 2), 0x22, device=DEV, dtype=U8)  # the grouped QKV layout (code 2 is 1.0)
    wg[N:2 * N] = wq
    sg = torch.full((3 * N, K // 32), 127, device=DEV, dtype=U8)
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
    # padded scale rows (a stride of 64 for 51 bytes), at an odd offset into the row
    sp = torch.full((N, 64), 0xFF, device=DEV, dtype=U8)
    sp[:, 5:5 + K // 32] = s
    assert torch.equal(_run(x, wq, sp[:, 5:5 + K // 32]), ref)
    # the torch views of wq / scale and ops.skinny_linear_mxfp4 (leading dims restored) give the same bits
    assert torch.equal(_run(x, wq.view(torch.float4_e2m1fn_x2), s.view(torch.float8_e8m0fnu)), ref)
    assert torch.equal(ops.skinny_linear_mxfp4(x.view(M, 1, K), wq, s), ref.view(M, 1, N))


@pytest.mark.parametrize("dt,M,N,K", [(BF16, 3, 17, 1632), (F16, 16, 50257, 128)])
def test_poisoned_surroundings(dt, M, N, K):
    """All operands are cut out of larger poisoned buffers: NaN around ``x`` and ``out``, 0xFF bytes (the code
    -6 twice) around ``wq`` and 0xFF scale bytes (2^128: inf as the conversion's operand) around ``scale``, so
    that an out-of-row W byte always meets such a scale. A W row >= N, a batch row >= M, a scale row >= N, a
    block or a k >= K that leaked into a stored value, or a store outside ``out``, shows without any fault."""
    x, wq, s = _inputs(M, N, K, dt, seed=1)
    nan = float("nan")
    xb = torch.full((M + 2, K + 16), nan, device=DEV, dtype=dt)
    wb = torch.full((N + 2, K // 2 + 32), 0xFF, device=DEV, dtype=U8)
    sb = torch.full((N + 2, K // 32 + 7), 0xFF, device=DEV, dtype=U8)
    ob = torch.full((M + 2, N + 16), nan, device=DEV, dtype=dt)
    xb[1:M + 1, 8:8 + K] = x
    wb[1:N + 1, 16:16 + K // 2] = wq
    sb[1:N + 1, 3:3 + K // 32] = s
    before = ob.clone().view(torch.int16)
    out = ob[1:M + 1, 4:4 + N]
    _run(xb[1:M + 1, 8:8 + K], wb[1:N + 1, 16:16 + K // 2], sb[1:N + 1, 3:3 + K // 32], out)
    assert torch.isfinite(out).all()
    _check(x, wq, s, out, "poisoned")
    after = ob.view(torch.int16).clone()
    after[1:M + 1, 4:4 + N] = before[1:M + 1, 4:4 + N]
    assert torch.equal(after, before)  # the bytes around out are untouched


@pytest.mark.parametrize("dt", [BF16, F16])
def test_bitwise_reproducible(dt):
    for M, N, K in [(16, 48, 8288), (3, 8200, 1632), (1, 50257, 128)]:
        x, wq, s = _inputs(M, N, K, dt, seed=2)
        assert torch.equal(_run(x, wq, s), _run(x, wq, s))


def test_unsupported_inputs_raise_and_skinny_linear_mxfp4_falls_back():
    def raises(x, wq, s, out=None):
        out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
        with pytest.raises(RuntimeError):
            _hip().gemm_skinny_w4(x, wq, s, out)

    def falls_back(x, wq, s):
        got = ops.skinny_linear_mxfp4(x, wq, s)
        assert got.dtype == x.dtype and got.shape == (x.shape[0], wq.shape[0])
        if x.dtype in (BF16, F16):
            ref64, ref32 = _refs(x, wq, s)
            r = check(got, ref64, ref32, x.dtype, "gemm_skinny_w4.fallback", k=4)
            print(f"gemm_skinny_w4.fallback M {x.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")
        else:
            assert torch.equal(got, ops.skinny_linear_mxfp4_ref(x, wq, s))

    x, wq, s = _inputs(17, 32, 128, BF16)  # M = 17: the existing GEMM on the dequantized weight, fp32 result
    raises(x, wq, s)
    falls_back(x, wq, s)
    x, wq, s = _inputs(4, 32, 128, BF16)
    raises(x[:, :48].contiguous(), wq[:, :24].contiguous(), s[:, :1].contiguous())  # K = 48: K % 32 != 0
    assert not gemm.skinny_w4_ok(x[:, :48].contiguous(), wq[:, :24].contiguous(), s[:, :1].contiguous())
    raises(x.float(), wq, s)  # fp32 x
    falls_back(x.float(), wq, s)
    raises(x, wq, s, torch.empty(4, 32, device=DEV, dtype=F16))  # x / out dtype mismatch
    raises(x, wq, s[:31])  # scale of the wrong shape
    raises(x, wq, s[:, :3])
    raises(x, wq, s[:, 0])
    raises(x, wq, s.float())  # ... or dtype
    raises(x, wq, s.view(torch.float8_e4m3fn))
    raises(x, wq, torch.full((32, 8), 127, device=DEV, dtype=U8)[:, ::2])  # ... or without a contiguous last dim
    raises(x, wq.to(BF16), s)  # wq must be bytes (or float4_e2m1fn_x2)
    raises(x, wq.view(torch.float8_e4m3fn), s)
    raises(x, wq, s, torch.empty(4, 31, device=DEV, dtype=BF16))  # out shape
    xb = torch.zeros(4, 136, device=DEV, dtype=BF16)
    xm = xb[:, 4:132]  # rows start 8 bytes off a 16-byte boundary
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 8
    raises(xm, wq, s)
    falls_back(xm, wq, s)
    ok = _hip().gemm_skinny_w4_ok
    assert ok(1, 1, 32, 2) and ok(16, 50257, 1600, 2)
    assert not ok(17, 32, 128, 2) and not ok(0, 32, 128, 2) and not ok(4, 32, 48, 2) and not ok(4, 32, 16, 2)
    assert not ok(4, 32, 128, 4) and not ok(4, 1 << 30, 128, 2) and not ok(4, 32, 1 << 30, 2)


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        x = torch.empty(3, 128, device=DEV, dtype=BF16)
        wq = torch.empty(50257, 64, device=DEV, dtype=U8)
        s = torch.empty(50257, 4, device=DEV, dtype=U8)
        out = torch.empty(3, 50257, device=DEV, dtype=BF16)
        assert torch.ops.cs336.gemm_skinny_w4(x, wq, s, out) is None
        y = gemm.skinny_w4_mm(x, wq, s)
        assert y.shape == (3, 50257) and y.dtype == BF16
