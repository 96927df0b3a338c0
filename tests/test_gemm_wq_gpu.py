"""The weight-only FP8 / MXFP4 GEMM for 17..128 rows (``csrc/gemm/gemm_wq.hip``, ``cs336::gemm_wq_w8`` /
``gemm_wq_w4``) against an fp64 oracle, with the one comparison rule of ``test_kernel_edges_gpu.py``
(``check``, ``k = 4``). References and inputs are those of ``test_skinny_w8_gpu.py`` /
``test_skinny_w4_gpu.py``: ``ref64`` and ``ref32`` come from the DEQUANTIZED operands (the conversion in the
kernel is exact, so no case has a margin of its own); ``x`` randn, W rows randn times 2^e, e in -6 .. 6.

Shapes follow the plan as committed (``csrc/gemm/gemm_wq_plan.h``). ``SLAB[fmt][MB]`` is the k of one x slab;
``PATHS`` reaches every ``(RW, KG, TN)`` the plan returns, each with a short K and a long one with a tail
where the plan has both, and every (MB, tiles per workgroup) kernel at least once; the test asserts the plan
it expects, so a changed plan fails here rather than silently leaving a kernel untested. Contiguous ``wq``
from the quantizer is the case whose last row ends where its allocation's data ends."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, Mxfp4DecodeWeights
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import _ext, gemm

from . import test_decode_graph_fp8_gpu as g8
from . import test_skinny_w4_gpu as t4
from . import test_skinny_w8_gpu as t8
from .test_kernel_edges_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, U8 = torch.bfloat16, torch.float16, torch.uint8
KL = {"w8": 16, "w4": 32}
SLAB = {"w8": {2: 256, 4: 128, 8: 64}, "w4": {2: 256, 4: 128, 8: 128}}
WG_ROWS_M33 = {"w8": 32, "w4": 64}  # rows per workgroup at M 33 and small N
MOD = {"w8": t8, "w4": t4}
FMT_DT = [(f, dt) for f in ("w8", "w4") for dt in (BF16, F16)]
# (M, N, K) -> (RW, KG, TN)
PATHS = {
    "w8": {(17, 48, 256): (1, 1, 1), (17, 48, 1616): (1, 2, 1), (64, 100, 128): (2, 1, 1), (64, 100, 1616): (2, 2, 1),
           (128, 100, 64): (2, 1, 2), (128, 100, 1616): (2, 2, 2), (128, 65536, 64): (4, 1, 2), (128, 65536, 272): (4, 2, 2),
           (32, 16400, 272): (2, 1, 1), (32, 32800, 272): (2, 1, 2), (32, 65536, 272): (4, 1, 2), (64, 32800, 272): (2, 1, 2),
           (64, 65536, 272): (4, 1, 2)},
    "w4": {(17, 48, 256): (2, 1, 1), (17, 48, 1632): (2, 2, 1), (64, 100, 128): (2, 1, 2), (64, 100, 1632): (2, 2, 2),
           (128, 100, 128): (4, 1, 2), (128, 100, 1632): (4, 1, 2), (64, 65536, 128): (4, 1, 2), (64, 65536, 544): (4, 2, 2),
           (32, 32800, 288): (2, 1, 2), (32, 65536, 288): (4, 1, 2)},
}


def _mb(M):
    return 2 if M <= 32 else (4 if M <= 64 else 8)


def _run(fmt, x, wq, s, out=None):
    out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
    getattr(_ext.ops(), "gemm_wq_" + fmt)(x, wq, s, out)
    return out


def _check(fmt, x, wq, s, got, tag):
    ref64, ref32 = MOD[fmt]._refs(x, wq, s)
    r = check(got, ref64, ref32, x.dtype, f"gemm_wq_{fmt}.{tag}", k=4)
    print(f"gemm_wq_{fmt}.{tag} M {x.shape[0]} N {wq.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")


def _ks(fmt, M):
    kl, ks = KL[fmt], SLAB[fmt][_mb(M)]
    return sorted({kl, ks - kl, ks, ks + kl, 1600, 1600 + kl})


@pytest.mark.parametrize("M,N", [(M, 48) for M in (17, 32, 33, 64, 65, 128)] + [(33, N) for N in (1, 15, 17, None)])
@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_boundaries(fmt, dt, M, N):
    N = WG_ROWS_M33[fmt] + 1 if N is None else N
    for K in _ks(fmt, M):
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt)
        _check(fmt, x, wq, s, _run(fmt, x, wq, s), "edges")


@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_plan_paths(fmt, dt):
    for (M, N, K), want in PATHS[fmt].items():
        assert tuple(_ext.ops().gemm_wq_plan(fmt == "w4", M, N, K)) == want, (M, N, K)
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt)
        _check(fmt, x, wq, s, _run(fmt, x, wq, s), "paths")
    reached = set(PATHS[fmt].values())
    every = {(1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1), (2, 1, 2), (2, 2, 2), (4, 1, 2), (4, 2, 2)}
    assert reached == (every if fmt == "w8" else every - {(1, 1, 1), (1, 2, 1)})


@pytest.mark.parametrize("M,N,K", [(17, 17, 1616 + 16), (65, 50, 96), (128, 33, 1600)])
@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_views_and_poison(fmt, dt, M, N, K):
    """x is every other row of a NaN buffer, wq / scale sit in buffers of 0xFF bytes / NaN, out is a slice
    of a NaN buffer: a row >= M or >= N, a k >= K or a scale outside its tensor that reached a stored value,
    or a store outside out, shows without any fault."""
    x, wq, s = MOD[fmt]._inputs(M, N, K, dt, seed=1)
    nan, kb = float("nan"), wq.shape[1]
    xb = torch.full((2 * M + 2, K + 16), nan, device=DEV, dtype=dt)
    xv = xb[1:2 * M + 1:2, 8:8 + K]
    xv.copy_(x)
    wb = torch.full((N + 2, kb + 32), 0xFF, device=DEV, dtype=U8)
    wv = wb[1:N + 1, 16:16 + kb]
    wv.copy_(wq.view(U8))
    if fmt == "w8":
        sb = torch.full((N + 8,), nan, device=DEV)
        sv = sb[4:4 + N]
        wv = wv.view(torch.float8_e4m3fn)
    else:
        sb = torch.full((N + 2, K // 32 + 7), 0xFF, device=DEV, dtype=U8)
        sv = sb[1:N + 1, 3:3 + K // 32]
    sv.copy_(s)
    ob = torch.full((M + 2, N + 16), nan, device=DEV, dtype=dt)
    before = ob.clone().view(torch.int16)
    out = ob[1:M + 1, 4:4 + N]
    _run(fmt, xv, wv, sv, out)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _run(fmt, x, wq, s))
    _check(fmt, x, wq, s, out, "poisoned")
    after = ob.view(torch.int16).clone()
    after[1:M + 1, 4:4 + N] = before[1:M + 1, 4:4 + N]
    assert torch.equal(after, before)  # the bytes around out are untouched


@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_bitwise_reproducible(fmt, dt):
    for M, N, K in [(32, 100, 1632), (64, 100, 1632), (128, 100, 1632)]:
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt, seed=2)
        assert torch.equal(_run(fmt, x, wq, s), _run(fmt, x, wq, s))


@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_routing(fmt, dt):
    linear = ops.skinny_linear_fp8 if fmt == "w8" else ops.skinny_linear_mxfp4
    ok = gemm.wq_w8_ok if fmt == "w8" else gemm.wq_w4_ok
    N, K = 512, 1632  # K < 4 N: not the long-K, short-N exception of gemm.wq_w8_routed
    for M in (17, 128):
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt)
        assert ok(x, wq, s)
        assert torch.equal(linear(x.view(M, 1, K), wq, s), _run(fmt, x, wq, s).view(M, 1, N))
    x, wq, s = MOD[fmt]._inputs(129, N, K, dt)
    assert not ok(x, wq, s)
    _check(fmt, x, wq, s, linear(x, wq, s), "fallback")

    def raises(x, wq, s):
        assert not ok(x, wq, s)
        with pytest.raises(RuntimeError):
            _run(fmt, x, wq, s)

    raises(x, wq, s)  # M 129
    raises(x[:16], wq, s)  # M 16: the skinny kernel's
    raises(x[:20].float(), wq, s)
    k = K - KL[fmt] // 2  # K % 16 / K % 32 != 0
    raises(x[:20, :k].contiguous(), wq[:, :k // (2 if fmt == "w4" else 1)].contiguous(), s if fmt == "w8" else s[:, :k // 32])
    xb = torch.zeros(20, K + 8, device=DEV, dtype=dt)
    raises(xb[:, 4:4 + K], wq, s)  # rows start 8 bytes off a 16-byte boundary
    fn = _ext.ops().gemm_skinny_w8_ok if fmt == "w8" else _ext.ops().gemm_skinny_w4_ok
    assert fn(16, N, K, 2) and not fn(17, N, K, 2)


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        x = torch.empty(40, 128, device=DEV, dtype=BF16)
        out = torch.empty(40, 500, device=DEV, dtype=BF16)
        w8, s8 = torch.empty(500, 128, device=DEV, dtype=torch.float8_e4m3fn), torch.empty(500, device=DEV)
        w4, s4 = torch.empty(500, 64, device=DEV, dtype=U8), torch.empty(500, 4, device=DEV, dtype=U8)
        assert torch.ops.cs336.gemm_wq_w8(x, w8, s8, out) is None and torch.ops.cs336.gemm_wq_w4(x, w4, s4, out) is None
        for y in (gemm.wq_w8_mm(x, w8, s8), gemm.wq_w4_mm(x, w4, s4)):
            assert y.shape == (40, 500) and y.dtype == BF16


@pytest.mark.parametrize("cls,mm", [(Fp8DecodeWeights, "wq_w8_mm"), (Mxfp4DecodeWeights, "wq_w4_mm")])
def test_model_chunk_step(cls, mm):
    """B 8 x 4 tokens = 32 rows per projection on the small model of ``test_decode_graph_fp8_gpu.py``: the
    captured step equals the eager one over three replays, every projection runs the new op, and the logits
    meet that file's bound (2 e_hip + ulp) against the fp32 forward of the dequantized weights."""
    from unittest import mock

    d_model, heads, B, n = 256, 4, 8, 4
    m = g8._model(d_model, heads, seed=5)
    qw = cls(m)
    seq = torch.randint(0, 500, (B, 8 + 3 * n), device=DEV)
    m32 = BasicsTransformerLM(**g8._cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref16 = m32(seq).double()[:, 8:]
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 8:] - ref16).abs().max().item()
    m32.load_state_dict(qw.dequantized_state_dict(torch.float32))
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]
    cg, ce = KVCache(m, B), KVCache(m, B)
    with torch.no_grad(), gemm.skinny_decode(weights=qw):
        for c in (cg, ce):
            m.forward_cached(seq[:, :8], c)
    rows = []
    with torch.no_grad(), mock.patch.object(gemm, mm, wraps=getattr(gemm, mm)) as op:
        dg = DecodeGraph(m, cg, tokens=n, weights=qw)
        de = DecodeGraph(m, ce, capture=False, tokens=n, weights=qw)
        assert op.call_count == 3 * (4 * 2 + 1)  # two warm-up steps and the captured one
        for t in range(8, 8 + 3 * n, n):
            got, want = dg.step(seq[:, t:t + n]), de.step(seq[:, t:t + n])
            assert got.shape == (B, n, 500) and torch.equal(got, want), t
            rows.append(got.clone())
    e_graph = (torch.cat(rows, dim=1).double() - ref).abs().max().item()
    ulp = g8._ulp(BF16, ref.abs().max().item())
    print(f"{cls.__name__}: e_hip {e_hip:.4e} e_step {e_graph:.4e} ulp {ulp:.3e}")
    assert e_graph <= 2 * e_hip + ulp, (e_graph, e_hip, ulp)
