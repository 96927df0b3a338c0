"""The weight-only FP8 / MXFP4 tile GEMM above 128 rows (``csrc/gemm/gemm_wqt.hip``, ``cs336::gemm_wqt_w8`` /
``gemm_wqt_w4``) against an fp64 oracle, with the comparison rule of ``test_kernel_edges_gpu.py`` (``check``,
``k = 4``) and the references and inputs of ``test_skinny_w8_gpu.py`` / ``test_skinny_w4_gpu.py``, as
``test_gemm_wq_gpu.py`` uses them: the conversion in the kernel is exact, so no case has a margin of its own.

Shapes follow the plan as committed (``csrc/gemm/gemm_wqt_plan.h``): tiles (128, 128), (128, 64), (64, 64),
k-tile 64, K split 2 / 4 / 8 ways on the (64, 64) tile. ``PATHS`` reaches every (BM, BN, splits) the plan
returns with a short K and a long one with a tail, and asserts the plan, so a changed plan fails here rather
than leaving a kernel untested."""

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
BM, BN, KT = 128, 128, 64  # the largest tile; the smaller ones are 64 rows / columns
KL = {"w8": 16, "w4": 32}
MOD = {"w8": t8, "w4": t4}
FMT_DT = [(f, dt) for f in ("w8", "w4") for dt in (BF16, F16)]
# (M, N, K) -> (BM, BN, splits); K 928 and 1632 / 3232 end in half a k-tile
PATHS = {
    (129, 50257, 64): (128, 128, 1), (129, 16400, 1632): (128, 128, 1),
    (129, 10000, 64): (128, 64, 1), (129, 8200, 1632): (128, 64, 1),
    (129, 48, 64): (64, 64, 1), (129, 6400, 1632): (64, 64, 1),
    (129, 48, 512): (64, 64, 2), (129, 48, 928): (64, 64, 2),
    (129, 48, 1024): (64, 64, 4), (129, 1600, 1632): (64, 64, 4),
    (129, 48, 2048): (64, 64, 8), (129, 48, 3232): (64, 64, 8),
}


def _run(fmt, x, wq, s, out=None):
    out = torch.empty(x.shape[0], wq.shape[0], device=DEV, dtype=x.dtype) if out is None else out
    getattr(_ext.ops(), "gemm_wqt_" + fmt)(x, wq, s, out)
    return out


def _check(fmt, x, wq, s, got, tag):
    ref64, ref32 = MOD[fmt]._refs(x, wq, s)
    r = check(got, ref64, ref32, x.dtype, f"gemm_wqt_{fmt}.{tag}", k=4)
    print(f"gemm_wqt_{fmt}.{tag} M {x.shape[0]} N {wq.shape[0]} K {x.shape[1]} {x.dtype}: ratio {r:.3f}")


@pytest.mark.parametrize("M,N", [(M, 48) for M in (129, BM // 2 * 3 + 1, 2 * BM, 2 * BM + 1)]
                         + [(129, N) for N in (1, BN // 2 - 1, BN // 2 + 1, BN - 1, BN + 1)])
@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_boundaries(fmt, dt, M, N):
    kl = KL[fmt]
    for K in sorted({kl, KT - kl, KT, KT + kl, 1600, 1600 + kl}):
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt)
        _check(fmt, x, wq, s, _run(fmt, x, wq, s), "edges")


@pytest.mark.parametrize("shape", PATHS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_plan_paths(fmt, dt, shape):
    assert tuple(_ext.ops().gemm_wqt_plan(fmt == "w4", *shape)) == PATHS[shape]
    x, wq, s = MOD[fmt]._inputs(*shape, dt)
    _check(fmt, x, wq, s, _run(fmt, x, wq, s), "paths")


@pytest.mark.parametrize("M,N,K", [(129, 17, 1632), (193, 50, 96), (257, 130, 1600)])
@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_views_and_poison(fmt, dt, M, N, K):
    """x is every other row of a NaN buffer, wq / scale sit in buffers of 0xFF bytes / NaN, out is a slice
    of a NaN buffer: a row >= M or >= N, a k >= K or a scale outside its tensor that reached a stored value,
    or a store outside out, shows without any fault. (129, 17, 1632) is a split-K launch."""
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
    for K in (96, 928, 1632, 3232):  # 1, 2, 4 and 8 splits
        x, wq, s = MOD[fmt]._inputs(129, 48, K, dt, seed=2)
        assert torch.equal(_run(fmt, x, wq, s), _run(fmt, x, wq, s))


@pytest.mark.parametrize("fmt,dt", FMT_DT)
def test_routing(fmt, dt):
    linear = ops.skinny_linear_fp8 if fmt == "w8" else ops.skinny_linear_mxfp4
    ok = gemm.wqt_w8_ok if fmt == "w8" else gemm.wqt_w4_ok
    assert gemm.WQT_MIN_M == 129
    # the measured FP8 exception (long K, short N at 512 rows and more) and nothing else stays on the old path
    assert gemm.wqt_routed(fmt, 512, 1600, 6400) == (fmt == "w4") and gemm.wqt_routed(fmt, 511, 1600, 6400)
    N, K = 512, 1632
    for M in (129, 300):
        x, wq, s = MOD[fmt]._inputs(M, N, K, dt)
        assert ok(x, wq, s) and gemm.wqt_routed(fmt, M, N, K)
        assert torch.equal(linear(x.view(M, 1, K), wq, s), _run(fmt, x, wq, s).view(M, 1, N))
    out = torch.empty(128, N, device=DEV, dtype=dt)
    getattr(_ext.ops(), "gemm_wq_" + fmt)(x[:128], wq, s, out)
    assert not ok(x[:128], wq, s) and torch.equal(linear(x[:128], wq, s), out)

    def raises(x, wq, s):
        assert not ok(x, wq, s)
        with pytest.raises(RuntimeError):
            _run(fmt, x, wq, s)

    raises(x[:128], wq, s)
    raises(x.float(), wq, s)
    k = K - KL[fmt] // 2  # K % 16 / K % 32 != 0
    raises(x[:, :k].contiguous(), wq[:, :k // (2 if fmt == "w4" else 1)].contiguous(), s if fmt == "w8" else s[:, :k // 32])
    xb = torch.zeros(300, K + 8, device=DEV, dtype=dt)
    raises(xb[:, 4:4 + K], wq, s)  # rows start 8 bytes off a 16-byte boundary


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        x = torch.empty(200, 128, device=DEV, dtype=BF16)
        out = torch.empty(200, 500, device=DEV, dtype=BF16)
        w8, s8 = torch.empty(500, 128, device=DEV, dtype=torch.float8_e4m3fn), torch.empty(500, device=DEV)
        w4, s4 = torch.empty(500, 64, device=DEV, dtype=U8), torch.empty(500, 4, device=DEV, dtype=U8)
        assert torch.ops.cs336.gemm_wqt_w8(x, w8, s8, out) is None and torch.ops.cs336.gemm_wqt_w4(x, w4, s4, out) is None
        for y in (gemm.wqt_w8_mm(x, w8, s8), gemm.wqt_w4_mm(x, w4, s4)):
            assert y.shape == (200, 500) and y.dtype == BF16


def test_mxfp4_verify_graph_above_128_rows():
    """B 9 x 16 tokens = 144 rows per projection: the captured verify step on MXFP4 weights equals the eager
    one over three replays."""
    B, n = 9, 16
    m = g8._model(256, 4, seed=5)
    q4 = Mxfp4DecodeWeights(m)
    seq = torch.randint(0, 500, (B, 8 + 3 * n), device=DEV)
    cg, ce = KVCache(m, B), KVCache(m, B)
    with torch.no_grad():
        for c in (cg, ce):
            m.forward_cached(seq[:, :8], c, weights=q4)
        dg = DecodeGraph(m, cg, tokens=n, verify=True, weights=q4)
        de = DecodeGraph(m, ce, capture=False, tokens=n, verify=True, weights=q4)
        for t in range(8, 8 + 3 * n, n):
            got, want = dg.step(seq[:, t:t + n]), de.step(seq[:, t:t + n])
            assert got.shape == (B, n, 500) and torch.isfinite(got).all() and torch.equal(got, want), t


@pytest.mark.parametrize("cls,mm", [(Fp8DecodeWeights, "wqt_w8_mm"), (Mxfp4DecodeWeights, "wqt_w4_mm")])
def test_model_prefill_and_generate(cls, mm):
    """2 x 80 prompt tokens = 160 rows per projection on the small model of ``test_decode_graph_fp8_gpu.py``:
    every projection of the prefill runs the new op and the logits meet that file's bound (2 e_hip + ulp)
    against the fp32 forward of the dequantized weights; ``generate(quantized_prefill=True)`` emits the tokens
    of the same ops run by hand."""
    from unittest import mock

    d_model, heads, B, P, new = 256, 4, 2, 80, 6
    m = g8._model(d_model, heads, seed=5)
    qw = cls(m)
    seq = torch.randint(0, 500, (B, P), device=DEV)
    m32 = BasicsTransformerLM(**g8._cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref16 = m32(seq).double()
    with torch.no_grad():
        e_hip = (m(seq).double() - ref16).abs().max().item()
    m32.load_state_dict(qw.dequantized_state_dict(torch.float32))
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()
    cache = KVCache(m, B)
    with mock.patch.object(gemm, mm, wraps=getattr(gemm, mm)) as op:
        logits = m.forward_cached(seq, cache, weights=qw)
        assert op.call_count == 4 * 2 + 1
    e = (logits.double() - ref).abs().max().item()
    ulp = g8._ulp(BF16, ref.abs().max().item())
    print(f"{cls.__name__}: e_hip {e_hip:.4e} e_prefill {e:.4e} ulp {ulp:.3e}")
    assert e <= 2 * e_hip + ulp, (e, e_hip, ulp)

    torch.manual_seed(7)  # generate's own sampling at top_k=1 draws from the generator (ties)
    toks = [g8._sample_top1(logits)]
    with torch.no_grad():
        dg = DecodeGraph(m, cache, weights=qw)
        for _ in range(new - 1):
            toks.append(g8._sample_top1(dg.step(toks[-1])))
    torch.manual_seed(7)
    got = m.generate(seq, new, top_k=1, use_cache=True, graph=True, weights=qw, quantized_prefill=True)
    assert torch.equal(got, torch.cat(toks, dim=1))
