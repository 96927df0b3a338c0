"""Verify attention on the FP8 KV cache (``csrc/flash_attn/fa_verify_kv8.hip``) on the GPU: the 16-query
MFMA tile over e4m3 rows with per-row scales, ``verify_cached(kv_fp8=True)`` and ``DecodeGraph(verify=True)``
on a ``KVCache(fp8=True)``.

Oracle and checks are ``test_decode_kv8_gpu.py``'s (imported): fp64 attention over ``bytes * scale`` of
each query's own key prefix, the NaN byte and NaN scales from ``kv_len[b]`` on, max |o - ref| < 2e-2 and
max |lse - ref| < 2e-2, an exact finiteness pattern of the LSE and o == 0 where lse = -inf. The bounds
carry over: K's conversion is exact and V gains one 16-bit rounding (2^-9 relative in bf16).

Measured on an MI355X: see the README paragraph on the FP8 verify kernel."""

import functools
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache

from .test_decode_kv8_gpu import B, DEV, E4M3, H, _cache, _check, _chunk_oracle, _deq64, _planes
from .test_kv_cache_fp8_gpu import _cfg, _fp32_twin, _same_cache, _ulp

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16


def _kv(kv_set, n):
    # a chunk on an empty cache; the 128-key and 32-key edges and the cache end; queries with no key at
    # all; a sequence that reaches the end of planes whose max_len is no multiple of 4
    return {"empty": ((n, n + 1, 300), 320), "edges": ((128, 160, 320), 320), "short": ((0, 3, n - 1), 320),
            "end321": ((n, 200, 321), 321)}[kv_set]


GRID = [
    (32, BF16, 1, "empty", 0), (32, F16, 5, "edges", 1), (32, BF16, 16, "short", 2), (32, F16, 17, "empty", 5),
    (32, BF16, 33, "edges", 0), (32, F16, 16, "edges", 2),
    (64, F16, 1, "edges", 5), (64, BF16, 5, "short", 0), (64, F16, 16, "empty", 1), (64, BF16, 17, "edges", 2),
    (64, F16, 33, "short", 5), (64, BF16, 16, "end321", 0),
    (80, BF16, 1, "short", 2), (80, F16, 5, "empty", 5), (80, BF16, 16, "edges", 0), (80, F16, 17, "short", 1),
    (80, BF16, 33, "empty", 2), (80, F16, 16, "end321", 5),
    (128, F16, 1, "empty", 1), (128, BF16, 5, "edges", 2), (128, F16, 16, "short", 5), (128, BF16, 17, "empty", 0),
    (128, F16, 33, "edges", 1), (128, BF16, 16, "edges", 5),
]


@functools.lru_cache(maxsize=None)
def _case(dt, d, n, kv_len, max_len, qmul=1.0):
    k8, v8, ks, vs, lens, kd, vd = _cache(d, kv_len, max_len)
    g = torch.Generator(device=DEV).manual_seed(177 + d + n)
    q = (torch.randn(B, n, H, d, device=DEV, generator=g) * qmul).to(dt)
    return (q, k8, v8, ks, vs, lens) + _chunk_oracle(q, kd, vd, kv_len, 1.0 / math.sqrt(d))


@pytest.mark.parametrize("d,dt,n,kv_set,splits", GRID)
def test_verify_attention_kv8_grid(d, dt, n, kv_set, splits):
    kv_len, max_len = _kv(kv_set, n)
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(dt, d, n, kv_len, max_len)
    o, lse = ops.verify_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} n{n} {kv_len} splits {splits}:")


def test_scale_spread_fp16():
    """V rows scaled by 2^-10 .. 2^4, neighbours in a sub-tile far apart: v_scale is applied to V, not to
    P, so the kernel is as good as the 16-bit kernel on the dequantized planes (2 * e16 + ulp)."""
    d, n, kv_len, max_len = 64, 16, (128, 160, 320), 320
    g = torch.Generator(device=DEV).manual_seed(5)
    pw = 2.0 ** ((torch.arange(max_len, device=DEV) % 15) - 10.0)
    k8, ks = _planes(torch.randn(B, H, max_len, d, device=DEV, generator=g), kv_len)
    v8, vs = _planes(torch.randn(B, H, max_len, d, device=DEV, generator=g) * pw[:, None], kv_len)
    q = torch.randn(B, n, H, d, device=DEV, generator=g).to(F16)
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    kd, vd = _deq64(k8, ks), _deq64(v8, vs)
    ref_o, ref_l = _chunk_oracle(q, kd, vd, kv_len, 1.0 / math.sqrt(d))
    o, lse = ops.verify_attention(q, k8, v8, lens, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, F16, "scale spread:")
    o16, _ = ops.verify_attention(q, kd.to(F16), vd.to(F16), lens)
    e8, e16 = ((x.double() - ref_o).abs().max().item() for x in (o, o16))
    ulp = _ulp(F16, ref_o.abs().max().item())
    print(f"scale spread fp16: e_kv8 {e8:.4e} e16 {e16:.4e} ulp {ulp:.3e}")
    assert e8 <= 2 * e16 + ulp, (e8, e16, ulp)


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("n", [5, 17])
def test_peaky(n, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(BF16, 64, n, *_kv("empty", n), 8.0)
    o, lse = ops.verify_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, BF16, f"peaky n{n} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
def test_layer_slice_and_run_to_run_bitwise(splits):
    """A layer slice of (2, B, H, max_len, d) / (2, B, H, max_len) planes is read in place and gives the
    bits of the contiguous call; two calls give the same bits."""
    q, k8, v8, ks, vs, lens, _, _ = _case(BF16, 80, 16, *_kv("edges", 16))
    o0, l0 = ops.verify_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    o1, l1 = ops.verify_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    big = [torch.full((2, *t.shape), 0x7f, device=DEV, dtype=torch.uint8).view(E4M3) for t in (k8, v8)]
    bigs = [torch.full((2, *t.shape), float("nan"), device=DEV) for t in (ks, vs)]
    for dst, src in zip(big + bigs, (k8, v8, ks, vs)):
        dst[1].copy_(src)
    o2, l2 = ops.verify_attention(q, big[0][1], big[1][1], lens, splits=splits, k_scale=bigs[0][1], v_scale=bigs[1][1])
    assert torch.equal(o2, o0) and torch.equal(l2, l0)


# ---- model ----
def _pieces(m, seq, cache, **kw):
    return torch.cat([m.verify_cached(seq[:, a:b], cache, **kw) for a, b in ((0, 5), (5, 12), (12, 28), (28, 52))], dim=1)


@pytest.mark.parametrize("d_model,heads", [(256, 4), (160, 2)])
def test_verify_cached_fp8_against_fp32(d_model, heads):
    """``e <= 2 * (e_q + e_hip) + ulp``, the rule of ``test_kv_cache_fp8_gpu.py``: ``e_q`` is what the format
    costs the fp32 model (eager backend, the same pieces over an FP8 and over a plain cache)."""
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (2, 52), device=DEV)
    m32 = _fp32_twin(m, d_model, heads)
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()
        e_q = (_pieces(m32, seq, KVCache(m32, 2, fp8=True), kv_fp8=True).double()
               - _pieces(m32, seq, KVCache(m32, 2)).double()).abs().max().item()
    with torch.no_grad():
        e_hip = (m(seq).double() - ref).abs().max().item()
        cache = KVCache(m, 2, fp8=True)
        e = (_pieces(m, seq, cache, kv_fp8=True).double() - ref).abs().max().item()
    assert cache.length == 52 and cache.lengths.tolist() == [52, 52]
    ulp = _ulp(BF16, ref.abs().max().item())
    print(f"d_model {d_model}: e_hip {e_hip:.4e} e_q {e_q:.4e} ulp {ulp:.3e} e_verify_kv8 {e:.4e}")
    assert e <= 2 * (e_q + e_hip) + ulp, (e, e_q, e_hip, ulp)


def test_decode_graph_verify_fp8():
    """Several replays of the captured 4-token verify step on an FP8 cache equal the eager step bitwise
    (logits, bytes and scales), also after a truncate (rejected proposals) in between."""
    torch.manual_seed(3)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (2, 64), device=DEV)
    cg, ce = KVCache(m, 2, fp8=True), KVCache(m, 2, fp8=True)
    with torch.no_grad():
        for c in (cg, ce):
            m.forward_cached(seq[:, :9], c)
        dg = DecodeGraph(m, cg, capture=True, tokens=4, verify=True)
        de = DecodeGraph(m, ce, capture=False, tokens=4, verify=True)
        p = 9
        for i in range(5):
            got, want = dg.step(seq[:, p:p + 4]), de.step(seq[:, p:p + 4])
            assert got.shape == (2, 4, 500) and torch.equal(got, want), p
            p += 4
            if i == 2:
                p -= 3
                cg.truncate(p)
                ce.truncate(p)
    assert cg.length == ce.length == p and cg.lengths.tolist() == [p, p] and _same_cache(cg, ce)
