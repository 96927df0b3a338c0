"""Multi-token decode attention (``csrc/flash_attn/fa_decode_chunk.hip``) and the chunk-append kernel
on the GPU.

Oracle: fp64 attention of every query over its own key prefix ``[0, kv_len[b] - (n - 1 - i))`` and its
LSE, from the same rounded inputs. Tolerances are the ones ``test_decode_attention_gpu.py`` holds
``fa_decode`` to: max |o - ref| < 2e-2 for 16-bit inputs, < 1e-4 for fp32, the same bounds for the
finite LSE entries, and an exact finiteness pattern of the LSE. The append kernel is held to the RoPE
kernel's tolerances (1e-5 fp32, 1e-2 16-bit)."""

import functools
import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, MAX_LEN = 3, 3, 320
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DIMS = [32, 64, 80, 128]
NS = [1, 2, 7, 8, 9, 17]  # below, at and above a query tile (8); two tiles with a one-query tail
KV_SETS = ["empty", "edges", "short"]
SPLITS = [0, 1, 2, 5]


def _kv_len(kv_set, n):
    # a chunk on an empty cache; key-tile edges and the cache end; queries with no key at all
    return {"empty": (n, 65, 300), "edges": (64, 128, 320), "short": (0, 3, 300)}[kv_set]


def _grid():
    """24 of the 216 (dtype, n, kv set, splits) points per head dim, shifted per head dim; every value
    of every axis meets every head dim (checked below), and n = 7 meets the short set (queries whose
    bound is <= 0) for every head dim."""
    cases = []
    for di, d in enumerate(DIMS):
        mine = set()
        for i in range(24):
            mine.add((DTYPES[(i + i // 6) % 3], NS[i % 6], KV_SETS[(i // 2 + di) % 3], SPLITS[(i + i // 6 + di) % 4]))
        mine.add((DTYPES[di % 3], 7, "short", SPLITS[(di + 1) % 4]))
        for axis, vals in enumerate((DTYPES, NS, KV_SETS, SPLITS)):
            assert {c[axis] for c in mine} == set(vals), (d, axis)
        cases += [(d, *c) for c in sorted(mine, key=str)]
    return cases


def _tol(dt):
    return 2e-2 if dt != torch.float32 else 1e-4


def _bound(kv, n, i, max_len):
    return min(max(kv - (n - 1 - i), 0), max_len)


def _oracle(q, k, v, kv_len, scale):
    """fp64 attention of each query over its own key prefix only (NaN tails never touched)."""
    Bq, n = q.shape[:2]
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, kv in enumerate(kv_len):
        for i in range(n):
            L = _bound(kv, n, i, k.shape[2])
            if L == 0:
                continue
            s = torch.einsum("hd,hnd->hn", q[b, i].double(), k[b, :, :L].double()) * scale
            lse[b, i] = torch.logsumexp(s, -1)
            o[b, i] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v[b, :, :L].double())
    return o, lse


@functools.lru_cache(maxsize=None)
def _case(dt, d, n, kv_len, qmul=1.0):
    """Inputs (cache rows at and beyond kv_len[b] are NaN) and their oracle, built once per case and
    shared by every split count; nothing modifies them."""
    g = torch.Generator(device=DEV).manual_seed(4321 + d + n)
    q = (torch.randn(B, n, H, d, device=DEV, generator=g) * qmul).to(dt)
    k = torch.randn(B, H, MAX_LEN, d, device=DEV, generator=g).to(dt)
    v = torch.randn(B, H, MAX_LEN, d, device=DEV, generator=g).to(dt)
    for b, kv in enumerate(kv_len):
        k[b, :, kv:] = float("nan")
        v[b, :, kv:] = float("nan")
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, kv_len, 1.0 / math.sqrt(d))
    return q, k, v, lens, ref_o, ref_l


def _check(o, lse, ref_o, ref_l, dt, what=""):
    assert o.dtype == dt and lse.dtype == torch.float32
    assert o.shape == ref_o.shape and lse.shape == ref_l.shape
    assert torch.isfinite(o).all(), what
    eo = (o.double() - ref_o).abs().max().item()
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(lse), fin), what
    assert (lse[~fin] < 0).all(), what
    assert torch.equal(o[~fin], torch.zeros_like(o[~fin])), what  # a query with no key: o = 0
    el = (lse.double()[fin] - ref_l[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what} max|o-ref| {eo:.3e} max|lse-ref| {el:.3e}")
    assert eo < _tol(dt), (what, eo)
    assert el < _tol(dt), (what, el)


def test_extension_has_chunk_ops():
    assert _ext.load_ext(), _ext.load_error()
    assert hasattr(torch.ops.cs336, "fa_decode_chunk") and hasattr(torch.ops.cs336, "kv_append_rope_chunk")
    assert [int(torch.ops.cs336.fa_decode_chunk_qt(n)) for n in (1, 2, 3, 4, 5, 8, 9, 17)] == [1, 4, 4, 4, 8, 8, 8, 8]


@pytest.mark.parametrize("d,dt,n,kv_set,splits", _grid())
def test_decode_attention_chunk_grid(d, dt, n, kv_set, splits):
    kv_len = _kv_len(kv_set, n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    o, lse = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    if kv_set == "short" and n >= 7:
        assert not torch.isfinite(ref_l[0]).any() and not torch.isfinite(ref_l[1, :n - 3]).any()
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} n{n} {kv_len} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("n", [2, 9])
@pytest.mark.parametrize("dt", DTYPES)
def test_peaky(dt, n, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k, v, lens, ref_o, ref_l = _case(dt, 64, n, _kv_len("empty", n), 8.0)
    o, lse = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, dt, f"peaky {dt} n{n} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("n", [7, 9])
def test_masking_is_structural(n, splits):
    """Large finite garbage in cache row j leaves every query whose bound is <= j bitwise unchanged and
    moves every query that sees row j."""
    dt = torch.bfloat16
    kv_len = _kv_len("edges", n)
    q, k, v, lens, _, _ = _case(dt, 64, n, kv_len)
    o0, l0 = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    back = 3  # row j = kv_len - 3: the last 3 queries see it, the others do not
    k2, v2 = k.clone(), v.clone()
    for b, kv in enumerate(kv_len):
        k2[b, :, kv - back] = 1.0e4
        v2[b, :, kv - back] = -1.0e4
    o1, l1 = ops.decode_attention_chunk(q, k2, v2, lens, splits=splits)
    assert torch.isfinite(o1).all()
    assert torch.equal(o1[:, :n - back], o0[:, :n - back]) and torch.equal(l1[:, :n - back], l0[:, :n - back])
    for i in range(n - back, n):
        assert not torch.equal(o1[:, i], o0[:, i]) and not torch.equal(l1[:, i], l0[:, i]), i


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("d", [64, 80])
def test_strided_cache_views_bitwise(d, splits):
    """A layer slice of an (L, B, H, max_len, d) cache and a batch sub-view are read in place and give
    the bits of the contiguous call."""
    dt, n = torch.bfloat16, 9
    kv_len = _kv_len("empty", n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    o0, l0 = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    big_k = torch.full((2, B, H, MAX_LEN, d), float("nan"), device=DEV, dtype=dt)
    big_v = torch.full_like(big_k, float("nan"))
    big_k[1].copy_(k)
    big_v[1].copy_(v)
    o1, l1 = ops.decode_attention_chunk(q, big_k[1], big_v[1], lens, splits=splits)
    assert torch.equal(o1, o0) and torch.equal(l1, l0)
    o2, l2 = ops.decode_attention_chunk(q[1:3], k[1:3], v[1:3], lens[1:3], splits=splits)
    o3, l3 = ops.decode_attention_chunk(q[1:3].clone(), k[1:3].clone(), v[1:3].clone(), lens[1:3].clone(),
                                        splits=splits)
    assert torch.equal(o2, o3) and torch.equal(l2, l3)
    _check(o2, l2, ref_o[1:3], ref_l[1:3], dt, f"batch sub-view d{d} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("n", [2, 17])
def test_run_to_run_bitwise(n, splits):
    q, k, v, lens, _, _ = _case(torch.bfloat16, 128, n, _kv_len("empty", n))
    o0, l0 = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    o1, l1 = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_one_query_agrees_with_fa_decode(dt, d, splits):
    q, k, v, lens, ref_o, ref_l = _case(dt, d, 1, _kv_len("empty", 1))
    o, lse = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
    o1, lse1 = ops.decode_attention(q[:, 0], k, v, lens, splits=splits)
    assert (o[:, 0].double() - o1.double()).abs().max().item() < _tol(dt)
    assert (lse[:, 0].double() - lse1.double()).abs().max().item() < _tol(dt)


def test_64bit_cache_offsets():
    """Head 1 of a (1, 2, 2^23 + 8, 128) bf16 cache starts beyond a 2 GiB byte offset."""
    d, n, kv, max_len = 128, 9, 300, 2**23 + 8
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    k = torch.empty(1, 2, max_len, d, device=DEV, dtype=dt)
    v = torch.empty(1, 2, max_len, d, device=DEV, dtype=dt)
    assert k.stride(1) * k.element_size() > 2**31
    k[:, :, :kv] = torch.randn(1, 2, kv, d, device=DEV, generator=g).to(dt)
    v[:, :, :kv] = torch.randn(1, 2, kv, d, device=DEV, generator=g).to(dt)
    q = torch.randn(1, n, 2, d, device=DEV, generator=g).to(dt)
    lens = torch.tensor([kv], dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, (kv,), 1.0 / math.sqrt(d))
    for splits in (0, 1):  # 0: the host sizes the split count from max_kv_len = max_len
        o, lse = ops.decode_attention_chunk(q, k, v, lens, splits=splits)
        _check(o, lse, ref_o, ref_l, dt, f"64-bit splits {splits}:")


def test_unsupported_inputs_raise():
    q, k, v, lens, _, _ = _case(torch.bfloat16, 64, 2, _kv_len("empty", 2))
    hip = torch.ops.cs336
    with pytest.raises(RuntimeError):  # head dim the kernel does not take
        hip.fa_decode_chunk(q[..., :48].contiguous(), k[..., :48].contiguous(), v[..., :48].contiguous(), lens, 0.1,
                            300, 0)
    with pytest.raises(RuntimeError):  # q must be (B, n, H, D)
        hip.fa_decode_chunk(q[:, 0], k, v, lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # kv_len must be int32 on the device
        hip.fa_decode_chunk(q, k, v, lens.long(), 0.1, 300, 0)
    with pytest.raises(RuntimeError):
        hip.fa_decode_chunk(q, k, v, lens, 0.1, MAX_LEN + 1, 0)
    with pytest.raises(RuntimeError):
        hip.fa_decode_chunk(q, k.float(), v.float(), lens, 0.1, 300, 0)
    # the wrapper runs the reference for other head dims
    o, lse = ops.decode_attention_chunk(q[..., :48].contiguous(), k[..., :48].contiguous(),
                                        v[..., :48].contiguous(), lens)
    assert o.shape == (B, 2, H, 48) and torch.isfinite(o).all()


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        q = torch.empty(2, 4, 5, 80, device=DEV, dtype=torch.bfloat16)
        cache = torch.empty(3, 2, 5, 40, 80, device=DEV, dtype=torch.bfloat16)
        lens = torch.empty(2, device=DEV, dtype=torch.int32)
        o, lse = torch.ops.cs336.fa_decode_chunk(q, cache[1], cache[2], lens, 0.1, 40, 0)
        assert o.shape == (2, 4, 5, 80) and o.dtype == torch.bfloat16
        assert lse.shape == (2, 4, 5) and lse.dtype == torch.float32
        qkv = torch.empty(2, 4, 3 * 5 * 80, device=DEV, dtype=torch.bfloat16)
        cs = torch.empty(40, 40, device=DEV, dtype=torch.float32)
        qo = torch.ops.cs336.kv_append_rope_chunk(qkv, cs, cs, lens, cache[1], cache[2])
        assert qo.shape == (2, 4, 5, 80) and qo.dtype == torch.bfloat16


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_kv_append_rope_chunk(dt, d, n):
    from cs336_systems.models import RotaryEmbedding

    max_len = 16
    g = torch.Generator(device=DEV).manual_seed(d + n)
    re = RotaryEmbedding(max_len, d, 10000.0).to(DEV)
    qkv = torch.randn(B, n, 3 * H * d, device=DEV, generator=g).to(dt)
    # caches are layer slices of a larger tensor, pre-filled with a sentinel
    sent_k, sent_v = 3.0, -5.0
    big_k = torch.full((2, B, H, max_len, d), sent_k, device=DEV, dtype=dt)
    big_v = torch.full((2, B, H, max_len, d), sent_v, device=DEV, dtype=dt)
    pos_l = [0, 5, max_len - 2]  # the last sequence's tail overruns the cache for n > 2
    pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
    q = ops.kv_append_rope_chunk(qkv, re.cos, re.sin, pos, big_k[1], big_v[1])
    assert q.shape == (B, n, H, d) and q.dtype == dt and q.is_contiguous()
    q_in, k_in, v_in = qkv.view(B, n, 3, H, d).unbind(2)
    tol = 1e-5 if dt == torch.float32 else 1e-2
    untouched = torch.ones(2, B, H, max_len, dtype=torch.bool, device=DEV)
    for b, pb in enumerate(pos_l):
        for i in range(n):
            slot = pb + i
            if slot >= max_len:  # nothing stored, a zero q row
                assert torch.equal(q[b, i], torch.zeros_like(q[b, i]))
                continue
            p = torch.tensor([slot], device=DEV)
            q_ref = ops.rope_ref(q_in[b, i].float().unsqueeze(1), re.cos, re.sin, p).squeeze(1)
            k_ref = ops.rope_ref(k_in[b, i].float().unsqueeze(1), re.cos, re.sin, p).squeeze(1)
            torch.testing.assert_close(q[b, i].float(), q_ref, rtol=tol, atol=tol)
            torch.testing.assert_close(big_k[1, b, :, slot].float(), k_ref, rtol=tol, atol=tol)
            assert torch.equal(big_v[1, b, :, slot], v_in[b, i])
            untouched[1, b, :, slot] = False
    assert (big_k[untouched] == sent_k).all() and (big_v[untouched] == sent_v).all()


def test_chunk_step_runs_the_hip_ops():
    """A chunk step calls decode_attention_chunk and kv_append_rope_chunk once per layer, and they go
    to the HIP ops (the eager references are never entered)."""
    from cs336_systems.models import BasicsTransformerLM
    from cs336_systems.models.kv_cache import KVCache
    from cs336_systems.ops import decode as dec

    torch.manual_seed(2)
    cfg = dict(vocab_size=500, context_length=128, d_model=160, num_layers=2, num_heads=2, d_ff=512, rope_theta=10000.0)
    m = BasicsTransformerLM(**cfg, device=DEV).to(torch.bfloat16).eval()
    x = torch.randint(0, 500, (2, 30), device=DEV)
    cache = KVCache(m, 2)
    boom = AssertionError("the eager reference ran on the GPU path")
    with mock.patch.object(ops, "decode_attention_chunk", wraps=ops.decode_attention_chunk) as att, \
            mock.patch.object(ops, "kv_append_rope_chunk", wraps=ops.kv_append_rope_chunk) as app, \
            mock.patch.object(dec, "decode_attention_chunk_ref", side_effect=boom), \
            mock.patch.object(dec, "kv_append_rope_chunk_ref", side_effect=boom), \
            mock.patch.object(dec, "decode_attention_ref", side_effect=boom), \
            mock.patch.object(dec, "kv_append_rope_ref", side_effect=boom):
        m.forward_cached(x[:, :9], cache, chunk=True)
        assert att.call_count == 0 and app.call_count == 0  # the prefill is the ordinary attention
        p = 9
        for i, n in enumerate((2, 9, 5)):
            logits = m.forward_cached(x[:, p:p + n], cache, chunk=True)
            assert logits.shape == (2, n, 500)
            p += n
            assert att.call_count == 2 * (i + 1) and app.call_count == 2 * (i + 1)
        m.forward_cached(x[:, p:p + 1], cache, chunk=True)  # one token: the single-token ops
        assert att.call_count == 6 and app.call_count == 6
    assert cache.length == 26 and cache.lengths.tolist() == [26, 26]
