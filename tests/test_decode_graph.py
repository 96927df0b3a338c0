"""``DecodeGraph`` / ``generate(graph=...)`` / ``ops.skinny_linear`` on the CPU (fp32, eager reference
ops), on the tiny model of ``test_generate_cache.py``. The eager arm (``capture=False``) runs the same
step function a captured graph records, so on the CPU it must equal ``forward_cached`` bit for bit:
the only difference, the fixed decode-attention bound, only picks a GPU kernel's split count."""

from unittest import mock

import pytest
import torch
import torch.nn.functional as F

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import gemm

CFG = dict(vocab_size=101, context_length=32, d_model=64, num_layers=2, num_heads=4, d_ff=96, rope_theta=10000.0)


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    m = BasicsTransformerLM(**CFG).eval()
    x = torch.randint(0, 101, (3, 5))
    with torch.no_grad():
        ref = m.generate(x, 27, top_k=1, use_cache=True)
    return m, x, ref


def test_eager_step_equals_forward_cached_bitwise(setup):
    m, x, ref = setup
    seq = torch.cat((x, ref), dim=1)  # (3, 32)
    ca, cb = KVCache(m, 3), KVCache(m, 3)
    dg = DecodeGraph(m, cb, capture=False)
    with torch.no_grad():
        assert torch.equal(m.forward_cached(seq[:, :5], ca), m.forward_cached(seq[:, :5], cb))
        for n in range(5, 32):
            want = m.forward_cached(seq[:, n:n + 1], ca)
            got = dg.step(seq[:, n:n + 1])
            assert got.shape == (3, 1, 101) and torch.equal(got, want), n
            assert cb.length == ca.length == n + 1 and cb.lengths.tolist() == [n + 1] * 3
    assert torch.equal(ca.k, cb.k) and torch.equal(ca.v, cb.v)


def test_capture_needs_a_gpu(setup):
    m, _, _ = setup
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 3))
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 3), capture=True)


def test_step_on_empty_and_full_cache_raises_and_changes_nothing(setup):
    m, x, ref = setup
    seq = torch.cat((x, ref), dim=1)
    cache = KVCache(m, 3)
    dg = DecodeGraph(m, cache, capture=False)
    k0 = cache.k.clone()
    with pytest.raises(ValueError, match="prefill first"):
        dg.step(seq[:, :1])
    assert cache.length == 0 and cache.lengths.tolist() == [0, 0, 0] and torch.equal(cache.k, k0)
    with torch.no_grad():
        m.forward_cached(seq, cache)  # full: 32 of 32
    before_k, before_v = cache.k.clone(), cache.v.clone()
    with pytest.raises(ValueError):
        dg.step(seq[:, :1])
    assert cache.length == 32 and cache.lengths.tolist() == [32] * 3
    assert torch.equal(cache.k, before_k) and torch.equal(cache.v, before_v)
    with pytest.raises(ValueError):  # (B, 1) of the cache's batch only
        dg.step(seq[:2, :1])
    small = KVCache((2, 4, 16), batch=3, max_len=8, dtype=torch.float32)
    with torch.no_grad():
        m.forward_cached(seq[:, :8], small)
    with pytest.raises(ValueError):  # max_len below context_length bounds the steps too
        DecodeGraph(m, small, capture=False).step(seq[:, 8:9])
    assert small.length == 8


def test_generate_graph_argument_errors(setup):
    m, x, _ = setup
    with pytest.raises(ValueError):  # capturing needs a GPU model
        m.generate(x, 4, top_k=1, use_cache=True, graph=True)
    with pytest.raises(ValueError):  # graph needs the cache
        m.generate(x, 4, top_k=1, use_cache=False, graph=True)
    dg = DecodeGraph(m, KVCache(m, 3), capture=False)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, graph=dg)
    with pytest.raises(ValueError):  # batch differs
        m.generate(x[:2], 4, top_k=1, use_cache=True, graph=dg)
    other = BasicsTransformerLM(**CFG).eval()
    with pytest.raises(ValueError):  # another model's graph
        other.generate(x, 4, top_k=1, use_cache=True, graph=dg)


def test_generate_with_a_caller_owned_eager_graph(setup):
    m, x, ref = setup
    dg = DecodeGraph(m, KVCache(m, 3), capture=False)
    out = m.generate(x, 27, top_k=1, use_cache=True, graph=dg)
    assert torch.equal(out, ref)
    assert dg.cache.length == 31  # prompt 5 + 26 steps (the last token is sampled, not fed back)
    # reused: the cache is reset and prefilled again; past the window the uncached step takes over
    out = m.generate(x, 40, top_k=1, use_cache=True, graph=dg)
    assert out.shape == (3, 40) and torch.equal(out, m.generate(x, 40, top_k=1, use_cache=True))


def test_parallel_models_raise(setup):
    m, _, _ = setup
    m.layers[0].attn.context_parallel = (None, "ring")
    try:
        with pytest.raises(NotImplementedError):
            DecodeGraph(m, KVCache(m, 3), capture=False)
    finally:
        m.layers[0].attn.context_parallel = None


@pytest.mark.parametrize("rows", [(1,), (16,), (2, 3), (17,), (5, 8)])
def test_skinny_linear_cpu_is_f_linear(rows):
    torch.manual_seed(1)
    x, w = torch.randn(*rows, 24), torch.randn(13, 24)
    assert torch.equal(ops.skinny_linear(x, w), F.linear(x, w))
    assert torch.equal(ops.skinny_linear_ref(x, w), F.linear(x, w))
    xb, wb = x.bfloat16(), w.bfloat16()
    assert torch.equal(ops.skinny_linear(xb, wb), F.linear(xb, wb))


def test_mm_nt_reaches_the_skinny_kernel_only_inside_the_context():
    torch.manual_seed(2)
    x, w = torch.randn(4, 16), torch.randn(8, 16)
    sentinel = torch.full((4, 8), 7.0)
    with mock.patch.object(gemm, "skinny_ok", return_value=True) as ok, \
            mock.patch.object(gemm, "skinny_mm", return_value=sentinel) as mm:
        assert torch.equal(gemm.mm_nt(x, w), x @ w.t())  # off by default
        assert ok.call_count == 0 and mm.call_count == 0
        with gemm.skinny_decode():
            assert gemm.mm_nt(x, w) is sentinel
            assert mm.call_count == 1
            big = torch.randn(17, 16)
            assert torch.equal(gemm.mm_nt(big, w), big @ w.t())  # more than 16 rows: the existing path
            assert mm.call_count == 1
        assert torch.equal(gemm.mm_nt(x, w), x @ w.t())  # and off again afterwards
        assert mm.call_count == 1
    with gemm.skinny_decode():  # the real predicate refuses CPU tensors
        assert not gemm.skinny_ok(x, w)
        assert torch.equal(gemm.mm_nt(x, w), x @ w.t())
