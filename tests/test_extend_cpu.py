"""Extend attention on the CPU: the ops run the eager reference, ``extend_cached`` reproduces the
one-shot prefill (to 1e-5, the reference path's bound in ``test_generate_chunk.py``), an FP8 cache raises
and the steps that were not supported before stay so."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache, PagedKVCache


def _model(ctx=64):
    torch.manual_seed(0)
    return BasicsTransformerLM(vocab_size=64, context_length=ctx, d_model=32, num_layers=2, num_heads=2, d_ff=64).eval()


def test_ops_run_the_reference_on_cpu():
    g = torch.Generator().manual_seed(3)
    B, n, H, d, P = 2, 5, 2, 16, 16
    q = torch.randn(B, n, H, d, generator=g)
    k, v = torch.randn(B, H, 32, d, generator=g), torch.randn(B, H, 32, d, generator=g)
    lens = torch.tensor([5, 23], dtype=torch.int32)
    want = ops.decode_attention_chunk_ref(q, k, v, lens)
    got = ops.extend_attention(q, k, v, lens, splits=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the same rows in pages 3, 0 (sequence 0) and 1, 2 (sequence 1); page 4 is nobody's
    table = torch.tensor([[3, 0], [1, 2]], dtype=torch.int32)
    kp, vp = torch.full((5, H, P, d), float("nan")), torch.full((5, H, P, d), float("nan"))
    for b in range(B):
        for t in range(2):
            kp[table[b, t]], vp[table[b, t]] = k[b, :, t * P:(t + 1) * P], v[b, :, t * P:(t + 1) * P]
    got = ops.extend_attention_paged(q, kp, vp, table, lens)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    e4m3 = torch.float8_e4m3fn
    with pytest.raises(ValueError):
        ops.extend_attention(q, k.to(e4m3), v.to(e4m3), lens)
    with pytest.raises(ValueError):
        ops.extend_attention_paged(q, kp.to(e4m3), vp.to(e4m3), table, lens)


@pytest.mark.parametrize("paged", [False, True])
def test_extend_cached_reproduces_the_prefill(paged):
    m = _model()
    seq = torch.randint(0, 64, (2, 40), generator=torch.Generator().manual_seed(4))
    cache = PagedKVCache(m, 2, page_size=16) if paged else KVCache(m, 2)
    with torch.no_grad():
        full = m(seq)
        pieces = [m.extend_cached(seq[:, a:b], cache) for a, b in ((0, 5), (5, 12), (12, 13), (13, 40))]
    assert cache.length == 40
    torch.testing.assert_close(torch.cat(pieces, dim=1), full, atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):
        m.extend_cached(seq[:, :30], cache)  # 40 + 30 exceed the window


def test_generate_prefill_chunk():
    m = _model()
    x = torch.randint(0, 64, (1, 21), generator=torch.Generator().manual_seed(5)).expand(2, -1).contiguous()
    want = m.generate(x, 8, top_k=1, use_cache=True)
    for kw in ({}, {"paged": True, "page_size": 16}, {"paged": True, "page_size": 16, "share_prompt": True}):
        assert torch.equal(m.generate(x, 8, top_k=1, use_cache=True, prefill_chunk=8, **kw), want), kw
    with pytest.raises(NotImplementedError):
        m.generate(x, 8, top_k=1, use_cache=True, prefill_chunk=8, kv_fp8=True)
    with pytest.raises(ValueError):
        m.generate(x, 8, top_k=1, prefill_chunk=8)


def test_what_raised_before_still_raises():
    m = _model()
    x = torch.randint(0, 64, (2, 9), generator=torch.Generator().manual_seed(7))
    dense, paged, fp8 = KVCache(m, 2), PagedKVCache(m, 2, page_size=16), KVCache(m, 2, fp8=True)
    for c in (dense, paged, fp8):
        m.forward_cached(x, c)
    with pytest.raises(NotImplementedError):
        m.extend_cached(x, fp8)
    with pytest.raises(NotImplementedError):
        m.forward_cached(x, dense)  # n > 1 without chunk
    with pytest.raises(NotImplementedError):
        m.forward_cached(x, paged)
    with pytest.raises(NotImplementedError):
        m.forward_cached(x, paged, chunk=True)
    with pytest.raises(NotImplementedError):
        DecodeGraph(m, paged, capture=False, tokens=2)
    with pytest.raises(NotImplementedError):
        m.generate(x, 4, top_k=1, use_cache=True, paged=True, draft=m)
