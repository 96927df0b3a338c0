"""The verify step off the GPU (reference path of ``ops.verify_attention``): ``verify_cached``,
``generate(draft=, verify="mfma")`` on dense and paged caches, and the raises that stay."""

import copy

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache, PagedKVCache


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    m = BasicsTransformerLM(vocab_size=300, context_length=64, d_model=64, num_layers=2, num_heads=2, d_ff=128,
                            rope_theta=10000.0).eval()
    noisy = copy.deepcopy(m)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in noisy.parameters():
            if p.dim() > 1:
                p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.08)
    return m, noisy, torch.randint(0, 300, (2, 9))


@pytest.mark.parametrize("kw", [{}, {"paged": True, "page_size": 16}])
def test_generate_verify_mfma_equals_greedy(models, kw):
    m, noisy, x = models
    want = m.generate(x, 40, top_k=1, use_cache=True)
    assert torch.equal(m.generate(x, 40, top_k=1, use_cache=True, draft=noisy, verify="mfma", **kw), want)


def test_verify_cached_equals_chunk_step_and_returns_pages(models):
    m, _, _ = models
    seq = torch.randint(0, 300, (2, 30))
    dense, chunk, paged = KVCache(m, 2), KVCache(m, 2), PagedKVCache(m, 2, page_size=16)
    for c in (dense, chunk, paged):
        m.forward_cached(seq[:, :9], c)
    before = paged.pages_in_use
    want = m.forward_cached(seq[:, 9:30], chunk, chunk=True)
    torch.testing.assert_close(m.verify_cached(seq[:, 9:30], dense), want)
    torch.testing.assert_close(m.verify_cached(seq[:, 9:30], paged), want)
    assert paged.length == 30 and paged.pages_in_use == before + 2
    paged.truncate(9)
    assert paged.pages_in_use == before
    paged.reset()
    assert paged.pages_in_use == 0


def test_verify_attention_paged_reference():
    g = torch.Generator().manual_seed(1)
    q = torch.randn(2, 5, 2, 32, generator=g)
    kp, vp = torch.randn(7, 2, 16, 32, generator=g), torch.randn(7, 2, 16, 32, generator=g)
    table = torch.tensor([[4, 1, -1], [6, 0, 2]], dtype=torch.int32)
    lens = torch.tensor([20, 41], dtype=torch.int32)
    o, lse = ops.verify_attention_paged(q, kp, vp, table, lens)
    ro, rl = ops.decode_attention_chunk_ref(q, ops.paged_gather(kp, table), ops.paged_gather(vp, table), lens,
                                            32 ** -0.5)
    assert torch.equal(o, ro) and torch.equal(lse, rl)


def test_old_raises_hold(models):
    m, noisy, x = models
    paged = PagedKVCache(m, 2, page_size=16)
    m.forward_cached(x, paged)
    with pytest.raises(NotImplementedError):
        m.forward_cached(x[:, :3], paged, chunk=True)
    with pytest.raises(NotImplementedError):
        DecodeGraph(m, paged, capture=False, tokens=3)
    with pytest.raises(NotImplementedError):
        m.generate(x, 4, top_k=1, use_cache=True, draft=noisy, paged=True)
    with pytest.raises(NotImplementedError):
        m.verify_cached(x[:, :3], KVCache(m, 2, fp8=True))
    DecodeGraph(m, paged, capture=False, tokens=3, verify=True).step(x[:, :3])
    assert paged.length == 12
