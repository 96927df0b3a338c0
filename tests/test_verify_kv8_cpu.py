"""The FP8 verify step off the GPU (reference path of ``ops.verify_attention(k_scale=, v_scale=)``), its
argument errors, greedy speculative decoding over FP8 caches with ``verify="mfma"`` and the raises that stay."""

import copy

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM
from cs336_systems.models.kv_cache import KVCache


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


def test_verify_attention_fp8_reference_and_argument_errors():
    g = torch.Generator().manual_seed(1)
    q = torch.randn(2, 5, 2, 32, generator=g)
    k, v = torch.randn(2, 2, 48, 32, generator=g), torch.randn(2, 2, 48, 32, generator=g)
    (k8, ks), (v8, vs) = ops.kv_quantize_ref(k), ops.kv_quantize_ref(v)
    lens = torch.tensor([20, 41], dtype=torch.int32)
    o, lse = ops.verify_attention(q, k8, v8, lens, k_scale=ks, v_scale=vs)
    ro, rl = ops.decode_attention_chunk_ref(q, ops.kv_dequantize(k8, ks), ops.kv_dequantize(v8, vs), lens, 32 ** -0.5)
    assert torch.equal(o, ro) and torch.equal(lse, rl)
    with pytest.raises(ValueError):
        ops.verify_attention(q, k8, v8, lens)
    with pytest.raises(ValueError):
        ops.verify_attention(q, k.bfloat16(), v.bfloat16(), lens, k_scale=ks, v_scale=vs)


def test_generate_verify_mfma_over_fp8_caches_equals_greedy(models):
    m, noisy, x = models
    want = m.generate(x, 40, top_k=1, use_cache=True, kv_fp8=True)
    got = m.generate(x, 40, top_k=1, use_cache=True, kv_fp8=True, draft=noisy, verify="mfma")
    assert torch.equal(got, want)


def test_verify_cached_keyword_and_the_raises_that_stay(models):
    m, noisy, x = models
    with pytest.raises(NotImplementedError):
        m.verify_cached(x[:, :3], KVCache(m, 2, fp8=True))
    with pytest.raises(ValueError):
        m.verify_cached(x[:, :3], KVCache(m, 2), kv_fp8=True)
    with pytest.raises((NotImplementedError, ValueError)):
        m.generate(x, 4, top_k=1, use_cache=True, draft=noisy, verify="mfma", kv_fp8=True, paged=True)
    a, b = KVCache(m, 2, fp8=True), KVCache(m, 2, fp8=True)
    seq = torch.randint(0, 300, (2, 30))
    for c in (a, b):
        m.forward_cached(seq[:, :9], c)
    torch.testing.assert_close(m.verify_cached(seq[:, 9:30], a, kv_fp8=True), m.forward_cached(seq[:, 9:30], b, chunk=True))
    assert a.length == 30
