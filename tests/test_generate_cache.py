"""KV-cached generation on CPU (fp32, eager reference ops): ``forward_cached`` and
``generate(use_cache=True)`` against the full forward / the uncached ``generate``.

Figures for this set-up (pure-PyTorch cached step, fp32 CPU): cached and full-forward logits differ
by at most 1.2e-6 over the 27 steps, and the full forward's top-2 logit gap never falls below 9.7e-3,
so greedy equality can neither hold nor break by a tie."""

import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops.rope import rope_ref

CFG = dict(vocab_size=101, context_length=32, d_model=64, num_layers=2, num_heads=4, d_ff=96, rope_theta=10000.0)


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    m = BasicsTransformerLM(**CFG).eval()
    x = torch.randint(0, 101, (3, 5))
    with torch.no_grad():
        ref = m.generate(x, 27, top_k=1)  # the uncached greedy continuation, computed once
    return m, x, ref


def test_teacher_forced_logits_match_full_forward(setup):
    m, x, ref = setup
    seq = torch.cat((x, ref), dim=1)  # (3, 32)
    cache = KVCache(m, 3)
    with torch.no_grad():
        for n in range(5, 33):
            logits = m.forward_cached(seq[:, :5] if n == 5 else seq[:, n - 1:n], cache)
            full = m(seq[:, :n])[:, -1]
            err = (logits[:, -1] - full).abs().max().item()
            print(f"len {n}: max |cached - full| = {err:.3e}")
            torch.testing.assert_close(logits[:, -1], full, atol=1e-5, rtol=1e-5)
    assert cache.length == 32


def test_greedy_equals_uncached(setup):
    m, x, ref = setup
    seq = torch.cat((x, ref), dim=1)
    with torch.no_grad():
        for n in range(5, 32):  # the reference's decisions are not ties
            top2 = torch.topk(m(seq[:, :n])[:, -1].float(), 2).values
            gap = (top2[:, 0] - top2[:, 1]).min().item()
            assert gap > 1e-3, (n, gap)
    out = m.generate(x, 27, top_k=1, use_cache=True)
    assert torch.equal(out, ref)


def test_window_overflow_and_long_prompt(setup):
    m, x, _ = setup
    ref = m.generate(x, 40, top_k=1)
    out = m.generate(x, 40, top_k=1, use_cache=True)
    assert out.shape == (3, 40) and torch.equal(out, ref)
    torch.manual_seed(1)
    long = torch.randint(0, 101, (2, 45))  # longer than context_length: prefill on the last 32 tokens
    assert torch.equal(m.generate(long, 6, top_k=1, use_cache=True), m.generate(long, 6, top_k=1))


def test_shapes_eos_and_sampling(setup):
    m, x, ref = setup
    out = m.generate(x[0], 7, top_k=1, use_cache=True)  # 1-D prompt
    assert out.shape == (1, 7) and torch.equal(out, ref[:1, :7])
    # eos early stop (batch 1): stop at the token greedy decoding emits third
    eos = int(ref[0, 2])
    first = next(i for i in range(27) if int(ref[0, i]) == eos)
    out = m.generate(x[0], 27, top_k=1, eos_token_id=eos, use_cache=True)
    assert torch.equal(out, m.generate(x[0], 27, top_k=1, eos_token_id=eos))
    assert out.shape == (1, first)
    torch.manual_seed(3)
    out = m.generate(x, 9, temperature=0.7, top_k=5, use_cache=True)
    assert out.shape == (3, 9) and out.dtype == torch.int64
    assert int(out.min()) >= 0 and int(out.max()) < 101
    assert m.generate(x, 0, use_cache=True).shape == (3, 0)


def test_kv_cache_contract(setup):
    m, x, ref = setup
    cache = KVCache(m, 3)
    assert cache.k.shape == (2, 3, 4, 32, 16) and cache.v.shape == cache.k.shape
    assert cache.max_len == 32 and cache.length == 0
    assert cache.lengths.dtype == torch.int32 and cache.lengths.tolist() == [0, 0, 0]
    logits = m.forward_cached(x, cache)
    assert logits.shape == (3, 5, 101)
    assert cache.length == 5 and cache.lengths.tolist() == [5, 5, 5]
    assert m.forward_cached(ref[:, :1], cache).shape == (3, 1, 101)
    assert cache.length == 6 and cache.lengths.tolist() == [6, 6, 6]
    with pytest.raises(NotImplementedError):  # chunked prefill
        m.forward_cached(ref[:, 1:3], cache)
    with pytest.raises(ValueError):  # batch mismatch
        m.forward_cached(ref[:2, 1:2], cache)
    assert cache.length == 6
    cache.reset()
    assert cache.length == 0 and cache.lengths.tolist() == [0, 0, 0]
    # a full cache: the step raises on the host and changes nothing
    seq = torch.cat((x, ref), dim=1)
    m.forward_cached(seq, cache)
    assert cache.length == 32
    before = cache.k.clone()
    with pytest.raises(ValueError):
        m.forward_cached(seq[:, :1], cache)
    assert cache.length == 32 and torch.equal(cache.k, before)
    with pytest.raises(ValueError):  # a prompt longer than the cache
        m.forward_cached(torch.cat((seq, seq[:, :1]), dim=1), KVCache(m, 3))
    small = KVCache((2, 4, 16), batch=3, max_len=8, dtype=torch.float32)
    assert small.k.shape == (2, 3, 4, 8, 16)
    m.forward_cached(seq[:, :8], small)
    with pytest.raises(ValueError):  # max_len below context_length bounds the steps too
        m.forward_cached(seq[:, 8:9], small)


def test_parallel_models_raise(setup):
    m, x, _ = setup
    m.layers[0].attn.context_parallel = (None, "ring")
    try:
        with pytest.raises(NotImplementedError):
            m.forward_cached(x, KVCache(m, 3))
    finally:
        m.layers[0].attn.context_parallel = None


def test_decode_attention_ref_against_naive():
    torch.manual_seed(0)
    B, H, n, d = 4, 3, 20, 16
    q = torch.randn(B, H, d, dtype=torch.float64)
    k = torch.randn(B, H, n, d, dtype=torch.float64)
    v = torch.randn(B, H, n, d, dtype=torch.float64)
    kv_len = torch.tensor([1, 7, 20, 0], dtype=torch.int32)
    for b in range(B):  # rows beyond the valid range must never enter the arithmetic
        k[b, :, int(kv_len[b]):] = float("nan")
        v[b, :, int(kv_len[b]):] = float("nan")
    o, lse = ops.decode_attention(q, k, v, kv_len)  # CPU: the reference
    assert o.dtype == torch.float64 and lse.dtype == torch.float32 and o.shape == (B, H, d) and lse.shape == (B, H)
    for b in range(3):
        L = int(kv_len[b])
        want = ops.naive_attention(q[b, :, None], k[b, :, :L], v[b, :, :L], is_causal=False)[:, 0]
        torch.testing.assert_close(o[b], want, atol=1e-6, rtol=1e-6)  # naive_attention's softmax is fp32
        s = torch.einsum("hd,hnd->hn", q[b], k[b, :, :L]) / math.sqrt(d)
        torch.testing.assert_close(lse[b], torch.logsumexp(s, -1).float(), atol=1e-6, rtol=1e-6)
    assert torch.equal(o[3], torch.zeros(H, d, dtype=torch.float64))
    assert torch.isinf(lse[3]).all() and (lse[3] < 0).all()
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()


def test_kv_append_rope_ref_against_rope_ref():
    torch.manual_seed(0)
    B, H, d, max_len, ctx = 3, 2, 8, 6, 10
    pe = BasicsTransformerLM(**CFG).positional_encoder._init_cache(ctx, d, 10000.0)
    cos, sin = pe[0], pe[1]
    qkv = torch.randn(B, 3 * H * d, dtype=torch.float64)
    kc = torch.full((B, H, max_len, d), 7.0, dtype=torch.float64)
    vc = torch.full((B, H, max_len, d), -7.0, dtype=torch.float64)
    pos = torch.tensor([0, 5, 6], dtype=torch.int32)  # the last one is past the cache: skipped
    q = ops.kv_append_rope(qkv, cos, sin, pos, kc, vc)
    q_in, k_in, v_in = qkv.view(B, 3, H, d).unbind(1)
    for b in range(2):
        p = torch.tensor([int(pos[b])])
        torch.testing.assert_close(q[b], rope_ref(q_in[b, :, None], cos, sin, p)[:, 0])
        torch.testing.assert_close(kc[b, :, int(pos[b])], rope_ref(k_in[b, :, None], cos, sin, p)[:, 0])
        assert torch.equal(vc[b, :, int(pos[b])], v_in[b])
    written = torch.zeros(B, H, max_len, dtype=torch.bool)
    written[0, :, 0] = written[1, :, 5] = True
    assert (kc[~written] == 7.0).all() and (vc[~written] == -7.0).all()  # no other row touched
    assert torch.equal(q[2], torch.zeros(H, d, dtype=torch.float64))
