"""Multi-token cached steps and greedy speculative decoding on CPU (fp32, eager reference ops), with
the set-up of ``test_generate_cache.py``: there, cached and full-forward logits differ by at most
1.2e-6 and the greedy path's top-2 logit gap never falls below 9.7e-3, so greedy equality can neither
hold nor break by a tie."""

import copy
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.models.speculative import speculative_generate
from cs336_systems.ops.rope import rope_ref

CFG = dict(vocab_size=101, context_length=32, d_model=64, num_layers=2, num_heads=4, d_ff=96, rope_theta=10000.0)


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    m = BasicsTransformerLM(**CFG).eval()
    x = torch.randint(0, 101, (3, 5))
    with torch.no_grad():
        ref = m.generate(x, 40, top_k=1)  # the uncached greedy continuation, computed once
        ref1 = m.generate(x[:1], 40, top_k=1)
    return m, x, ref, ref1


@pytest.fixture(scope="module")
def drafts(setup):
    m = setup[0]
    torch.manual_seed(5)
    other = BasicsTransformerLM(**CFG).eval()  # a freshly seeded different model
    noisy = copy.deepcopy(m)  # the target with Gaussian noise on every weight matrix, relative to its spread
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in noisy.parameters():
            if p.dim() > 1:  # 8 % of each matrix's spread: acceptance well inside (10 %, 90 %), asserted below
                p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.08)
    return dict(self=m, other=other, noisy=noisy)


# ---------------------------------------------------------------- reference ops
@pytest.mark.parametrize("n", [1, 3, 7])
def test_decode_attention_chunk_ref_against_naive(n):
    torch.manual_seed(0)
    B, H, N, d = 4, 3, 20, 16
    q = torch.randn(B, n, H, d, dtype=torch.float64)
    k = torch.randn(B, H, N, d, dtype=torch.float64)
    v = torch.randn(B, H, N, d, dtype=torch.float64)
    kv_len = torch.tensor([n, 7, 20, 2], dtype=torch.int32)
    for b in range(B):  # rows beyond the valid range must never enter the arithmetic
        k[b, :, int(kv_len[b]):] = float("nan")
        v[b, :, int(kv_len[b]):] = float("nan")
    o, lse = ops.decode_attention_chunk(q, k, v, kv_len)  # CPU: the reference
    assert o.dtype == torch.float64 and lse.dtype == torch.float32
    assert o.shape == (B, n, H, d) and lse.shape == (B, n, H)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    empty = 0
    for b in range(B):
        for i in range(n):
            L = min(max(int(kv_len[b]) - (n - 1 - i), 0), N)
            if L == 0:
                assert torch.equal(o[b, i], torch.zeros(H, d, dtype=torch.float64))
                assert torch.isinf(lse[b, i]).all() and (lse[b, i] < 0).all()
                empty += 1
                continue
            want = ops.naive_attention(q[b, i, :, None], k[b, :, :L], v[b, :, :L], is_causal=False)[:, 0]
            torch.testing.assert_close(o[b, i], want, atol=1e-6, rtol=1e-6)  # naive_attention's softmax is fp32
            s = torch.einsum("hd,hnd->hn", q[b, i], k[b, :, :L]) / math.sqrt(d)
            torch.testing.assert_close(lse[b, i], torch.logsumexp(s, -1).float(), atol=1e-6, rtol=1e-6)
    assert empty == max(n - 2, 0)  # kv_len 2 under n queries: all but the last two see no key


@pytest.mark.parametrize("n", [1, 3, 7])
def test_kv_append_rope_chunk_ref_against_rope_ref(n):
    torch.manual_seed(0)
    B, H, d, max_len, ctx = 3, 2, 8, 12, 16
    pe = BasicsTransformerLM(**CFG).positional_encoder._init_cache(ctx, d, 10000.0)
    cos, sin = pe[0], pe[1]
    qkv = torch.randn(B, n, 3 * H * d, dtype=torch.float64)
    kc = torch.full((B, H, max_len, d), 7.0, dtype=torch.float64)
    vc = torch.full((B, H, max_len, d), -7.0, dtype=torch.float64)
    pos = torch.tensor([0, 4, max_len - 2], dtype=torch.int32)  # the last chunk's tail overruns (n > 2)
    q = ops.kv_append_rope_chunk(qkv, cos, sin, pos, kc, vc)
    assert q.shape == (B, n, H, d)
    q_in, k_in, v_in = qkv.view(B, n, 3, H, d).unbind(2)
    written = torch.zeros(B, H, max_len, dtype=torch.bool)
    for b in range(B):
        for i in range(n):
            slot = int(pos[b]) + i
            if slot >= max_len:
                assert torch.equal(q[b, i], torch.zeros(H, d, dtype=torch.float64))
                continue
            p = torch.tensor([slot])
            torch.testing.assert_close(q[b, i], rope_ref(q_in[b, i, :, None], cos, sin, p)[:, 0])
            torch.testing.assert_close(kc[b, :, slot], rope_ref(k_in[b, i, :, None], cos, sin, p)[:, 0])
            assert torch.equal(vc[b, :, slot], v_in[b, i])
            written[b, :, slot] = True
    assert (kc[~written] == 7.0).all() and (vc[~written] == -7.0).all()  # no other row touched


# ---------------------------------------------------------------- the model's chunk step
def test_chunk_logits_match_full_forward(setup):
    m, x, ref, _ = setup
    seq = torch.cat((x, ref), dim=1)[:, :32]
    cache = KVCache(m, 3)
    with torch.no_grad():
        full = m(seq)
        m.forward_cached(seq[:, :5], cache)
        p = 5
        for n in (2, 3, 7, 1, 8, 6):
            logits = m.forward_cached(seq[:, p:p + n], cache, chunk=True)
            assert logits.shape == (3, n, 101)
            print(f"chunk of {n} at {p}: max |chunk - full| = {(logits - full[:, p:p + n]).abs().max().item():.3e}")
            torch.testing.assert_close(logits, full[:, p:p + n], atol=1e-5, rtol=1e-5)
            p += n
            assert cache.length == p and cache.lengths.tolist() == [p, p, p]
    assert p == 32


def test_chunk_contract_and_truncate(setup):
    m, x, ref, _ = setup
    seq = torch.cat((x, ref), dim=1)[:, :32]
    cache = KVCache(m, 3)
    with torch.no_grad():
        m.forward_cached(seq[:, :5], cache)
        with pytest.raises(NotImplementedError):  # the default stays as it was
            m.forward_cached(seq[:, 5:8], cache)
        with pytest.raises(NotImplementedError):
            m.forward_cached(seq[:, 5:8], cache, chunk=False)
        assert cache.length == 5
        a = m.forward_cached(seq[:, 5:12], cache, chunk=True)
        b = m.forward_cached(seq[:, 12:20], cache, chunk=True)
        # a chunk past the cache end raises on the host and changes nothing
        k0, v0, l0 = cache.k.clone(), cache.v.clone(), cache.lengths.clone()
        with pytest.raises(ValueError):
            m.forward_cached(seq[:, :13], cache, chunk=True)
        assert cache.length == 20 and torch.equal(cache.lengths, l0)
        assert torch.equal(cache.k, k0) and torch.equal(cache.v, v0)
        # truncate, then the same tokens again: the same logits
        cache.truncate(12)
        assert cache.length == 12 and cache.lengths.tolist() == [12, 12, 12]
        torch.testing.assert_close(m.forward_cached(seq[:, 12:20], cache, chunk=True), b, atol=1e-5, rtol=1e-5)
        cache.truncate(5)
        torch.testing.assert_close(m.forward_cached(seq[:, 5:12], cache, chunk=True), a, atol=1e-5, rtol=1e-5)
        cache.truncate(12)  # a no-op length is fine
        for bad in (-1, 13):
            with pytest.raises(ValueError):
                cache.truncate(bad)
        assert cache.length == 12 and cache.lengths.tolist() == [12, 12, 12]
        cache.truncate(0)
        assert cache.length == 0 and cache.lengths.tolist() == [0, 0, 0]


# ---------------------------------------------------------------- speculative decoding
def test_reference_decisions_are_not_ties(setup):
    m, x, ref, _ = setup
    seq = torch.cat((x, ref), dim=1)
    with torch.no_grad():
        for n in range(5, 32):
            top2 = torch.topk(m(seq[:, :n])[:, -1].float(), 2).values
            gap = (top2[:, 0] - top2[:, 1]).min().item()
            assert gap > 1e-3, (n, gap)


@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("n_new", [27, 40])  # ends exactly at the window / crosses into the sliding tail
@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("which", ["self", "other", "noisy"])
def test_speculative_equals_greedy(setup, drafts, which, k, n_new, batch):
    m, x, ref, ref1 = setup
    xb, want = (x, ref) if batch == 3 else (x[:1], ref1)
    out = m.generate(xb, n_new, top_k=1, use_cache=True, draft=drafts[which], draft_tokens=k)
    assert out.shape == (batch, n_new) and torch.equal(out, want[:, :n_new])


def test_acceptance_rates(setup, drafts):
    m, x, ref, ref1 = setup
    for k in (1, 4, 15):
        out, st = speculative_generate(m, m, x, 27, draft_tokens=k)
        assert torch.equal(out, ref[:, :27])
        assert st["rounds"] > 0 and st["accepted"] == st["proposed"], st  # (shrunk rounds propose less)
    _, st = speculative_generate(m, drafts["other"], x, 27, draft_tokens=4)
    print("different model:", st)
    assert st["accepted"] < 0.5 * st["proposed"], st
    for xb in (x, x[:1]):
        _, st = speculative_generate(m, drafts["noisy"], xb, 27, draft_tokens=4)
        rate = st["accepted"] / st["proposed"]
        print(f"noisy draft, batch {xb.shape[0]}: {st}, acceptance {rate:.2f}")
        assert 0.1 < rate < 0.9, st


def test_speculative_eos_and_shapes(setup, drafts):
    m, x, ref, ref1 = setup
    eos = int(ref1[0, 2])
    first = next(i for i in range(27) if int(ref1[0, i]) == eos)
    for which in ("self", "noisy"):
        out = m.generate(x[0], 27, top_k=1, eos_token_id=eos, use_cache=True, draft=drafts[which])
        assert out.shape == (1, first) and torch.equal(out, ref1[:, :first])
    assert torch.equal(out, m.generate(x[0], 27, top_k=1, eos_token_id=eos))
    out, st = speculative_generate(m, m, x, 0)
    assert out.shape == (3, 0) and st == dict(rounds=0, proposed=0, accepted=0)
    out = m.generate(x, 7, top_k=1, use_cache=True, draft=m, draft_tokens=4)  # trimmed to max_new_tokens
    assert out.shape == (3, 7) and torch.equal(out, ref[:, :7])
    torch.manual_seed(1)
    long = torch.randint(0, 101, (2, 45))  # a prompt longer than the window: sliding steps from the start
    assert torch.equal(m.generate(long, 6, top_k=1, use_cache=True, draft=m), m.generate(long, 6, top_k=1))


def test_speculative_errors(setup):
    m, x, _, _ = setup
    other_vocab = BasicsTransformerLM(**{**CFG, "vocab_size": 99}).eval()
    short = BasicsTransformerLM(**{**CFG, "context_length": 16}).eval()
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, draft=other_vocab)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, draft=short)
    for k in (0, 16):
        with pytest.raises(ValueError):
            m.generate(x, 4, top_k=1, use_cache=True, draft=m, draft_tokens=k)
    with pytest.raises(ValueError):  # no cache
        m.generate(x, 4, top_k=1, draft=m)
    with pytest.raises(ValueError):  # sampling from a draft
        m.generate(x, 4, top_k=5, use_cache=True, draft=m)
    with pytest.raises(ValueError):
        m.generate(x, 4, use_cache=True, draft=m)
    with pytest.raises(ValueError):  # a caller-owned graph
        m.generate(x, 4, top_k=1, use_cache=True, draft=m, graph=object())
    with pytest.raises(ValueError):  # graph=True on a CPU model
        m.generate(x, 4, top_k=1, use_cache=True, draft=m, graph=True)
