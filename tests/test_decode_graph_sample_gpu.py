"""``DecodeGraph(sampler=)`` and ``generate(sample_on_device=True)`` on the GPU: the captured sequence
(model step, fused sampler, ``step += 1``) replayed against the same sequence run eagerly
(``capture=False``) on a second cache, token for token; ``advance`` without a host sync; ``generate``
against a hand loop over the eager step and ``ops.sample_logits`` on the same table of uniforms, also
across the sliding-window tail; the end-token handling; the argument errors.

The model is the tiny one of ``test_decode_graph_gpu.py`` (vocab 500, context 128, 2 layers) in bf16."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, Sampler
from cs336_systems.models.kv_cache import KVCache

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _model(context_length=128, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(vocab_size=500, context_length=context_length, d_model=256, num_layers=2, num_heads=4,
                               d_ff=512, rope_theta=10000.0, device=DEV).to(torch.bfloat16).eval()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _prefill(m, prompt, cache, u0, sampler):
    with torch.no_grad():
        logits = m.forward_cached(prompt, cache)
    return ops.sample_logits(logits[:, -1], u0, sampler.temperature, sampler.top_k)[:, None]


@pytest.mark.parametrize("B,top_k,fp8w,fp8kv", [(1, 1, False, False), (1, 20, False, False), (3, 1, False, False),
                                                (3, 20, False, False), (3, 20, True, False), (3, 20, False, True)])
def test_replay_equals_eager(B, top_k, fp8w, fp8kv):
    m = _model()
    sampler = Sampler(0.9, top_k)
    qw = Fp8DecodeWeights(m) if fp8w else None
    prompt = torch.randint(0, 500, (B, 9), device=DEV)
    table = torch.rand(25, B, device=DEV, generator=_gen(1))
    cg, ce = KVCache(m, B, fp8=fp8kv), KVCache(m, B, fp8=fp8kv)
    first = _prefill(m, prompt, cg, table[0], sampler)
    assert torch.equal(first, _prefill(m, prompt, ce, table[0], sampler))
    dg = DecodeGraph(m, cg, capture=True, weights=qw, sampler=sampler)
    assert cg.length == 9 and cg.lengths.tolist() == [9] * B  # construction leaves the cache as it found it
    de = DecodeGraph(m, ce, capture=False, weights=qw, sampler=sampler)
    for d in (dg, de):
        d.begin(first, 25, table=table)
        d.advance(24)
    got, want = dg.tokens(), de.tokens()
    assert got.shape == (B, 25) and torch.equal(got[:, :1], first) and torch.equal(got, want)
    assert cg.length == ce.length == 33 and torch.equal(cg.lengths, ce.lengths)
    assert int(dg.step_t) == 25 and not dg.all_done()
    # a second run on the same graph: the buffers are re-used, nothing is re-captured
    cg.reset()
    first = _prefill(m, prompt, cg, table[0], sampler)
    dg.begin(first, 25, table=table)
    dg.advance(24)
    assert torch.equal(dg.tokens(), want)


def test_advance_synchronizes_nothing_and_failed_checks_change_nothing():
    m = _model()
    sampler = Sampler(1.0, 20, eos_token_id=3)
    prompt = torch.randint(0, 500, (2, 9), device=DEV)
    cache = KVCache(m, 2)
    first = _prefill(m, prompt, cache, torch.rand(2, device=DEV), sampler)
    dg = DecodeGraph(m, cache, capture=True, sampler=sampler)
    dg.begin(first, 12, generator=_gen(2))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dg.advance(8)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert dg.tokens().shape == (2, 9) and cache.length == 17
    before = dg.tokens()
    for bad in (lambda: dg.advance(4), lambda: dg.step(first), lambda: dg.begin(first, 129),
                lambda: dg.begin(first[:1], 4)):
        with pytest.raises(ValueError):
            bad()
    assert cache.length == 17 and cache.lengths.tolist() == [17, 17] and torch.equal(dg.tokens(), before)
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 2), capture=False, tokens=2, sampler=sampler)
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 2), capture=False).begin(first, 4)


def _hand_loop(m, prompt, n, table, temperature, top_k):
    """The eager DecodeGraph step + ops.sample_logits while the window has room, the sliding-window forward after."""
    L = m.context_length
    cache = KVCache(m, prompt.shape[0])
    sampler = Sampler(temperature, top_k)
    tok = _prefill(m, prompt, cache, table[0], sampler)
    de = DecodeGraph(m, cache, capture=False)
    seq = torch.cat((prompt, tok), dim=-1)
    with torch.no_grad():
        for s in range(1, n):
            logits = de.step(tok) if seq.shape[1] <= L else m(seq[:, -L:])
            tok = ops.sample_logits(logits[:, -1], table[s], temperature, top_k)[:, None]
            seq = torch.cat((seq, tok), dim=-1)
    return seq[:, prompt.shape[1]:]


@pytest.mark.parametrize("L,P,n,B", [(128, 9, 24, 3), (32, 20, 20, 2)])  # the second crosses into the sliding window
def test_generate_equals_hand_loop(L, P, n, B):
    m = _model(context_length=L, seed=1)
    prompt = torch.randint(0, 500, (B, P), device=DEV)
    table = torch.rand(n, B, device=DEV, generator=_gen(3))
    want = _hand_loop(m, prompt, n, table, 0.8, 20)
    kw = dict(use_cache=True, sample_on_device=True)
    got = m.generate(prompt, n, 0.8, 20, graph=True, generator=_gen(3), **kw)
    assert got.shape == (B, n) and torch.equal(got, want)
    # without a graph the cached steps are forward_cached's (other GEMM kernels: other roundings); token 0 is the same
    eager = m.generate(prompt, n, 0.8, 20, generator=_gen(3), **kw)
    assert eager.shape == (B, n) and torch.equal(eager[:, :1], want[:, :1])
    # a caller-owned graph, twice
    dg = DecodeGraph(m, KVCache(m, B), capture=True, sampler=Sampler(0.8, 20))
    for _ in range(2):
        assert torch.equal(m.generate(prompt, n, 0.8, 20, graph=dg, generator=_gen(3), **kw), want)
    with pytest.raises(ValueError):  # the graph samples by its own Sampler
        m.generate(prompt, n, 0.7, 20, graph=dg, **kw)
    with pytest.raises(ValueError):
        m.generate(prompt, n, 0.8, 20, graph=DecodeGraph(m, KVCache(m, B), capture=False), **kw)


def _expected(ref, eos):
    """What the run that produced ``ref`` without an end token gives with one: a row keeps its tokens up
    to its first ``eos`` and emits ``eos`` from there on (rows do not see each other); once every row has
    ended the result stops with the column in which the last one did."""
    rows = [r.index(eos) if eos in r else None for r in ref.tolist()]
    out = ref.clone()
    for b, f in enumerate(rows):
        if f is not None:
            out[b, f:] = eos
    return out if None in rows else out[:, :max(rows) + 1]


def test_generate_eos():
    m = _model(seed=2)
    kw = dict(use_cache=True, sample_on_device=True, graph=True)
    p1 = torch.randint(0, 500, (1, 9), device=DEV)
    ref = m.generate(p1, 24, 1.0, 20, generator=_gen(4), **kw)
    eos = int(ref[0, 5])
    cut = ref[0].tolist().index(eos)  # 5, unless the token came up before
    got = m.generate(p1, 24, 1.0, 20, eos_token_id=eos, sync_every=4, generator=_gen(4), **kw)
    assert torch.equal(got, ref[:, :cut])
    # B = 2, greedy rows on one prompt end together: generation stops and the result ends with that column
    p2 = p1.expand(2, -1).contiguous()
    ref2 = m.generate(p2, 24, 1.0, 1, generator=_gen(4), **kw)
    assert torch.equal(ref2[0], ref2[1])
    eos = int(ref2[0, 5])
    cache = KVCache(m, 2)
    dg = DecodeGraph(m, cache, capture=True, sampler=Sampler(1.0, 1, eos))
    got = m.generate(p2, 24, 1.0, 1, eos_token_id=eos, sync_every=4, generator=_gen(4), use_cache=True,
                     sample_on_device=True, graph=dg)
    assert got.shape[1] <= 6 and torch.equal(got, _expected(ref2, eos))
    assert cache.length <= 9 + 8  # stopped at the poll after both rows ended, not at the end of the run
    # B = 2, sampled rows: the row that ends is padded with the end token, the other runs on
    p3 = torch.randint(0, 500, (2, 9), device=DEV)
    ref3 = m.generate(p3, 24, 1.0, 20, generator=_gen(5), **kw)
    eos = int(ref3[0, 3])
    got = m.generate(p3, 24, 1.0, 20, eos_token_id=eos, sync_every=4, generator=_gen(5), **kw)
    assert torch.equal(got, _expected(ref3, eos)) and bool((got[0, 3:] == eos).all())


def test_generate_errors():
    m = _model()
    prompt = torch.randint(0, 500, (1, 9), device=DEV)
    with pytest.raises(ValueError):
        m.generate(prompt, 4, top_k=1, use_cache=True, sample_on_device=True, draft=m)
    with pytest.raises(ValueError):
        m.generate(prompt, 4, sample_on_device=True)
