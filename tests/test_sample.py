"""The sampling rule of ``cs336_systems/ops/sample.py`` on the CPU: the eager reference against a
plain fp64 loop over the rule, ``generate(sample_on_device=True)`` against a hand-written loop on the
same table of uniforms, reproducibility from a generator seed, and the argument errors.

The interval rule (also ``tests/test_sample_gpu.py``): a token ``t`` passes if it is in the fp64 kept
set and ``cdf64[t-1] - 1e-5 <= u <= cdf64[t] + 1e-5`` with the CDF normalised. The 1e-5 is derived:
fp32 ``exp`` on an argument of magnitude below about 40 carries a relative error under 3e-6 and a sum
of positive fp32 terms in a blocked order under 2e-6; a wrong index is off by whole probability masses."""

import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Sampler
from cs336_systems.models.kv_cache import KVCache

TOL = 1e-5
U_TOP = 1.0 - 2.0 ** -24


def _loop64(x, u, temperature, top_k):
    """The rule, one row, Python floats (fp64): (token, kept list, cdf list)."""
    x = [float(v) for v in x]
    V = len(x)
    if top_k and top_k < V:
        kth = sorted(x, reverse=True)[top_k - 1]
        keep = [v >= kth for v in x]
    else:
        keep = [True] * V
    m = max(x)
    w = [math.exp((v - m) / temperature) if k else 0.0 for v, k in zip(x, keep)]
    c, acc = [], 0.0
    for v in w:
        acc += v
        c.append(acc)
    tok = next((i for i in range(V) if keep[i] and c[i] > u * acc), None)
    if tok is None:
        tok = max(i for i in range(V) if keep[i] and w[i] > 0)
    return tok, keep, [v / acc for v in c]


def _cases():
    g = torch.Generator().manual_seed(0)
    for V in (1, 2, 7, 64, 65, 300):
        for top_k in (None, 0, 1, 2, 5, V, V + 3):
            for temperature in (0.7, 1.0, 1.5):
                x = torch.randn(4, V, generator=g) * 4
                u = torch.rand(4, generator=g)
                u[0], u[1] = 0.0, U_TOP
                yield x, u, temperature, top_k


def test_reference_fp64_is_the_rule_and_fp32_obeys_the_interval():
    rows = differ = 0
    for x, u, temperature, top_k in _cases():
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            xd = x.to(dt)
            r64 = ops.sample_logits_ref(xd, u, temperature, top_k, dtype=torch.float64)
            r32 = ops.sample_logits_ref(xd, u, temperature, top_k)
            assert r64.dtype == torch.int64 and r64.shape == (4,)
            for b in range(4):
                tok, keep, cdf = _loop64(xd[b].double().tolist(), float(u[b]), temperature, top_k)
                assert int(r64[b]) == tok
                t = int(r32[b])
                assert keep[t]
                assert (cdf[t - 1] if t else 0.0) - TOL <= float(u[b]) <= cdf[t] + TOL
                rows += 1
                differ += t != tok
    assert differ <= 0.02 * rows, (differ, rows)


def test_reference_ties_signed_zeros_and_inf():
    ninf = float("-inf")
    x = torch.tensor([[1.0, ninf, 3.0, -0.0, 3.0, 0.0, ninf, 2.0]])
    # top_k 1 with a tied max: u splits the two 3.0 entries, nothing else is returned
    got = {int(ops.sample_logits_ref(x, torch.tensor([u]), 1.0, 1)) for u in (0.0, 0.25, 0.49, 0.51, 0.75, U_TOP)}
    assert got == {2, 4}
    # k = 5: the threshold is +-0.0 and both zeros are kept; -inf never is returned
    seen = {int(ops.sample_logits_ref(x, torch.tensor([i / 512]), 1.0, 5)) for i in range(512)}
    assert seen == {0, 2, 3, 4, 5, 7}
    # no filter: -inf has probability 0 also at u = 0 and at the top
    y = torch.tensor([[ninf, 0.5, ninf]])
    assert int(ops.sample_logits_ref(y, torch.tensor([0.0]))) == 1 and int(ops.sample_logits_ref(y, torch.tensor([U_TOP]))) == 1
    # degenerate rows return an index in range
    for z in (torch.full((1, 5), ninf), torch.tensor([[1.0, float("nan"), 0.0]])):
        assert 0 <= int(ops.sample_logits_ref(z, torch.tensor([0.5]), 1.0, 2)) < z.shape[1]


def test_sample_logits_dispatch_and_errors():
    x = torch.randn(3, 11)
    u = torch.rand(3)
    assert torch.equal(ops.sample_logits(x, u, 0.8, 4), ops.sample_logits_ref(x, u, 0.8, 4))
    strided = torch.randn(3, 2, 11)
    assert torch.equal(ops.sample_logits(strided[:, -1], u), ops.sample_logits_ref(strided[:, -1].clone(), u))
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1)):
        with pytest.raises(ValueError):
            ops.sample_logits(x, u, **bad)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(3, 11, dtype=torch.int64), u)
    for bad_u in (torch.rand(4), torch.rand(3, 1), torch.rand(3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ops.sample_logits(x, bad_u)
    with pytest.raises(ValueError):
        Sampler(temperature=0.0)
    with pytest.raises(ValueError):
        Sampler(top_k=-2)


def test_sample_advance_reference():
    B, S, V = 3, 6, 17
    g = torch.Generator().manual_seed(1)
    table = torch.rand(S, B, generator=g)
    tok = torch.full((B, 1), -7)
    out = torch.full((B, S), -7)
    done = torch.zeros(B, dtype=torch.int32)
    step = torch.zeros(1, dtype=torch.int32)
    logits = [torch.randn(B, V, generator=g) * 3 for _ in range(S)]
    want = [ops.sample_logits_ref(logits[s], table[s], 0.9, 5) for s in range(S)]
    eos = int(want[2][1])  # row 1 ends at step 2 (or earlier, should the token come up before)
    ended = torch.zeros(B, dtype=torch.bool)
    for s in range(S):
        ops.sample_advance(logits[s], table, step, 0.9, 5, eos, tok, out, done)
        exp = torch.where(ended, eos, want[s])
        ended |= exp == eos
        assert torch.equal(out[:, s], exp) and torch.equal(tok[:, 0], exp)
        assert (out[:, s + 1:] == -7).all() and torch.equal(done.bool(), ended)
        step += 1
    assert ended[1]
    before = (tok.clone(), out.clone(), done.clone())
    for s in (S, -1):  # outside the table: nothing is stored
        step.fill_(s)
        ops.sample_advance(logits[0], table, step, 0.9, 5, eos, tok, out, done)
        assert all(torch.equal(a, b) for a, b in zip(before, (tok, out, done)))
    done.zero_()
    step.zero_()
    ops.sample_advance(logits[2], table, step, 0.9, 5, -1, tok, out, done)  # no end token: never latches
    assert not done.any()
    with pytest.raises(ValueError):
        ops.sample_advance(logits[0], table[0], step, 0.9, 5, eos, tok, out, done)
    with pytest.raises(ValueError):
        ops.sample_advance(logits[0], table, step.long(), 0.9, 5, eos, tok, out, done)


def _model(context_length=48, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(vocab_size=97, context_length=context_length, d_model=32, num_layers=2, num_heads=2,
                               d_ff=64, rope_theta=10000.0).eval()


def _hand_loop(m, prompt, n, table, temperature, top_k):
    """forward_cached + sample_logits_ref while the window has room, the sliding-window forward after."""
    L = m.context_length
    cache = KVCache(m, prompt.shape[0])
    with torch.no_grad():
        logits = m.forward_cached(prompt, cache)
        seq = prompt
        for s in range(n):
            if s:
                fits = seq.shape[1] <= L
                logits = m.forward_cached(seq[:, -1:], cache) if fits else m(seq[:, -L:])
            tok = ops.sample_logits_ref(logits[:, -1], table[s], temperature, top_k)
            seq = torch.cat((seq, tok[:, None]), dim=-1)
    return seq[:, prompt.shape[1]:]


@pytest.mark.parametrize("B,top_k,temperature", [(1, None, 1.0), (3, 5, 0.8), (2, 1, 1.0)])
def test_generate_on_device_equals_hand_loop_cpu(B, top_k, temperature):
    m = _model()
    prompt = torch.randint(0, 97, (B, 7), generator=torch.Generator().manual_seed(2))
    table = torch.rand(12, B, generator=torch.Generator().manual_seed(9))
    got = m.generate(prompt, 12, temperature, top_k, use_cache=True, sample_on_device=True,
                     generator=torch.Generator().manual_seed(9))
    assert got.shape == (B, 12) and torch.equal(got, _hand_loop(m, prompt, 12, table, temperature, top_k))
    # the same seed gives the same tokens, another seed does not (97 tokens, 12 draws per row)
    again = m.generate(prompt, 12, temperature, top_k, use_cache=True, sample_on_device=True,
                       generator=torch.Generator().manual_seed(9))
    assert torch.equal(got, again)
    if top_k != 1:
        other = m.generate(prompt, 12, temperature, top_k, use_cache=True, sample_on_device=True,
                           generator=torch.Generator().manual_seed(10))
        assert not torch.equal(got, other)


def test_generate_on_device_sliding_window_and_eager_decode_graph_cpu():
    m = _model(context_length=16, seed=1)
    prompt = torch.randint(0, 97, (2, 10), generator=torch.Generator().manual_seed(3))
    table = torch.rand(14, 2, generator=torch.Generator().manual_seed(4))
    want = _hand_loop(m, prompt, 14, table, 1.0, 10)  # tokens 1..6 cached, 7..13 on the sliding window
    got = m.generate(prompt, 14, 1.0, 10, use_cache=True, sample_on_device=True, generator=torch.Generator().manual_seed(4))
    assert torch.equal(got, want)
    # the eager arm of DecodeGraph(sampler=) emits the same cached tokens
    cache = KVCache(m, 2)
    with torch.no_grad():
        first = ops.sample_logits(m.forward_cached(prompt, cache)[:, -1], table[0], 1.0, 10)[:, None]
    dg = DecodeGraph(m, cache, capture=False, sampler=Sampler(1.0, 10))
    dg.begin(first, 7, table=table[:7])
    dg.advance(2)
    dg.advance(4)
    assert not dg.all_done() and torch.equal(dg.tokens(), want[:, :7])
    length = cache.length
    for bad in (lambda: dg.advance(1), lambda: dg.step(first), lambda: dg.begin(first, 17)):
        with pytest.raises(ValueError):  # past the run begin() was given; no step(); beyond the capacity
            bad()
    assert cache.length == length and torch.equal(dg.tokens(), want[:, :7])


def test_generate_on_device_eos_cpu():
    m = _model(seed=2)
    kw = dict(use_cache=True, sample_on_device=True)
    p1 = torch.randint(0, 97, (1, 5), generator=torch.Generator().manual_seed(5))
    ref = m.generate(p1, 16, 1.0, 8, generator=torch.Generator().manual_seed(6), **kw)
    eos = int(ref[0, 5])
    cut = ref[0].tolist().index(eos)
    got = m.generate(p1, 16, 1.0, 8, eos_token_id=eos, sync_every=4, generator=torch.Generator().manual_seed(6), **kw)
    assert torch.equal(got, ref[:, :cut])
    # B = 2, greedy rows on one prompt end together: the result stops with the column of their end token
    p2 = p1.expand(2, -1).contiguous()
    ref2 = m.generate(p2, 16, 1.0, 1, generator=torch.Generator().manual_seed(6), **kw)
    eos = int(ref2[0, 5])
    cut = ref2[0].tolist().index(eos)
    got = m.generate(p2, 16, 1.0, 1, eos_token_id=eos, sync_every=4, generator=torch.Generator().manual_seed(6), **kw)
    assert torch.equal(got, ref2[:, :cut + 1])
    # B = 2, sampled rows: the row that ends is padded with the end token, the other runs on
    p3 = torch.randint(0, 97, (2, 5), generator=torch.Generator().manual_seed(7))
    ref3 = m.generate(p3, 16, 1.0, 8, generator=torch.Generator().manual_seed(8), **kw)
    eos = int(ref3[0, 3])
    got = m.generate(p3, 16, 1.0, 8, eos_token_id=eos, sync_every=4, generator=torch.Generator().manual_seed(8), **kw)
    cut0 = ref3[0].tolist().index(eos)
    assert got[0, :cut0 + 1].tolist() == ref3[0, :cut0 + 1].tolist() and (got[0, cut0:] == eos).all()
    if eos not in ref3[1].tolist():
        assert torch.equal(got[1], ref3[1]) and got.shape == (2, 16)


def test_generate_on_device_argument_errors():
    m = _model()
    prompt = torch.randint(0, 97, (1, 4))
    with pytest.raises(ValueError):
        m.generate(prompt, 4, sample_on_device=True)  # needs use_cache
    with pytest.raises(ValueError):
        m.generate(prompt, 4, top_k=1, use_cache=True, sample_on_device=True, draft=m)
    with pytest.raises(ValueError):
        m.generate(prompt, 4, temperature=0.0, use_cache=True, sample_on_device=True)
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 1), capture=False, tokens=2, sampler=Sampler())
    assert m.generate(prompt, 0, use_cache=True, sample_on_device=True).shape == (1, 0)
