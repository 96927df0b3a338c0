"""``DecodeGraph(weights=Mxfp4DecodeWeights(model))`` on the GPU, by the pattern of
``test_decode_graph_fp8_gpu.py``: the captured and replayed MXFP4 weight-only step against the same step run
eagerly (``capture=False``) on a second cache, bit for bit, and against the fp32 eager forward of a model
loaded with the DEQUANTIZED weights, with the yardstick and bound of ``test_decode_graph_gpu.py``: ``e_hip`` is
the worst error of the bf16 model's ordinary forward against the fp32 eager forward of its own weights, ``ulp``
one bf16 ulp of the largest reference logit, and the quantized steps may be off by ``2 * e_hip + ulp``.

Both arms prefill their prompt inside ``gemm.skinny_decode(weights=qw)``, so the cached K / V of the prompt
come from the quantized weights like everything after them.

Models are those of ``test_decode_graph_fp8_gpu.py`` (context 128, 2 layers, d_model 256 / 4 heads and 160 / 2
heads, d_ff 512) in bf16; every K is a multiple of 32.

Measured on an MI355X (e_hip / quantized steps / ulp / largest distance to the unquantized graph):
d_model 256: 2.03e-02 / 1.90e-02 / 1.56e-02 / 6.17e-01; d_model 160: 1.58e-02 / 1.59e-02 / 1.56e-02 / 5.29e-01.
The quantized step is as close to its exact model as the bf16 forward is to its own, and ten times the bound
away from the unquantized step: four times the FP8 step's distance."""

import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Mxfp4DecodeWeights, Sampler
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import gemm

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
MODELS = [(256, 4), (160, 2)]


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


def _model(d_model, heads, dt=BF16, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()


def _same_cache(a, b):
    return (a.length == b.length and torch.equal(a.lengths, b.lengths) and torch.equal(a.k, b.k)
            and torch.equal(a.v, b.v))


def _prefill(m, qw, tok, *caches):
    with torch.no_grad(), gemm.skinny_decode(weights=qw):
        return [m.forward_cached(tok, c) for c in caches]


@pytest.mark.parametrize("d_model,heads", MODELS)
def test_replay_equals_eager_and_error_against_the_dequantized_fp32_model(d_model, heads):
    dt = BF16
    m = _model(d_model, heads)
    qw = Mxfp4DecodeWeights(m)
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref16 = m32(seq).double()[:, 8:]  # the bf16 model's exact counterpart: e_hip as test_decode_graph_gpu takes it
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 8:] - ref16).abs().max().item()
    m32.load_state_dict(qw.dequantized_state_dict(torch.float32))
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # logits at positions 8 .. 127 of the dequantized model
    cg, ce, cp = KVCache(m, 2), KVCache(m, 2), KVCache(m, 2)
    first = _prefill(m, qw, seq[:, :9], cg, ce)[0][:, -1]
    with torch.no_grad():
        m.forward_cached(seq[:, :9], cp)
        dg = DecodeGraph(m, cg, capture=True, warmup=2, weights=qw)
        assert cg.length == 9 and cg.lengths.tolist() == [9, 9]
        de = DecodeGraph(m, ce, capture=False, weights=qw)
        plain = DecodeGraph(m, cp, capture=True)  # the unquantized graph
        rows, gap = [first], 0.0
        for n in range(9, 128):  # 119 teacher-forced steps
            got = dg.step(seq[:, n:n + 1])
            want = de.step(seq[:, n:n + 1])
            assert got.shape == (2, 1, 500) and got.dtype == dt
            assert torch.equal(got, want), n
            rows.append(got[:, -1].clone())  # the static buffer is overwritten by the next step
            gap = max(gap, (got.double() - plain.step(seq[:, n:n + 1]).double()).abs().max().item())
    assert cg.length == 128 and cg.lengths.tolist() == [128, 128] and _same_cache(cg, ce)
    graphed = torch.stack(rows, dim=1)
    e_graph = (graphed.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_mxfp4 {e_graph:.4e} ulp {ulp:.3e} "
          f"gap to the unquantized graph {gap:.4e}")
    assert e_graph <= 2 * e_hip + ulp, (e_graph, e_hip, ulp)
    # ... and it is not the unquantized step: on some step the logits differ by more than that bound
    assert gap > 2 * e_hip + ulp, (gap, e_hip, ulp)


def test_every_projection_runs_the_mxfp4_op():
    """Inside the step every projection (QKV, o, W1|W3, W2 per layer and the head) reaches
    ``cs336::gemm_skinny_w4``; the 16-bit and FP8 skinny kernels, ``torch.mm`` and the references are never
    entered."""
    from cs336_systems.ops import skinny

    m = _model(160, 2, seed=2)
    qw = Mxfp4DecodeWeights(m)
    x = torch.randint(0, 500, (2, 12), device=DEV)
    cache, cache2 = KVCache(m, 2), KVCache(m, 2)
    with torch.no_grad():  # the prefills: the ordinary projections on the 16-bit weights
        m.forward_cached(x[:, :9], cache)
        m.forward_cached(x[:, :9], cache2)
    boom = AssertionError("a 16-bit, FP8 or reference path ran inside the quantized step")
    with mock.patch.object(gemm, "skinny_w4_mm", wraps=gemm.skinny_w4_mm) as w4, \
            mock.patch.object(gemm, "skinny_mm", side_effect=boom) as sk, \
            mock.patch.object(gemm, "skinny_w8_mm", side_effect=boom), \
            mock.patch.object(torch, "mm", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_fp8", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_fp8_ref", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_mxfp4_ref", side_effect=boom), \
            mock.patch.object(skinny, "dequantize_mxfp4_rows", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_ref", side_effect=boom):
        dg = DecodeGraph(m, cache, capture=True, warmup=1, weights=qw)
        calls = w4.call_count
        assert calls == 2 * (4 * 2 + 1)  # one warm-up step and the captured one
        for i in range(3):
            dg.step(x[:, 9 + i:10 + i])
        assert w4.call_count == calls  # replays launch the recorded kernels, not Python
        DecodeGraph(m, cache2, capture=False, weights=qw).step(x[:, 9:10])
        assert w4.call_count == calls + 4 * 2 + 1 and sk.call_count == 0
    assert cache.length == 12 and cache2.length == 10


def test_fp8_cache_combines_and_refresh_is_picked_up():
    m = _model(160, 2, seed=3)
    qw = Mxfp4DecodeWeights(m)
    seq = torch.randint(0, 500, (3, 32), device=DEV)
    cg, ce, cw = KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True)
    with torch.no_grad():
        for c in (cg, ce, cw):
            m.forward_cached(seq[:, :9], c)
        dg = DecodeGraph(m, cg, weights=qw)
        de = DecodeGraph(m, ce, capture=False, weights=qw)
        d16 = DecodeGraph(m, cw, capture=False)  # 16-bit weights over an FP8 cache
        moved = False
        for n in range(9, 17):
            got = dg.step(seq[:, n:n + 1])
            assert torch.equal(got, de.step(seq[:, n:n + 1])), n
            moved = moved or not torch.equal(got, d16.step(seq[:, n:n + 1]))
        assert moved and _same_cache(cg, ce)
        # an in-place weight update: refresh() requantizes in place and the next replay reads it. Doubling the
        # head is a power of two: it moves into the scale bytes alone and doubles every logit exactly.
        old = DecodeGraph(m, cw, capture=False, weights=qw)  # a third arm on a cache of its own
        cw.reset()
        m.forward_cached(seq[:, :9], cw)
        for n in range(9, 17):
            old.step(seq[:, n:n + 1])
        m.lm_head.weight.mul_(2.0)
        stale = old.step(seq[:, 17:18]).clone()  # the quantized copy is still the old head
        qw.refresh()
        got = dg.step(seq[:, 17:18])
        assert torch.equal(got, de.step(seq[:, 17:18])) and _same_cache(cg, ce)
        assert torch.equal(got, 2 * stale) and bool(got.any())


def test_sampler_in_the_graph():
    m = _model(256, 4)
    sampler = Sampler(0.9, 20)
    qw = Mxfp4DecodeWeights(m)
    prompt = torch.randint(0, 500, (3, 9), device=DEV)
    table = torch.rand(17, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    cg, ce = KVCache(m, 3), KVCache(m, 3)
    with torch.no_grad():
        firsts = [ops.sample_logits(m.forward_cached(prompt, c)[:, -1], table[0], sampler.temperature, sampler.top_k)[:, None]
                  for c in (cg, ce)]
    assert torch.equal(*firsts)
    dg = DecodeGraph(m, cg, capture=True, weights=qw, sampler=sampler)
    de = DecodeGraph(m, ce, capture=False, weights=qw, sampler=sampler)
    for d in (dg, de):
        d.begin(firsts[0], 17, table=table)
        d.advance(16)
    got, want = dg.tokens(), de.tokens()
    assert got.shape == (3, 17) and torch.equal(got, want)
    assert cg.length == ce.length == 25 and torch.equal(cg.lengths, ce.lengths)


def test_generate_takes_the_weights():
    m = _model(160, 2, seed=4)
    qw = Mxfp4DecodeWeights(m)
    x = torch.randint(0, 500, (2, 9), device=DEV)
    torch.manual_seed(7)
    out = m.generate(x, 10, top_k=1, use_cache=True, graph=True, weights=qw)
    dg = DecodeGraph(m, KVCache(m, 2), capture=False, weights=qw)
    torch.manual_seed(7)
    assert out.shape == (2, 10) and torch.equal(out, m.generate(x, 10, top_k=1, use_cache=True, graph=dg))
