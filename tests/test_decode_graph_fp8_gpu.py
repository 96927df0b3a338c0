"""``DecodeGraph(weights=Fp8DecodeWeights(model))`` on the GPU: the captured and replayed FP8 weight-only
step against the same step run eagerly (``capture=False``) on a second cache, bit for bit, and against
the fp32 eager forward of a model loaded with the DEQUANTIZED weights, with the yardstick and bound of
``test_decode_graph_gpu.py``: ``e_hip`` is the worst error of the bf16 model's ordinary forward against
the fp32 eager forward of its own weights, ``ulp`` one bf16 ulp of the largest reference logit, and the
quantized steps may be off by ``2 * e_hip + ulp``.

Both arms prefill their prompt inside ``gemm.skinny_decode(fp8=qw)``, so the cached K / V of the prompt
come from the quantized weights like everything after them. ``generate`` prefills on the 16-bit
weights (``test_generate_with_quantized_graph`` does the same by hand); against the dequantized model
that would put the quantization error of the prompt's K / V into the comparison.

Models are those of ``test_decode_graph_gpu.py`` (context 128, 2 layers, d_model 256 / 4 heads and
160 / 2 heads) in bf16; every K is a multiple of 16.

Measured on an MI355X (e_hip / quantized steps / ulp / largest distance to the unquantized graph):
d_model 256: 2.03e-02 / 1.92e-02 / 1.56e-02 / 1.52e-01; d_model 160: 1.58e-02 / 1.61e-02 / 1.56e-02 /
1.39e-01. The quantized step is as close to its exact model as the bf16 forward is to its own, and
seven to nine times the bound away from the unquantized step."""

import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights
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
    with torch.no_grad(), gemm.skinny_decode(fp8=qw):
        return [m.forward_cached(tok, c) for c in caches]


@pytest.mark.parametrize("d_model,heads", MODELS)
def test_replay_equals_eager_and_error_against_the_dequantized_fp32_model(d_model, heads):
    dt = BF16
    m = _model(d_model, heads)
    qw = Fp8DecodeWeights(m)
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
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_fp8 {e_graph:.4e} ulp {ulp:.3e} "
          f"gap to the unquantized graph {gap:.4e}")
    assert e_graph <= 2 * e_hip + ulp, (e_graph, e_hip, ulp)
    # ... and it is not the unquantized step: on some step the logits differ by more than that bound
    assert gap > 2 * e_hip + ulp, (gap, e_hip, ulp)


def test_every_projection_runs_the_fp8_op():
    """Inside the step every projection (QKV, o, W1|W3, W2 per layer and the head) reaches
    ``cs336::gemm_skinny_w8``; the 16-bit skinny kernel, ``torch.mm`` and the references are never entered."""
    from cs336_systems.ops import skinny

    m = _model(160, 2, seed=2)
    qw = Fp8DecodeWeights(m)
    x = torch.randint(0, 500, (2, 12), device=DEV)
    cache, cache2 = KVCache(m, 2), KVCache(m, 2)
    with torch.no_grad():  # the prefills: the ordinary projections on the 16-bit weights
        m.forward_cached(x[:, :9], cache)
        m.forward_cached(x[:, :9], cache2)
    boom = AssertionError("a 16-bit or reference path ran inside the quantized step")
    with mock.patch.object(gemm, "skinny_w8_mm", wraps=gemm.skinny_w8_mm) as w8, \
            mock.patch.object(gemm, "skinny_mm", side_effect=boom) as sk, \
            mock.patch.object(torch, "mm", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_fp8_ref", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_ref", side_effect=boom):
        dg = DecodeGraph(m, cache, capture=True, warmup=1, weights=qw)
        calls = w8.call_count
        assert calls == 2 * (4 * 2 + 1)  # one warm-up step and the captured one
        for i in range(3):
            dg.step(x[:, 9 + i:10 + i])
        assert w8.call_count == calls  # replays launch the recorded kernels, not Python
        DecodeGraph(m, cache2, capture=False, weights=qw).step(x[:, 9:10])
        assert w8.call_count == calls + 4 * 2 + 1 and sk.call_count == 0
    assert cache.length == 12 and cache2.length == 10


def test_in_place_weight_update_refresh_and_reuse_after_reset():
    m = _model(160, 2, seed=3)
    qw = Fp8DecodeWeights(m)
    seq = torch.randint(0, 500, (3, 40), device=DEV)
    cg, ce = KVCache(m, 3), KVCache(m, 3)
    _prefill(m, qw, seq[:, :9], cg, ce)
    with torch.no_grad():
        dg = DecodeGraph(m, cg, weights=qw)
        de = DecodeGraph(m, ce, capture=False, weights=qw)
        for n in range(9, 14):
            assert torch.equal(dg.step(seq[:, n:n + 1]), de.step(seq[:, n:n + 1]))
        before = dg.step(seq[:, 14:15]).clone()
        de.step(seq[:, 14:15])
        ptrs = [(wq.data_ptr(), s.data_ptr()) for _, wq, s in qw._groups]
        for p in m.parameters():
            p.mul_(1.25)
        qw.refresh()  # in place: the captured kernels keep reading the same buffers
        assert ptrs == [(wq.data_ptr(), s.data_ptr()) for _, wq, s in qw._groups]
        got, want = dg.step(seq[:, 15:16]), de.step(seq[:, 15:16])
        assert torch.equal(got, want) and not torch.equal(got, before)
        assert _same_cache(cg, ce)
        # the same graph after reset() and a prefill of another length
        for c in (cg, ce):
            c.reset()
        _prefill(m, qw, seq[:, 20:25], cg, ce)
        assert cg.length == 5
        for n in range(25, 32):
            assert torch.equal(dg.step(seq[:, n:n + 1]), de.step(seq[:, n:n + 1])), n
        assert _same_cache(cg, ce)


def test_chunk_step_replay_equals_eager():
    m = _model(256, 4, seed=4)
    qw = Fp8DecodeWeights(m)
    seq = torch.randint(0, 500, (2, 40), device=DEV)
    cg, ce = KVCache(m, 2), KVCache(m, 2)
    _prefill(m, qw, seq[:, :8], cg, ce)
    with torch.no_grad(), mock.patch.object(gemm, "skinny_w8_mm", wraps=gemm.skinny_w8_mm) as w8:
        dg = DecodeGraph(m, cg, tokens=4, weights=qw)  # 8 rows per projection
        de = DecodeGraph(m, ce, capture=False, tokens=4, weights=qw)
        assert w8.call_count == 3 * (4 * 2 + 1)  # two warm-up steps and the captured one
        for n in range(8, 40, 4):
            got, want = dg.step(seq[:, n:n + 4]), de.step(seq[:, n:n + 4])
            assert got.shape == (2, 4, 500) and torch.equal(got, want), n
    assert cg.length == 40 and _same_cache(cg, ce)


def _sample_top1(logits):
    """``generate``'s own sampling at ``top_k=1`` (as in ``test_decode_graph_gpu.py``)."""
    from cs336_systems.models import softmax

    logits = logits[:, -1].float() / 1.0
    vals, _ = torch.topk(logits, 1)
    logits = logits.masked_fill(logits < vals[:, -1:], float("-inf"))
    return torch.multinomial(softmax(logits, dim=-1), 1)


def test_generate_with_quantized_graph():
    m = _model(256, 4, seed=1)
    qw = Fp8DecodeWeights(m)
    x = torch.randint(0, 500, (3, 9), device=DEV)
    torch.manual_seed(7)
    out = m.generate(x, 16, top_k=1, use_cache=True, graph=True, weights=qw)
    # the same kernels in a manual loop over the eager arm: a 16-bit prefill, then quantized steps
    cache = KVCache(m, 3)
    de = DecodeGraph(m, cache, capture=False, weights=qw)
    torch.manual_seed(7)
    with torch.no_grad():
        logits = m.forward_cached(x, cache)
        toks = []
        for _ in range(16):
            toks.append(_sample_top1(logits))
            if len(toks) < 16:
                logits = de.step(toks[-1])
    assert out.shape == (3, 16) and torch.equal(out, torch.cat(toks, dim=1))
    # a caller-owned quantized graph: its own weights are used
    dg = DecodeGraph(m, KVCache(m, 3), weights=qw)
    torch.manual_seed(7)
    assert torch.equal(m.generate(x, 16, top_k=1, use_cache=True, graph=dg), out)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, weights=qw)
    with pytest.raises(ValueError):
        DecodeGraph(m, KVCache(m, 3), capture=False, weights=Fp8DecodeWeights(_model(256, 4, seed=5)))
