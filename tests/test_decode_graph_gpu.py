"""``DecodeGraph`` on the GPU: a captured and replayed decode step against the same step run eagerly
(``capture=False``) on a second cache, bit for bit, and against the fp32 eager forward with the
yardstick and bound of ``test_generate_cache_gpu.py`` (``2 * e_hip + ulp``).

Models are those of ``test_generate_cache_gpu.py`` (context 128, 2 layers, d_model 256 / 4 heads and
160 / 2 heads: head dims 64 and 80) in bf16, plus one fp32 model whose projections take the fallback
GEMM inside the capture. At these cache lengths ``fa_decode_splits`` gives 1 for every bound, so both
arms run identical launches."""

import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import gemm

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
MODELS = [(256, 4, BF16), (160, 2, BF16), (256, 4, F32)]


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


def _model(d_model, heads, dt, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()


def _same_cache(a, b):
    return (a.length == b.length and torch.equal(a.lengths, b.lengths) and torch.equal(a.k, b.k)
            and torch.equal(a.v, b.v))


@pytest.mark.parametrize("d_model,heads,dt", MODELS)
def test_replay_equals_eager_and_error_against_fp32(d_model, heads, dt):
    m = _model(d_model, heads, dt)
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # logits at positions 8 .. 127
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 8:] - ref).abs().max().item()
        cg, ce = KVCache(m, 2), KVCache(m, 2)
        first = m.forward_cached(seq[:, :9], cg)[:, -1]
        m.forward_cached(seq[:, :9], ce)
        # construction leaves the prefilled cache as it found it
        k0, v0 = cg.k[:, :, :, :9].clone(), cg.v[:, :, :, :9].clone()
        dg = DecodeGraph(m, cg, capture=True, warmup=2)
        assert cg.length == 9 and cg.lengths.tolist() == [9, 9]
        assert torch.equal(cg.k[:, :, :, :9], k0) and torch.equal(cg.v[:, :, :, :9], v0)
        de = DecodeGraph(m, ce, capture=False)
        rows = [first]
        for n in range(9, 128):  # 119 teacher-forced steps
            got = dg.step(seq[:, n:n + 1])
            want = de.step(seq[:, n:n + 1])
            assert got.shape == (2, 1, 500) and got.dtype == dt
            assert torch.equal(got, want), n
            rows.append(got[:, -1].clone())  # the static buffer is overwritten by the next step
    assert cg.length == 128 and cg.lengths.tolist() == [128, 128] and _same_cache(cg, ce)
    graphed = torch.stack(rows, dim=1)
    e_graph = (graphed.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_graph {e_graph:.4e} ulp {ulp:.3e}")
    assert e_graph <= 2 * e_hip + ulp, (e_graph, e_hip, ulp)
    # a full cache raises on the host and changes nothing
    before = cg.k.clone()
    with pytest.raises(ValueError):
        dg.step(seq[:, :1])
    assert cg.length == 128 and cg.lengths.tolist() == [128, 128] and torch.equal(cg.k, before)


def test_reuse_after_reset_and_in_place_weight_update():
    m = _model(160, 2, BF16, seed=3)
    seq = torch.randint(0, 500, (3, 40), device=DEV)
    cg, ce = KVCache(m, 3), KVCache(m, 3)
    with torch.no_grad():
        m.forward_cached(seq[:, :9], cg)
        m.forward_cached(seq[:, :9], ce)
        dg, de = DecodeGraph(m, cg), DecodeGraph(m, ce, capture=False)
        for n in range(9, 14):
            assert torch.equal(dg.step(seq[:, n:n + 1]), de.step(seq[:, n:n + 1]))
        # the same graph after reset() and a prefill of another length
        for c in (cg, ce):
            c.reset()
            m.forward_cached(seq[:, 20:25], c)
        assert cg.length == 5
        for n in range(25, 32):
            assert torch.equal(dg.step(seq[:, n:n + 1]), de.step(seq[:, n:n + 1])), n
        assert _same_cache(cg, ce)
        # in-place weight updates are picked up by the next replay
        before = dg.step(seq[:, 32:33]).clone()
        de.step(seq[:, 32:33])
        for p in m.parameters():
            p.mul_(1.25)
        got, want = dg.step(seq[:, 33:34]), de.step(seq[:, 33:34])
        assert torch.equal(got, want) and not torch.equal(got, before)
        assert _same_cache(cg, ce)


def _sample_top1(logits):
    """``generate``'s own sampling at ``top_k=1`` (a tie between two bf16 logits is drawn, not ranked:
    with the same seed and the same logits both loops draw the same token)."""
    from cs336_systems.models import softmax

    logits = logits[:, -1].float() / 1.0
    vals, _ = torch.topk(logits, 1)
    logits = logits.masked_fill(logits < vals[:, -1:], float("-inf"))
    return torch.multinomial(softmax(logits, dim=-1), 1)


@pytest.mark.parametrize("batch", [1, 3])
def test_generate_with_graph(batch):
    m = _model(256, 4, BF16, seed=1)
    x = torch.randint(0, 500, (batch, 9), device=DEV)
    torch.manual_seed(7)
    out = m.generate(x, 40, top_k=1, use_cache=True, graph=True)
    # the same kernels in a manual loop over the eager arm: the same tokens
    cache = KVCache(m, batch)
    de = DecodeGraph(m, cache, capture=False)
    torch.manual_seed(7)
    with torch.no_grad():
        logits = m.forward_cached(x, cache)
        toks = []
        for _ in range(40):
            toks.append(_sample_top1(logits))
            if len(toks) < 40:
                logits = de.step(toks[-1])
    assert out.shape == (batch, 40) and torch.equal(out, torch.cat(toks, dim=1))
    # past the window the uncached sliding step takes over
    torch.manual_seed(7)
    long = m.generate(x, 125, top_k=1, use_cache=True, graph=True)
    assert long.shape == (batch, 125) and long.dtype == torch.int64 and torch.equal(long[:, :40], out)
    # a caller-owned graph, reused over two calls
    dg = DecodeGraph(m, KVCache(m, batch))
    for _ in range(2):
        torch.manual_seed(7)
        assert torch.equal(m.generate(x, 40, top_k=1, use_cache=True, graph=dg), out)
    with pytest.raises(ValueError):
        m.generate(torch.cat((x, x)), 4, top_k=1, use_cache=True, graph=dg)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, graph=True)


def test_graphed_step_runs_the_hip_ops():
    """Inside the step every projection (QKV, o, W1|W3, W2 per layer and the head) reaches
    ``cs336::gemm_skinny``; the eager references are never entered."""
    from cs336_systems.ops import decode as dec
    from cs336_systems.ops import skinny

    m = _model(160, 2, BF16, seed=2)
    x = torch.randint(0, 500, (2, 12), device=DEV)
    cache = KVCache(m, 2)
    cache2 = KVCache(m, 2)
    with torch.no_grad():  # the prefills: the ordinary projections
        m.forward_cached(x[:, :9], cache)
        m.forward_cached(x[:, :9], cache2)
    boom = AssertionError("the eager reference ran on the GPU path")
    with mock.patch.object(gemm, "skinny_mm", wraps=gemm.skinny_mm) as sk, \
            mock.patch.object(torch, "mm", side_effect=boom), \
            mock.patch.object(skinny, "skinny_linear_ref", side_effect=boom), \
            mock.patch.object(dec, "decode_attention_ref", side_effect=boom), \
            mock.patch.object(dec, "kv_append_rope_ref", side_effect=boom):
        dg = DecodeGraph(m, cache, capture=True, warmup=1)
        calls = sk.call_count
        assert calls == 2 * (4 * 2 + 1)  # one warm-up step and the captured one
        for i in range(3):
            dg.step(x[:, 9 + i:10 + i])
        assert sk.call_count == calls  # replays launch the recorded kernels, not Python
        DecodeGraph(m, cache2, capture=False).step(x[:, 9:10])
        assert sk.call_count == calls + 4 * 2 + 1
    assert cache.length == 12 and cache2.length == 10
