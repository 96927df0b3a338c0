"""Chunk steps, ``DecodeGraph(tokens=n)`` and speculative decoding on the GPU (HIP kernels).

Yardstick and bound of ``test_generate_cache_gpu.py``: the fp32 full forward of the same weights on
the eager PyTorch backend; with ``e_hip`` the max logit error of the existing uncached HIP forward
against it, the chunked path must stay within ``2 * e_hip + ulp``. The speculative tests build their
models on the CPU generator (then move them), so the seed's greedy path is the one whose top-2 logit
gap was looked at when the seed was chosen: 2.6e-3 at its narrowest over the 119 steps, against fp32
path differences of 1e-5."""

import copy
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.models.speculative import speculative_generate

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


def _fp32_twin(m, d_model, heads):
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    return m32


@pytest.mark.parametrize("d_model,heads,dt", [(256, 4, BF16), (160, 2, BF16), (256, 4, F32)])
def test_teacher_forced_chunks_against_fp32(d_model, heads, dt):
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    m32 = _fp32_twin(m, d_model, heads)
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # logits at positions 8 .. 127
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 8:] - ref).abs().max().item()
        cache = KVCache(m, 2)
        rows = [m.forward_cached(seq[:, :9], cache)[:, -1:]]
        p, sizes = 9, [2, 8, 16, 5, 1, 9, 17, 3]
        while p < 128:
            n = min(sizes[len(rows) % len(sizes) - 1], 128 - p)
            rows.append(m.forward_cached(seq[:, p:p + n], cache, chunk=True))
            p += n
            assert cache.length == p and cache.lengths.tolist() == [p, p]
    chunked = torch.cat(rows, dim=1)
    assert chunked.dtype == dt and chunked.shape == ref.shape
    e_chunk = (chunked.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_chunk {e_chunk:.4e} ulp {ulp:.3e}")
    assert e_chunk <= 2 * e_hip + ulp, (e_chunk, e_hip, ulp)


def _same_cache(a, b, upto):
    return (a.length == b.length and torch.equal(a.lengths, b.lengths)
            and torch.equal(a.k[:, :, :, :upto], b.k[:, :, :, :upto]) and torch.equal(a.v[:, :, :, :upto], b.v[:, :, :, :upto]))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 5])
def test_decode_graph_tokens(n, batch):
    torch.manual_seed(3)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (batch, 128), device=DEV)
    cg, ce = KVCache(m, batch), KVCache(m, batch)
    with torch.no_grad():
        m.forward_cached(seq[:, :9], cg)
        m.forward_cached(seq[:, :9], ce)
        k0 = cg.k[:, :, :, :9].clone()
        dg = DecodeGraph(m, cg, capture=True, tokens=n)
        de = DecodeGraph(m, ce, capture=False, tokens=n)
        assert cg.length == 9 and cg.lengths.tolist() == [9] * batch and torch.equal(cg.k[:, :, :, :9], k0)
        p = 9
        for _ in range(4):
            got, want = dg.step(seq[:, p:p + n]), de.step(seq[:, p:p + n])
            assert got.shape == (batch, n, 500) and got.dtype == BF16
            assert torch.equal(got, want), p
            p += n
        assert _same_cache(cg, ce, p)
        # rejected tokens are forgotten in place; the graph goes on from the shorter cache
        for c in (cg, ce):
            c.truncate(p - n - 1)
        p = p - n - 1
        for _ in range(2):
            assert torch.equal(dg.step(seq[:, p:p + n]), de.step(seq[:, p:p + n])), p
            p += n
        assert _same_cache(cg, ce, p)
        # the same graph after reset() and a prefill of another length
        for c in (cg, ce):
            c.reset()
            m.forward_cached(seq[:, 40:47], c)
        p = 47
        for _ in range(2):
            assert torch.equal(dg.step(seq[:, p:p + n]), de.step(seq[:, p:p + n])), p
            p += n
        assert _same_cache(cg, ce, 7 + 2 * n)
        # checks: a wrong width, and too few slots left (nothing changes)
        with pytest.raises(ValueError):
            dg.step(seq[:, :n + 1])
        for c in (cg, ce):
            c.reset()
            m.forward_cached(seq[:, :128 - n + 1], c)
        before = cg.k.clone()
        for d in (dg, de):
            with pytest.raises(ValueError):
                d.step(seq[:, :n])
        assert cg.length == 128 - n + 1 and torch.equal(cg.k, before)


def _spec_models(dt):
    """Target and noisy draft, initialised on the CPU generator (reproducible across devices)."""
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(256, 4)).eval()
    x = torch.randint(0, 500, (2, 9))
    noisy = copy.deepcopy(m)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in noisy.parameters():
            if p.dim() > 1:
                p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.08)
    return m.to(DEV).to(dt).eval(), noisy.to(DEV).to(dt).eval(), x.to(DEV)


@pytest.fixture(scope="module")
def fp32_spec():
    m, noisy, x = _spec_models(F32)
    with torch.no_grad():
        want = m.generate(x, 119, top_k=1, use_cache=True)  # the existing stepwise path, to the window's end
        seq = torch.cat((x, want), dim=1)
        logits = m(seq)[:, 8:-1].float()
    top2 = torch.topk(logits, 2).values
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"greedy path: min top-2 logit gap {gap:.3e}")
    assert gap > 1e-3, gap
    return m, noisy, x, want


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("which", ["self", "noisy"])
def test_speculative_fp32_equals_greedy(fp32_spec, which, graph):
    m, noisy, x, want = fp32_spec
    out, st = speculative_generate(m, m if which == "self" else noisy, x, 119, draft_tokens=4, graph=graph)
    print(f"{which} draft, graph {graph}: {st}")
    assert torch.equal(out, want)
    if which == "self":
        assert st["accepted"] == st["proposed"] > 0
    out = m.generate(x, 30, top_k=1, use_cache=True, draft=noisy, draft_tokens=7, graph=graph)
    assert torch.equal(out, want[:, :30])


@pytest.mark.parametrize("graph", [False, True])
def test_speculative_bf16_tokens_are_near_argmax(graph):
    """No equality claim in bf16 (ties can flip between kernels): every emitted token was the argmax
    of logits that lie within E = 2 * e_hip + ulp of the fp32 eager logits ``ref``, so
    ``max(ref) - ref[token] <= 2 E``."""
    m, noisy, x = _spec_models(BF16)
    m32 = _fp32_twin(m, 256, 4)
    with torch.no_grad():
        out, st = speculative_generate(m, noisy, x, 119, draft_tokens=4, graph=graph)
        assert out.shape == (2, 119)
        seq = torch.cat((x, out), dim=1)
        with ops.backend("torch"):
            ref = m32(seq).double()[:, 8:-1]  # the logits each emitted token was chosen from
        e_hip = (m(seq).double()[:, 8:-1] - ref).abs().max().item()
    E = 2 * e_hip + _ulp(BF16, ref.abs().max().item())
    short = (ref.max(dim=-1).values - ref.gather(-1, out[..., None]).squeeze(-1)).max().item()
    print(f"bf16 graph {graph}: {st} e_hip {e_hip:.4e} E {E:.4e} worst max(ref) - ref[token] {short:.4e}")
    assert short <= 2 * E, (short, E)
