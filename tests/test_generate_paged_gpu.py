"""``forward_cached``, ``DecodeGraph`` and ``generate`` on a ``PagedKVCache`` on the GPU (HIP kernels:
``csrc/flash_attn/fa_decode_paged.hip``).

Teacher-forced error by the rule of ``test_generate_cache_gpu.py``: with ``e_hip`` the max logit error
of the uncached HIP forward against the fp32 eager forward of the same weights, the paged path
(prefill 9 + steps to 128, page size 16) stays within ``2 * e_hip + ulp``. The graph is held bitwise
to its eager arm (``capture=False``), as in ``test_decode_graph_gpu.py``."""

import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, PagedKVCache, Sampler

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 16


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _model(d_model=256, heads=4, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(torch.bfloat16).eval()


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _state(cache):
    return cache.block_table.tolist(), cache.lengths.tolist(), cache.seq_lengths, list(cache._pool.free)


@pytest.mark.parametrize("d_model,heads,dt", [(256, 4, torch.bfloat16), (160, 2, torch.bfloat16), (256, 4, torch.float32)])
def test_teacher_forced_error_against_fp32(d_model, heads, dt):
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # logits at positions 8 .. 127
    with torch.no_grad():
        full = m(seq)
        e_hip = (full.double()[:, 8:] - ref).abs().max().item()
        cache = PagedKVCache(m, 2, page_size=P)
        assert cache.dtype == dt
        rows = [m.forward_cached(seq[:, :9], cache)[:, -1]]
        for n in range(9, 128):
            rows.append(m.forward_cached(seq[:, n:n + 1], cache)[:, -1])
        assert cache.length == 128 and cache.lengths.tolist() == [128, 128] and cache.pages_free == 0
    cached = torch.stack(rows, dim=1)
    assert cached.dtype == dt and cached.shape == ref.shape
    e_paged = (cached.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_paged {e_paged:.4e} ulp {ulp:.3e} "
          f"max|ref| {ref.abs().max().item():.3f}")
    assert e_paged <= 2 * e_hip + ulp, (e_paged, e_hip, ulp)


def test_paged_step_runs_the_hip_ops():
    """Every step calls the two paged ops once per layer, and they go to ``cs336::fa_decode_paged`` /
    ``cs336::kv_append_rope_paged`` (the eager references are never entered)."""
    from cs336_systems.ops import decode as dec

    m = _model(160, 2, seed=2)
    x = torch.randint(0, 500, (2, 12), device=DEV)
    cache = PagedKVCache(m, 2, page_size=P)
    boom = AssertionError("the eager reference ran on the GPU path")
    launched = []
    hip_paged = torch.ops.cs336.fa_decode_paged

    def spy(*a, **k):
        launched.append(1)
        return hip_paged(*a, **k)

    with mock.patch.object(ops, "decode_attention_paged", wraps=ops.decode_attention_paged) as att, \
            mock.patch.object(ops, "kv_append_rope_paged", wraps=ops.kv_append_rope_paged) as app, \
            mock.patch.object(dec, "decode_attention_paged_ref", side_effect=boom), \
            mock.patch.object(dec, "kv_append_rope_paged_ref", side_effect=boom), \
            mock.patch.object(dec, "decode_attention_ref", side_effect=boom), \
            mock.patch.object(dec, "ops", return_value=mock.Mock(wraps=torch.ops.cs336, fa_decode_paged=spy)):
        m.forward_cached(x[:, :9], cache)
        assert att.call_count == 0 and app.call_count == 0  # the prefill is the ordinary attention
        for i in range(3):
            m.forward_cached(x[:, 9 + i:10 + i], cache)
            assert att.call_count == 2 * (i + 1) and app.call_count == 2 * (i + 1)
    assert len(launched) == 6 and cache.length == 12


@pytest.mark.parametrize("B", [1, 3])
def test_graph_replay_equals_eager_bitwise(B):
    m = _model()
    prompt = torch.randint(0, 500, (B, 9), device=DEV)
    toks = torch.randint(0, 500, (B, 30), device=DEV)
    cg, ce = PagedKVCache(m, B, page_size=P), PagedKVCache(m, B, page_size=P)
    with torch.no_grad():
        m.forward_cached(prompt, cg)
        m.forward_cached(prompt, ce)
    before = _state(cg)
    dg = DecodeGraph(m, cg, capture=True)
    assert _state(cg) == before  # warm-up and capture leave table, lengths and free list as found
    de = DecodeGraph(m, ce, capture=False)
    for i in range(30):  # slots 9 .. 38: two page boundaries
        assert torch.equal(dg.step(toks[:, i:i + 1]), de.step(toks[:, i:i + 1])), i
    assert cg.length == ce.length == 39 and cg.lengths.tolist() == [39] * B and cg.pages_in_use == 3 * B
    kg, vg = cg.gather()
    ke, ve = ce.gather()
    assert torch.equal(kg, ke) and torch.equal(vg, ve)
    # the same graph after reset() and a prompt of another length
    cg.reset()
    ce.reset()
    assert cg.pages_in_use == 0
    prompt = torch.randint(0, 500, (B, 20), device=DEV)
    with torch.no_grad():
        m.forward_cached(prompt, cg)
        m.forward_cached(prompt, ce)
    for i in range(14):
        assert torch.equal(dg.step(toks[:, i:i + 1]), de.step(toks[:, i:i + 1])), i
    with pytest.raises(NotImplementedError):
        DecodeGraph(m, PagedKVCache(m, B, page_size=P), capture=False, tokens=2)


@pytest.mark.parametrize("fp8w", [False, True])
def test_sampled_graph_on_paged_cache(fp8w):
    """``sampler=`` (and ``weights=``) on a paged cache: ``advance`` reads nothing back although it
    reserves pages on the way, and emits the eager arm's tokens."""
    B = 3
    m = _model()
    sampler = Sampler(0.9, 20)
    qw = Fp8DecodeWeights(m) if fp8w else None
    prompt = torch.randint(0, 500, (B, 9), device=DEV)
    table = torch.rand(30, B, device=DEV, generator=_gen(1))
    cg, ce = PagedKVCache(m, B, page_size=P), PagedKVCache(m, B, page_size=P)
    with torch.no_grad():
        first = ops.sample_logits(m.forward_cached(prompt, cg)[:, -1], table[0], 0.9, 20)[:, None]
        m.forward_cached(prompt, ce)
    before = _state(cg)
    dg = DecodeGraph(m, cg, capture=True, weights=qw, sampler=sampler)
    assert _state(cg) == before
    de = DecodeGraph(m, ce, capture=False, weights=qw, sampler=sampler)
    dg.begin(first, 30, table=table)
    de.begin(first, 30, table=table)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dg.advance(29)  # slots 9 .. 37: pages are reserved at 16 and 32
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    de.advance(29)
    assert cg.length == 38 and cg.pages_in_use == 3 * B
    assert dg.tokens().shape == (B, 30) and torch.equal(dg.tokens(), de.tokens())


def test_generate_paged_with_graph():
    B = 3
    m = _model(seed=1)
    x = torch.randint(0, 500, (B, 9), device=DEV)
    dense = m.generate(x, 40, top_k=1, use_cache=True, graph=True)
    out = m.generate(x, 40, top_k=1, use_cache=True, graph=True, paged=True, page_size=P)
    assert out.shape == dense.shape and out.dtype == dense.dtype and out.is_cuda
    # the same kernels in a manual loop over the eager paged step: the same tokens
    cache = PagedKVCache(m, B, page_size=P)
    de = DecodeGraph(m, cache, capture=False)
    with torch.no_grad():
        logits = m.forward_cached(x, cache)
        toks = []
        for _ in range(40):
            toks.append(logits[:, -1].float().argmax(dim=-1, keepdim=True))
            if len(toks) < 40:
                logits = de.step(toks[-1])
    assert torch.equal(out, torch.cat(toks, dim=1))
    # past the window the uncached sliding step takes over
    long = m.generate(x, 125, top_k=1, use_cache=True, graph=True, paged=True, page_size=P)
    assert long.shape == (B, 125) and torch.equal(long[:, :40], out)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, paged=True, kv_fp8=True)


def test_share_prompt_stores_the_prompt_once():
    B, n_prompt = 4, 40
    m = _model(seed=3)
    x = torch.randint(0, 500, (1, n_prompt), device=DEV).expand(B, -1).contiguous()
    dg = DecodeGraph(m, PagedKVCache(m, B, page_size=P))
    out = m.generate(x, 10, top_k=1, use_cache=True, graph=dg, share_prompt=True)
    cache = dg.cache
    assert cache.length == n_prompt + 9
    # 2 shared full pages; per row the copied tail page and one more for slots 48 ...
    assert cache.pages_in_use == 2 + 2 * B < B * 4
    k, v = cache.gather()
    for b in range(1, B):
        assert torch.equal(k[:, b, :, :n_prompt], k[:, 0, :, :n_prompt])
        assert torch.equal(v[:, b, :, :n_prompt], v[:, 0, :, :n_prompt])
    assert out.shape == (B, 10)
    with pytest.raises(ValueError):
        y = x.clone()
        y[2, 5] = (y[2, 5] + 1) % 500
        m.generate(y, 4, top_k=1, use_cache=True, graph=dg, share_prompt=True)


def test_shared_rows_diverge_without_disturbing_each_other():
    """Rows forked from one prompt sample different continuations from their own columns of the table,
    and row 0's tokens are those of a B = 1 run on column 0."""
    B, n_prompt, steps = 4, 21, 30
    m = _model(seed=4)
    sampler = Sampler(1.0, 50)
    prompt = torch.randint(0, 500, (1, n_prompt), device=DEV)
    table = torch.rand(steps, B, device=DEV, generator=_gen(5))

    def run(batch, tab):
        cache = PagedKVCache(m, batch, page_size=P)
        with torch.no_grad():
            logits = m.forward_cached(prompt, cache.row(0))[:, -1]
        cache.fork(0)
        first = ops.sample_logits(logits.expand(batch, -1).contiguous(), tab[0].contiguous(), 1.0, 50)[:, None]
        dg = DecodeGraph(m, cache, capture=True, sampler=sampler)
        dg.begin(first, steps, table=tab.contiguous())
        dg.advance(steps - 1)
        return dg.tokens(), cache

    toks, cache = run(B, table)
    one, _ = run(1, table[:, :1])
    assert len({tuple(r.tolist()) for r in toks}) > 1  # the rows did diverge
    assert torch.equal(toks[:1], one)
    assert cache.pages_in_use == 1 + 3 * B  # the shared full page; the tail copy and two more pages per row
