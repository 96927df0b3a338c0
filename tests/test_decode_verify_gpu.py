"""Verify attention (``csrc/flash_attn/fa_verify.hip``) on the GPU: the 16-query MFMA tile on dense and
paged caches, ``verify_cached``, ``DecodeGraph(verify=True)`` and paged speculative decoding.

Oracle, cases and checks are those of ``test_decode_extend_gpu.py`` (imported): fp64 attention of every query over its own key prefix
from the same rounded inputs, cache rows at and beyond ``kv_len[b]`` NaN, max |o - ref| < 2e-2 and
max |lse - ref| < 2e-2 on the finite entries, an exact finiteness pattern of the LSE and o == 0 where
lse = -inf. The model tests use ``e_verify <= 2 * e_hip + ulp`` against the fp32 eager forward."""

import copy

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.decode_graph import Sampler
from cs336_systems.models.speculative import speculative_generate

from .test_decode_extend_gpu import (BF16, DEV, DIMS, DTYPES, F16, KV_SETS, SPLITS, _case, _cfg, _check, _fp32_ref,
                                     _new_cache, _paginate, _ulp)

pytestmark = pytest.mark.gpu

NS = [1, 5, 16, 17, 33]  # one query, a partial tile, a full tile, a one-row tail in the second tile, three tiles


def _kv_len(kv_set, n):
    # a chunk on an empty cache; a full 128-key workgroup tile, a 32-key sub-tile edge and the cache end;
    # queries with no key at all
    return {"empty": (n, n + 1, 300), "edges": (128, 160, 320), "short": (0, 3, n - 1)}[kv_set]


def _grid():
    """20 of the 120 (dtype, n, kv set, splits) points per head dim, shifted per head dim; every value of
    every axis meets every head dim (checked below)."""
    cases = []
    for di, d in enumerate(DIMS):
        mine = {(DTYPES[(i + i // 5) % 2], NS[i % 5], KV_SETS[(i // 2 + di) % 3], SPLITS[(i + i // 5 + di) % 4])
                for i in range(20)}
        for axis, vals in enumerate((DTYPES, NS, KV_SETS, SPLITS)):
            assert {c[axis] for c in mine} == set(vals), (d, axis)
        cases += [(d, *c) for c in sorted(mine, key=str)]
    return cases


@pytest.mark.parametrize("d,dt,n,kv_set,splits", _grid())
def test_verify_attention_grid(d, dt, n, kv_set, splits):
    kv_len = _kv_len(kv_set, n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    o, lse = ops.verify_attention(q, k, v, lens, splits=splits)
    if kv_set == "short":
        assert not torch.isfinite(ref_l[0]).any() and not torch.isfinite(ref_l[1, :max(n - 3, 0)]).any()
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} n{n} {kv_len} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("n", [5, 17])
def test_peaky(n, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k, v, lens, ref_o, ref_l = _case(BF16, 64, n, _kv_len("empty", n), 8.0)
    o, lse = ops.verify_attention(q, k, v, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, BF16, f"peaky n{n} splits {splits}:")


@pytest.mark.parametrize("d,dt,n,kv_set", [(64, BF16, 33, "empty"), (80, F16, 16, "edges"), (128, BF16, 17, "short"),
                                           (32, F16, 5, "edges")])
@pytest.mark.parametrize("P", [16, 64])
def test_paged(P, d, dt, n, kv_set):
    kv_len = _kv_len(kv_set, n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    kp, vp, table = _paginate(k, v, kv_len, P, 1)
    kp2, vp2, table2 = _paginate(k, v, kv_len, P, 2)
    assert not torch.equal(table, table2)
    o, lse = ops.verify_attention_paged(q, kp, vp, table, lens)
    _check(o, lse, ref_o, ref_l, dt, f"paged P{P} {dt} d{d} n{n} {kv_len}:")
    for splits in (1, 2, 5):  # the bits of the dense kernel on the same rows, whatever the placement
        o1, l1 = ops.verify_attention_paged(q, kp, vp, table, lens, splits=splits)
        o2, l2 = ops.verify_attention_paged(q, kp2, vp2, table2, lens, splits=splits)
        od, ld = ops.verify_attention(q, k, v, lens, splits=splits)
        assert torch.equal(o1, od) and torch.equal(l1, ld), splits
        assert torch.equal(o1, o2) and torch.equal(l1, l2), splits


# ---- model ----
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d_model,heads", [(256, 4), (160, 2)])
def test_verify_cached_against_fp32(d_model, heads, paged):
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (2, 52), device=DEV)
    ref = _fp32_ref(m, _cfg(d_model, heads), seq)
    with torch.no_grad():
        e_hip = (m(seq).double() - ref).abs().max().item()
        cache = _new_cache(m, 2, paged)
        out = [m.verify_cached(seq[:, a:b], cache) for a, b in ((0, 5), (5, 12), (12, 28), (28, 52))]
    assert cache.length == 52 and cache.lengths.tolist() == [52, 52]
    e_ver = (torch.cat(out, dim=1).double() - ref).abs().max().item()
    ulp = _ulp(BF16, ref.abs().max().item())
    print(f"d_model {d_model} paged {paged}: e_hip {e_hip:.4e} e_verify {e_ver:.4e} ulp {ulp:.3e}")
    assert e_ver <= 2 * e_hip + ulp, (e_ver, e_hip, ulp)


@pytest.mark.parametrize("paged", [False, True])
def test_decode_graph_verify(paged):
    """Several replays of the captured 4-token verify step equal the eager step bitwise, also after a
    truncate (rejected proposals) in between."""
    torch.manual_seed(3)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (2, 64), device=DEV)
    cg, ce = _new_cache(m, 2, paged), _new_cache(m, 2, paged)
    with torch.no_grad():
        for c in (cg, ce):
            m.forward_cached(seq[:, :9], c)
        dg = DecodeGraph(m, cg, capture=True, tokens=4, verify=True)
        de = DecodeGraph(m, ce, capture=False, tokens=4, verify=True)
        p = 9
        for i in range(5):
            got, want = dg.step(seq[:, p:p + 4]), de.step(seq[:, p:p + 4])
            assert got.shape == (2, 4, 500) and torch.equal(got, want), p
            p += 4
            if i == 2:
                p -= 3
                cg.truncate(p)
                ce.truncate(p)
    assert cg.length == ce.length == p and cg.lengths.tolist() == [p, p]
    with pytest.raises(ValueError):
        DecodeGraph(m, cg, capture=False, tokens=1, verify=True, sampler=Sampler())


@pytest.mark.parametrize("graph", [False, True])
def test_speculative_paged_bf16_tokens_are_near_argmax(graph):
    """The rule of ``test_generate_chunk_gpu.py``: every emitted token was the argmax of logits within
    E = 2 * e_hip + ulp of the fp32 eager logits ``ref``, so ``max(ref) - ref[token] <= 2 E``."""
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(256, 4)).eval()
    x = torch.randint(0, 500, (2, 9)).to(DEV)
    noisy = copy.deepcopy(m)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in noisy.parameters():
            if p.dim() > 1:
                p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.08)
    m, noisy = m.to(DEV).to(BF16).eval(), noisy.to(DEV).to(BF16).eval()
    with torch.no_grad():
        out, st = speculative_generate(m, noisy, x, 119, draft_tokens=4, graph=graph, verify="mfma", paged=True,
                                       page_size=16)
        assert out.shape == (2, 119) and st["rounds"] > 0
        seq = torch.cat((x, out), dim=1)
        ref = _fp32_ref(m, _cfg(256, 4), seq)[:, 8:-1]  # the logits each emitted token was chosen from
        e_hip = (m(seq).double()[:, 8:-1] - ref).abs().max().item()
    E = 2 * e_hip + _ulp(BF16, ref.abs().max().item())
    short = (ref.max(dim=-1).values - ref.gather(-1, out[..., None]).squeeze(-1)).max().item()
    print(f"bf16 paged graph {graph}: {st} e_hip {e_hip:.4e} E {E:.4e} worst max(ref) - ref[token] {short:.4e}")
    assert short <= 2 * E, (short, E)
