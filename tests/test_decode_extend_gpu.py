"""Extend attention (``csrc/flash_attn/fa_extend.hip``) on the GPU: the MFMA kernel on dense and paged
caches, ``extend_cached`` and ``generate(prefill_chunk=)``.

Oracle: fp64 attention of every query over its own key prefix ``[0, kv_len[b] - (n - 1 - i))`` from the
same rounded inputs; cache rows at and beyond ``kv_len[b]`` are NaN. Tolerances are the decode family's:
max |o - ref| < 2e-2, max |lse - ref| < 2e-2 on the finite entries, an exact finiteness pattern of the LSE
and o == 0 where lse = -inf. The model tests use the rule of ``test_generate_chunk_gpu.py``: against the
fp32 eager forward of the same weights, ``e_extend <= 2 * e_hip + ulp``."""

import functools
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM
from cs336_systems.models.kv_cache import KVCache, PagedKVCache

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, MAX_LEN = 3, 3, 320
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16]
DIMS = [32, 64, 80, 128]
NS = [1, 17, 64, 65, 129]  # below a wave's rows, inside a tile, a full 64, one past it, past 128 with a one-row tail
KV_SETS = ["empty", "edges", "short"]
SPLITS = [0, 1, 2, 5]
TOL = 2e-2


def _kv_len(kv_set, n):
    # a chunk on an empty cache; key-tile edges and the cache end; queries with no key at all
    return {"empty": (n, n + 1, max(300, n)), "edges": (max(64, n), max(128, n), 320), "short": (0, 3, n - 1)}[kv_set]


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


def _oracle(q, k, v, kv_len, scale):
    """fp64 attention of each query over its own key prefix only (NaN tails never touched)."""
    n, N = q.shape[1], k.shape[2]
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, kv in enumerate(kv_len):
        L = min(max(kv, 0), N)  # the last query's prefix holds every other one
        if L == 0:
            continue
        bound = (kv - torch.arange(n - 1, -1, -1, device=q.device)).clamp(0, N)
        s = torch.einsum("nhd,hkd->nhk", q[b].double(), k[b, :, :L].double()) * scale
        s = s.masked_fill(torch.arange(L, device=q.device)[None, None, :] >= bound[:, None, None], float("-inf"))
        lse[b] = torch.logsumexp(s, -1)
        p = torch.exp(s - torch.where(torch.isinf(lse[b]), 0.0, lse[b])[..., None])
        o[b] = torch.einsum("nhk,hkd->nhd", p, v[b, :, :L].double())
    return o, lse


@functools.lru_cache(maxsize=None)
def _case(dt, d, n, kv_len, qmul=1.0):
    """Inputs and their oracle, built once per case and shared by every split count; nothing modifies them."""
    g = torch.Generator(device=DEV).manual_seed(977 + d + n)
    q = (torch.randn(B, n, H, d, device=DEV, generator=g) * qmul).to(dt)
    k = torch.randn(B, H, MAX_LEN, d, device=DEV, generator=g).to(dt)
    v = torch.randn(B, H, MAX_LEN, d, device=DEV, generator=g).to(dt)
    for b, kv in enumerate(kv_len):
        k[b, :, kv:] = float("nan")
        v[b, :, kv:] = float("nan")
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    return (q, k, v, lens) + _oracle(q, k, v, kv_len, 1.0 / math.sqrt(d))


def _check(o, lse, ref_o, ref_l, dt, what=""):
    assert o.dtype == dt and lse.dtype == F32 and o.shape == ref_o.shape and lse.shape == ref_l.shape
    assert torch.isfinite(o).all(), what
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(lse), fin) and (lse[~fin] < 0).all(), what
    assert torch.equal(o[~fin], torch.zeros_like(o[~fin])), what  # a query with no key: o = 0
    eo = (o.double() - ref_o).abs().max().item()
    el = (lse.double()[fin] - ref_l[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what} max|o-ref| {eo:.3e} max|lse-ref| {el:.3e}")
    assert eo < TOL and el < TOL, (what, eo, el)


@pytest.mark.parametrize("d,dt,n,kv_set,splits", _grid())
def test_extend_attention_grid(d, dt, n, kv_set, splits):
    kv_len = _kv_len(kv_set, n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    o, lse = ops.extend_attention(q, k, v, lens, splits=splits)
    if kv_set == "short":
        assert not torch.isfinite(ref_l[0]).any() and not torch.isfinite(ref_l[1, :n - 3]).any()
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} n{n} {kv_len} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("n", [17, 129])
@pytest.mark.parametrize("dt", DTYPES)
def test_peaky(dt, n, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k, v, lens, ref_o, ref_l = _case(dt, 64, n, _kv_len("empty", n), 8.0)
    o, lse = ops.extend_attention(q, k, v, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, dt, f"peaky {dt} n{n} splits {splits}:")


def _paginate(k, v, kv_len, P, seed):
    """The dense rows of ``_case`` in pages of a seeded random permutation: table entries past each
    sequence's pages are -1 and pages no sequence owns are NaN."""
    T = MAX_LEN // P
    perm = torch.randperm(B * T + 3, generator=torch.Generator().manual_seed(seed)).tolist()
    kp = torch.full((B * T + 3, H, P, k.shape[-1]), float("nan"), device=DEV, dtype=k.dtype)
    vp = torch.full_like(kp, float("nan"))
    table = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    for b, kv in enumerate(kv_len):
        for t in range(-(-kv // P)):
            page = perm.pop()
            table[b, t] = page
            kp[page] = k[b, :, t * P:(t + 1) * P]
            vp[page] = v[b, :, t * P:(t + 1) * P]
    return kp, vp, table


@pytest.mark.parametrize("d,dt,n,kv_set", [(64, BF16, 129, "empty"), (80, F16, 17, "edges"), (128, BF16, 65, "short"),
                                           (32, F16, 64, "edges")])
@pytest.mark.parametrize("P", [16, 64])
def test_paged(P, d, dt, n, kv_set):
    kv_len = _kv_len(kv_set, n)
    q, k, v, lens, ref_o, ref_l = _case(dt, d, n, kv_len)
    kp, vp, table = _paginate(k, v, kv_len, P, 1)
    kp2, vp2, table2 = _paginate(k, v, kv_len, P, 2)
    assert not torch.equal(table, table2) or max(kv_len) == 0
    o, lse = ops.extend_attention_paged(q, kp, vp, table, lens)
    _check(o, lse, ref_o, ref_l, dt, f"paged P{P} {dt} d{d} n{n} {kv_len}:")
    for splits in (1, 2, 5):  # the bits of the dense kernel on the same rows, whatever the placement
        o1, l1 = ops.extend_attention_paged(q, kp, vp, table, lens, splits=splits)
        o2, l2 = ops.extend_attention_paged(q, kp2, vp2, table2, lens, splits=splits)
        od, ld = ops.extend_attention(q, k, v, lens, splits=splits)
        assert torch.equal(o1, od) and torch.equal(l1, ld), splits
        assert torch.equal(o1, o2) and torch.equal(l1, l2), splits


# ---- model ----
def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    return 2.0 ** (math.floor(math.log2(x)) - {BF16: 7, F16: 10, F32: 23}[dt])


def _fp32_ref(m, cfg, seq):
    """Logits of the fp32 eager forward of the same weights."""
    m32 = BasicsTransformerLM(**cfg, device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        return m32(seq).double()


def _new_cache(m, batch, paged):
    return PagedKVCache(m, batch, page_size=16) if paged else KVCache(m, batch)


def _rows(cache, upto):
    k, v = cache.gather() if isinstance(cache, PagedKVCache) else (cache.k, cache.v)
    return k[:, :, :, :upto].float(), v[:, :, :, :upto].float()


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d_model,heads", [(256, 4), (160, 2)])
def test_extend_cached_against_fp32(d_model, heads, paged):
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(BF16).eval()
    seq = torch.randint(0, 500, (2, 52), device=DEV)
    ref = _fp32_ref(m, _cfg(d_model, heads), seq)
    with torch.no_grad():
        e_hip = (m(seq).double() - ref).abs().max().item()
        cache, one = _new_cache(m, 2, paged), _new_cache(m, 2, paged)
        m.forward_cached(seq, one)
        out = [m.extend_cached(seq[:, :5], cache), m.extend_cached(seq[:, 5:12], cache),
               m.extend_cached(seq[:, 12:], cache)]
    assert cache.length == 52 and cache.lengths.tolist() == [52, 52]
    e_ext = (torch.cat(out, dim=1).double() - ref).abs().max().item()
    ulp = _ulp(BF16, ref.abs().max().item())
    print(f"d_model {d_model} paged {paged}: e_hip {e_hip:.4e} e_extend {e_ext:.4e} ulp {ulp:.3e}")
    assert e_ext <= 2 * e_hip + ulp, (e_ext, e_hip, ulp)
    for got, want in zip(_rows(cache, 52), _rows(one, 52)):  # the append kernel's tolerance
        print(f"cache rows: max diff {(got - want).abs().max().item():.3e}")
        torch.testing.assert_close(got, want, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("kw", [{}, {"paged": True, "page_size": 16}, {"paged": True, "page_size": 16, "share_prompt": True}])
def test_generate_prefill_chunk_fp32(kw):
    """fp32 takes the reference path of the extend ops: the tokens of the one-shot prefill."""
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).eval()
    x = torch.randint(0, 500, (1, 41), device=DEV).expand(2, -1).contiguous()
    want = m.generate(x, 12, top_k=1, use_cache=True)
    assert torch.equal(m.generate(x, 12, top_k=1, use_cache=True, prefill_chunk=16, **kw), want)


def test_forked_prefix_with_different_suffixes():
    torch.manual_seed(1)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).to(BF16).eval()
    prefix = torch.randint(0, 500, (1, 37), device=DEV)
    suffix = torch.randint(0, 500, (2, 20), device=DEV)
    seq = torch.cat((prefix.expand(2, -1), suffix), dim=1)
    ref = _fp32_ref(m, _cfg(256, 4), seq)[:, 37:]
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 37:] - ref).abs().max().item()
        cache = PagedKVCache(m, 2, page_size=16)
        m.forward_cached(prefix, cache.row(0))
        cache.fork(0, 1)
        assert cache.pages_in_use == 2 + 2  # 2 full prefix pages stored once, a private tail page each
        got = m.extend_cached(suffix, cache)
        dense = []
        for b in range(2):  # two independent dense-cache runs
            c = KVCache(m, 1)
            m.forward_cached(prefix, c)
            dense.append(m.extend_cached(suffix[b:b + 1], c))
    assert cache.pages_in_use == 2 + 2 * 2 and cache.seq_lengths == [57, 57]
    ulp = _ulp(BF16, ref.abs().max().item())
    for name, y in (("forked", got), ("dense", torch.cat(dense))):
        e = (y.double() - ref).abs().max().item()
        print(f"{name}: e_hip {e_hip:.4e} e_extend {e:.4e} ulp {ulp:.3e}")
        assert e <= 2 * e_hip + ulp, (name, e, e_hip, ulp)
