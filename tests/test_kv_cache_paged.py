"""``PagedKVCache`` (``models/kv_cache.py``) on the CPU: the host-side allocator, the eager paged
references against the dense ones, and ``forward_cached`` / ``generate`` on a paged cache against the
dense cache (both run the eager references on equal values, so the comparison is bitwise)."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, KVCache, PagedKVCache

DIMS = (2, 2, 8)  # layers, heads, head dim


def _fill(cache, n, seed=0):
    """Append ``n`` recognisable rows to every sequence: reserve, store through the table, advance."""
    g = torch.Generator().manual_seed(seed)
    P = cache.page_size
    cache.reserve(n)
    for b, start in enumerate(cache.seq_lengths):
        for j in range(start, start + n):
            page = int(cache.block_table[b, j // P])
            assert 0 <= page < cache.num_pages
            cache.k[:, page, :, j % P] = torch.randn(cache.num_layers, cache.num_heads, cache.d_head, generator=g)
            cache.v[:, page, :, j % P] = torch.randn(cache.num_layers, cache.num_heads, cache.d_head, generator=g)
    cache.advance(n)


def _table(cache):
    return cache.block_table.tolist()


def test_constructor_checks():
    with pytest.raises(ValueError):
        PagedKVCache(DIMS, 2, page_size=24, max_len=64)
    with pytest.raises(ValueError):
        PagedKVCache(DIMS, 2, page_size=8, max_len=64)
    with pytest.raises(ValueError):
        PagedKVCache(DIMS, 2, page_size=16)  # dims need max_len
    with pytest.raises(NotImplementedError):
        PagedKVCache(DIMS, 2, page_size=16, max_len=64, fp8=True)
    c = PagedKVCache(DIMS, 3, page_size=16, max_len=40)
    assert c.k.shape == (2, 9, 2, 16, 8) and c.v.shape == c.k.shape  # 3 * ceil(40 / 16) pages
    assert c.block_table.shape == (3, 3) and c.block_table.dtype == torch.int32 and (c.block_table == -1).all()
    assert c.lengths.dtype == torch.int32 and c.length == 0 and c.pages_in_use == 0 and c.pages_free == 9
    assert c.nbytes == 2 * c.k.numel() * 4 + 9 * 4
    assert "page_size=16" in repr(c)


def test_reserve_across_page_boundaries():
    c = PagedKVCache(DIMS, 2, page_size=16, max_len=64)
    table_ptr, len_ptr = c.block_table.data_ptr(), c.lengths.data_ptr()
    c.reserve(1)
    assert c.pages_in_use == 2 and _table(c) == [[0, -1, -1, -1], [1, -1, -1, -1]]
    c.reserve(16)  # still the same page
    assert c.pages_in_use == 2
    c.advance(16)
    assert c.length == 16 and c.lengths.tolist() == [16, 16]
    c.reserve(1)  # slot 16: the second page
    assert c.pages_in_use == 4 and _table(c) == [[0, 2, -1, -1], [1, 3, -1, -1]]
    c.reserve(40)  # slots [16, 56): pages 1..3
    assert c.pages_in_use == 8
    with pytest.raises(ValueError):
        c.reserve(49)  # beyond the table
    assert c.block_table.data_ptr() == table_ptr and c.lengths.data_ptr() == len_ptr


def test_out_of_pages_raises_and_changes_nothing():
    c = PagedKVCache(DIMS, 2, page_size=16, num_pages=3, max_len=64)
    c.reserve(16)
    c.advance(16)
    before = (_table(c), c.seq_lengths, c.pages_free, c.lengths.tolist())
    with pytest.raises(RuntimeError, match="out of pages"):
        c.reserve(1)  # two sequences need a page each, one is free
    assert (_table(c), c.seq_lengths, c.pages_free, c.lengths.tolist()) == before
    c.free(1)
    c.row(0).reserve(17)  # sequence 0 alone fits now
    assert c.pages_free == 0


def test_free_reset_truncate_return_pages():
    c = PagedKVCache(DIMS, 2, page_size=16, max_len=64)
    _fill(c, 40)
    assert c.pages_in_use == 6 and c.length == 40
    c.truncate(33)  # still three pages each
    assert c.pages_in_use == 6 and c.lengths.tolist() == [33, 33]
    c.truncate(32)  # page 2 of each goes back
    assert c.pages_in_use == 4 and all(row[2] == -1 for row in _table(c))
    with pytest.raises(ValueError):
        c.truncate(33)
    c.free(0)
    assert c.pages_in_use == 2 and c.seq_lengths == [0, 32] and c.lengths.tolist() == [0, 32]
    assert _table(c)[0] == [-1, -1, -1, -1]
    with pytest.raises(ValueError):
        c.length  # ragged
    c.reset()
    assert c.pages_in_use == 0 and c.length == 0 and (c.block_table == -1).all() and c.lengths.tolist() == [0, 0]
    _fill(c, 5)  # and the pool is usable again
    assert c.pages_in_use == 2


def test_fork_reference_counts():
    c = PagedKVCache(DIMS, 3, page_size=16, max_len=64)
    r0 = c.row(0)
    _fill(r0, 40)  # two full pages and a tail of 8
    assert c.seq_lengths == [40, 0, 0] and c.pages_in_use == 3
    c.fork(0)
    t = _table(c)
    assert c.seq_lengths == [40, 40, 40] and c.lengths.tolist() == [40, 40, 40] and c.length == 40
    assert t[1][:2] == t[0][:2] and t[2][:2] == t[0][:2]  # full pages shared
    assert len({t[0][2], t[1][2], t[2][2]}) == 3  # the tail page private
    assert c.pages_in_use == 5  # 2 shared + 3 tails, not 9
    k0, v0 = c.gather()
    assert k0.shape == (2, 3, 2, 64, 8)
    assert torch.equal(k0[:, 1], k0[:, 0]) and torch.equal(v0[:, 2], v0[:, 0])
    assert (k0[:, :, :, 40:] == 0).all() and k0[:, :, :, :40].abs().sum() > 0
    # an append to a fork lands in its private tail: the source does not change
    _fill(c.row(1), 3, seed=1)
    k1, v1 = c.gather()
    assert torch.equal(k1[:, 0], k0[:, 0]) and torch.equal(v1[:, 0], v0[:, 0])
    assert torch.equal(k1[:, 2], k0[:, 2]) and not torch.equal(k1[:, 1], k0[:, 1])
    # shared pages are freed only when the last holder goes
    c.free(0)
    assert c.pages_in_use == 4
    c.free(1)
    assert c.pages_in_use == 3
    c.free(2)
    assert c.pages_in_use == 0
    # fork of a length that is a multiple of the page size copies nothing
    _fill(c.row(2), 32)
    c.fork(2, [0])
    assert c.pages_in_use == 2 and c.seq_lengths == [32, 0, 32]


def test_fork_out_of_pages_changes_nothing():
    c = PagedKVCache(DIMS, 3, page_size=16, num_pages=4, max_len=64)
    _fill(c.row(0), 40)  # 3 pages, 1 free, the forks need 2 tails
    before = (_table(c), c.seq_lengths, c.pages_free)
    with pytest.raises(RuntimeError, match="out of pages"):
        c.fork(0)
    assert (_table(c), c.seq_lengths, c.pages_free) == before
    c.fork(0, [2])
    assert c.pages_free == 0 and c.seq_lengths == [40, 0, 40]


def test_truncate_into_shared_page_privatises_it():
    c = PagedKVCache(DIMS, 2, page_size=16, max_len=64)
    _fill(c.row(0), 32)
    c.fork(0)  # both full pages shared
    assert c.pages_in_use == 2
    src_k, src_v = (t.clone() for t in c.row(0).gather())
    r1 = c.row(1)
    r1.truncate(20)  # into shared page 1
    t = _table(c)
    assert t[1][0] == t[0][0] and t[1][1] != t[0][1] and c.pages_in_use == 3
    assert c.seq_lengths == [32, 20] and c.lengths.tolist() == [32, 20]
    k1, _ = r1.gather()
    assert torch.equal(k1[..., :20, :], src_k[..., :20, :])  # the copy kept the rows
    _fill(r1, 6, seed=3)  # rows 20..25 of the fork
    k0, v0 = c.row(0).gather()
    assert torch.equal(k0, src_k) and torch.equal(v0, src_v)  # the source is unchanged
    # truncating to a page boundary needs no copy: the next append gets a fresh page
    r1.truncate(16)
    assert c.pages_in_use == 2
    _fill(r1, 1, seed=4)
    assert _table(c)[1][1] not in (_table(c)[0][1], -1)
    k0, _ = c.row(0).gather()
    assert torch.equal(k0, src_k)


def test_row_shares_storage():
    c = PagedKVCache(DIMS, 3, page_size=16, max_len=48)
    r = c.row(1)
    assert r.batch == 1 and r.k.data_ptr() == c.k.data_ptr()
    assert r.block_table.data_ptr() == c.block_table[1:2].data_ptr() and r.lengths.data_ptr() == c.lengths[1:2].data_ptr()
    _fill(r, 20)
    assert c.seq_lengths == [0, 20, 0] and c.lengths.tolist() == [0, 20, 0] and r.length == 20
    assert c.pages_in_use == 2 and r.pages_in_use == 2
    with pytest.raises(ValueError):
        c.length
    with pytest.raises(IndexError):
        c.row(3)
    r.reset()
    assert c.pages_in_use == 0 and c.length == 0


# ---- references ----
def _paged_inputs(seed, d=16, P=16, B=3, H=2, T=3):
    """Dense (B, H, T*P, d) tensors and the same rows in a pool under a random permutation with spares."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, H, T * P, d, generator=g)
    v = torch.randn(B, H, T * P, d, generator=g)
    num_pages = B * T + 4
    perm = torch.randperm(num_pages, generator=g)
    table = perm[:B * T].reshape(B, T).to(torch.int32)
    kp = torch.full((num_pages, H, P, d), float("nan"))
    vp = torch.full((num_pages, H, P, d), float("nan"))
    for b in range(B):
        for i in range(T):
            kp[table[b, i]] = k[b, :, i * P:(i + 1) * P]
            vp[table[b, i]] = v[b, :, i * P:(i + 1) * P]
    return k, v, kp, vp, table, g


def test_decode_attention_paged_ref_equals_dense():
    k, v, kp, vp, table, g = _paged_inputs(0)
    kv_len = torch.tensor([1, 17, 40], dtype=torch.int32)
    assert torch.equal(ops.paged_gather(kp, table), k)
    q = torch.randn(3, 2, 16, generator=g)
    o0, l0 = ops.decode_attention_ref(q, k, v, kv_len)
    o1, l1 = ops.decode_attention_paged_ref(q, kp, vp, table, kv_len)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    o2, l2 = ops.decode_attention_paged(q, kp, vp, table, kv_len)  # the CPU path of the op
    assert torch.equal(o0, o2) and torch.equal(l0, l2)


@pytest.mark.parametrize("n", [1, 3])
def test_kv_append_rope_paged_ref_equals_dense(n):
    from cs336_systems.models import RotaryEmbedding

    k, v, kp, vp, table, g = _paged_inputs(1)
    re = RotaryEmbedding(64, 16, 10000.0)
    pos = torch.tensor([1, 17, 40], dtype=torch.int32)  # n = 3: sequence 1 stays in page 1, 2 in page 2
    pos[0] = 15 if n == 3 else 1  # ... and sequence 0 crosses from page 0 into page 1
    qkv = torch.randn(3, n, 3 * 2 * 16, generator=g)
    if n == 1:
        q0 = ops.kv_append_rope_ref(qkv[:, 0], re.cos, re.sin, pos, k, v)
        q1 = ops.kv_append_rope_paged_ref(qkv[:, 0], re.cos, re.sin, pos, kp, vp, table)
    else:
        q0 = ops.kv_append_rope_chunk_ref(qkv, re.cos, re.sin, pos, k, v)
        q1 = ops.kv_append_rope_paged(qkv, re.cos, re.sin, pos, kp, vp, table)  # the CPU path of the op
    assert q1.shape == q0.shape and torch.equal(q0, q1)
    assert torch.equal(ops.paged_gather(kp, table), k) and torch.equal(ops.paged_gather(vp, table), v)


def test_kv_append_rope_paged_ref_guards():
    """A slot beyond the table or an entry that names no page stores nothing and zeroes q."""
    from cs336_systems.models import RotaryEmbedding

    _, _, kp, vp, table, g = _paged_inputs(2)
    kp.fill_(1.0)
    vp.fill_(2.0)
    table[1, 1] = -1
    table[2, 0] = kp.shape[0]
    re = RotaryEmbedding(64, 16, 10000.0)
    pos = torch.tensor([47, 15, 0], dtype=torch.int32)
    q = ops.kv_append_rope_paged_ref(torch.randn(3, 2, 3 * 2 * 16, generator=g), re.cos, re.sin, pos, kp, vp, table)
    assert q[0, 0].abs().sum() > 0 and (q[0, 1] == 0).all()  # slot 48 is beyond 3 pages
    assert q[1, 0].abs().sum() > 0 and (q[1, 1] == 0).all()  # slot 16: entry -1
    assert (q[2] == 0).all()  # entry num_pages
    changed = (kp != 1.0).any(dim=-1).sum().item()
    assert changed == 2 * 2  # two tokens x two heads


# ---- model ----
def _model(ctx=32):
    torch.manual_seed(0)
    return BasicsTransformerLM(vocab_size=64, context_length=ctx, d_model=32, num_layers=2, num_heads=2, d_ff=64)


def test_forward_cached_paged_equals_dense_bitwise():
    m = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 64, (2, 9), generator=g)
    dense, paged = KVCache(m, 2), PagedKVCache(m, 2, page_size=16)
    assert torch.equal(m.forward_cached(x, dense), m.forward_cached(x, paged))
    assert paged.pages_in_use == 2
    for step in range(10):  # 9 + 10 = 19: the step at slot 16 crosses into the second page
        t = torch.randint(0, 64, (2, 1), generator=g)
        assert torch.equal(m.forward_cached(t, dense), m.forward_cached(t, paged)), step
    assert paged.length == dense.length == 19 and paged.pages_in_use == 4
    kd, vd = paged.gather()
    assert torch.equal(kd[..., :19, :], dense.k[..., :19, :]) and torch.equal(vd[..., :19, :], dense.v[..., :19, :])
    with pytest.raises(NotImplementedError):
        m.forward_cached(x, paged, chunk=True)
    small = PagedKVCache(m, 2, page_size=16, num_pages=1)
    with pytest.raises(RuntimeError, match="out of pages"):
        m.forward_cached(x, small)


def test_generate_paged_equals_dense():
    m = _model()
    x = torch.randint(0, 64, (2, 9), generator=torch.Generator().manual_seed(6))
    ref = m.generate(x, 12, top_k=1, use_cache=True)
    out = m.generate(x, 12, top_k=1, use_cache=True, paged=True, page_size=16)
    assert out.shape == ref.shape and out.dtype == ref.dtype and torch.equal(out, ref)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, paged=True, kv_fp8=True)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, paged=True)
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, use_cache=True, share_prompt=True)  # needs paged=True
    with pytest.raises(NotImplementedError):
        m.generate(x, 4, top_k=1, use_cache=True, paged=True, draft=m)


def test_generate_share_prompt(monkeypatch):
    m = _model()
    B, pages_per_sequence = 4, 2
    x = torch.randint(0, 64, (1, 20), generator=torch.Generator().manual_seed(7)).expand(B, -1).contiguous()
    ref = m.generate(x, 6, top_k=1, use_cache=True, paged=True, page_size=16)
    caches = []
    new_cache = m._new_cache
    monkeypatch.setattr(m, "_new_cache", lambda *a: caches.append(new_cache(*a)) or caches[-1])
    out = m.generate(x, 6, top_k=1, use_cache=True, paged=True, page_size=16, share_prompt=True)
    assert torch.equal(out, ref)
    (cache,) = caches
    assert cache.length == 25 and cache.pages_per_sequence == pages_per_sequence
    assert cache.pages_in_use == 1 + B < B * pages_per_sequence  # one shared full page, a tail each
    k, _ = cache.gather(0)
    assert all(torch.equal(k[b, :, :20], k[0, :, :20]) for b in range(1, B))
    y = x.clone()
    y[1, 3] += 1
    with pytest.raises(ValueError):
        m.generate(y, 4, top_k=1, use_cache=True, paged=True, share_prompt=True)
    # sampled on the host-free path too: the same tokens as without sharing
    a = m.generate(x, 6, top_k=4, use_cache=True, paged=True, page_size=16, sample_on_device=True,
                   generator=torch.Generator().manual_seed(1))
    b = m.generate(x, 6, top_k=4, use_cache=True, paged=True, page_size=16, sample_on_device=True, share_prompt=True,
                   generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, b)


def test_decode_graph_eager_on_paged_cache():
    """``DecodeGraph(capture=False)`` on a paged cache: reserves per step, equals forward_cached."""
    from cs336_systems.models import DecodeGraph

    m = _model()
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 64, (2, 14), generator=g)
    a, b = PagedKVCache(m, 2, page_size=16), PagedKVCache(m, 2, page_size=16)
    m.forward_cached(x, a)
    m.forward_cached(x, b)
    dg = DecodeGraph(m, b, capture=False)
    for _ in range(4):  # slot 16 crosses a page boundary
        t = torch.randint(0, 64, (2, 1), generator=g)
        assert torch.equal(dg.step(t), m.forward_cached(t, a))
    assert b.pages_in_use == a.pages_in_use == 4 and b.length == 18
    with pytest.raises(NotImplementedError):
        DecodeGraph(m, b, capture=False, tokens=2)
