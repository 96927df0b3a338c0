"""Paged decode attention and the paged KV-append kernel (``csrc/flash_attn/fa_decode_paged.hip``) on
the GPU.

Oracle and tolerances are those of ``test_decode_attention_gpu.py``: fp64 attention over the first
``kv_len[b]`` rows of the LOGICAL cache, max |o - ref| and |lse - ref| < 2e-2 for 16-bit inputs and
< 1e-4 for fp32; the append is held to 1e-5 fp32 / 1e-2 bf16 against ``rope_ref``, V bitwise.

Every pool here has spare pages; the used pages are placed by a seeded permutation; every spare page
and every row at or beyond ``kv_len[b]`` of a used page is NaN; every table entry past a sequence's
last page points at an in-range NaN page (never at an out-of-range id): a kernel that reads too far
shows up as a NaN in the output, not as a fault."""

import functools
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, MAX_LEN = 3, 3, 320
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DIMS = [32, 64, 80, 128]
KV_LENS = [(1, 65, 300), (64, 128, 320)]
PAGES = [16, 64]


def _tol(dt):
    return 2e-2 if dt != torch.float32 else 1e-4


def _oracle(q, k, v, kv_len, scale):
    """fp64 attention of each sequence over its first kv_len[b] rows only (NaN tails never touched)."""
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:2], float("-inf"), dtype=torch.float64, device=q.device)
    for b, n in enumerate(kv_len):
        if n == 0:
            continue
        s = torch.einsum("hd,hnd->hn", q[b].double(), k[b, :, :n].double()) * scale
        lse[b] = torch.logsumexp(s, -1)
        o[b] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v[b, :, :n].double())
    return o, lse


@functools.lru_cache(maxsize=None)
def _case(dt, d, kv_len, batch=B, max_len=MAX_LEN):
    """Logical inputs (rows at and beyond kv_len[b] are NaN) and their oracle, built once per case and
    shared by every split count, page size and placement; nothing modifies them."""
    g = torch.Generator(device=DEV).manual_seed(1234 + d)
    q = torch.randn(batch, H, d, device=DEV, generator=g).to(dt)
    k = torch.randn(batch, H, max_len, d, device=DEV, generator=g).to(dt)
    v = torch.randn(batch, H, max_len, d, device=DEV, generator=g).to(dt)
    for b, n in enumerate(kv_len):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, kv_len, 1.0 / math.sqrt(d))
    return q, k, v, lens, ref_o, ref_l


@functools.lru_cache(maxsize=None)
def _paged(dt, d, kv_len, P, seed=0, spare=5, batch=B, max_len=MAX_LEN):
    """The case's rows in a NaN pool of ``used + spare`` pages under a seeded permutation -> (k_pool,
    v_pool, table). Table entries past a sequence's pages point at a spare (all-NaN) page."""
    _, k, v, _, _, _ = _case(dt, d, kv_len, batch, max_len)
    T = -(-max_len // P)
    used = [-(-n // P) for n in kv_len]
    num_pages = sum(used) + spare
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    kp = torch.full((num_pages, H, P, d), float("nan"), device=DEV, dtype=dt)
    vp = torch.full_like(kp, float("nan"))
    spare_ids = perm[sum(used):]
    table = torch.empty(batch, T, dtype=torch.int32)
    it = iter(perm)
    for b in range(batch):
        for i in range(T):
            if i < used[b]:
                page = next(it)
                kp[page] = k[b, :, i * P:(i + 1) * P]  # (rows at and beyond kv_len[b] are NaN already)
                vp[page] = v[b, :, i * P:(i + 1) * P]
            else:
                page = spare_ids[(b + i) % spare]
            table[b, i] = page
    return kp, vp, table.to(DEV)


def _check(o, lse, ref_o, ref_l, dt, what=""):
    assert o.dtype == dt and lse.dtype == torch.float32
    assert o.shape == ref_o.shape and lse.shape == ref_l.shape
    assert torch.isfinite(o).all(), what
    eo = (o.double() - ref_o).abs().max().item()
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(lse), fin), what
    el = (lse.double()[fin] - ref_l[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what} max|o-ref| {eo:.3e} max|lse-ref| {el:.3e}")
    assert eo < _tol(dt), (what, eo)
    assert el < _tol(dt), (what, el)


def test_extension_has_paged_ops():
    assert _ext.load_ext(), _ext.load_error()
    assert hasattr(torch.ops.cs336, "fa_decode_paged") and hasattr(torch.ops.cs336, "kv_append_rope_paged")


@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("kv_len", KV_LENS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_attention_paged_grid(dt, d, kv_len, splits, P):
    q, _, _, lens, ref_o, ref_l = _case(dt, d, kv_len)
    kp, vp, table = _paged(dt, d, kv_len, P)
    o, lse = ops.decode_attention_paged(q, kp, vp, table, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} {kv_len} splits {splits} page {P}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("d", [64, 80])
def test_placement_invariance_bitwise(d, P, splits):
    """The same logical rows under two permutations and pool sizes give the same bits; so does a rerun."""
    dt = torch.bfloat16
    q, _, _, lens, ref_o, ref_l = _case(dt, d, KV_LENS[0])
    k0, v0, t0 = _paged(dt, d, KV_LENS[0], P)
    k1, v1, t1 = _paged(dt, d, KV_LENS[0], P, seed=1, spare=9)
    assert k0.shape[0] != k1.shape[0] and not torch.equal(t0, t1)
    o0, l0 = ops.decode_attention_paged(q, k0, v0, t0, lens, splits=splits)
    o1, l1 = ops.decode_attention_paged(q, k1, v1, t1, lens, splits=splits)
    o2, l2 = ops.decode_attention_paged(q, k0, v0, t0, lens, splits=splits)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)
    _check(o0, l0, ref_o, ref_l, dt, f"placement d{d} page {P} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 1, 5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_empty_sequence(dt, splits):
    q, _, _, lens, ref_o, ref_l = _case(dt, 64, (0, 7), batch=2)
    kp, vp, table = _paged(dt, 64, (0, 7), 16, batch=2)
    o, lse = ops.decode_attention_paged(q, kp, vp, table, lens, splits=splits)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    assert torch.equal(o[0], torch.zeros_like(o[0]))
    assert torch.isinf(lse[0]).all() and (lse[0] < 0).all()
    _check(o, lse, ref_o, ref_l, dt, f"empty {dt} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("d", [64, 80])
def test_pool_as_layer_slice_bitwise(d, splits):
    """cache.k[l] of an (L, num_pages, H, P, d) pool is read in place: the bits of a contiguous copy."""
    dt, P = torch.bfloat16, 16
    q, _, _, lens, _, _ = _case(dt, d, KV_LENS[0])
    kp, vp, table = _paged(dt, d, KV_LENS[0], P)
    o0, l0 = ops.decode_attention_paged(q, kp, vp, table, lens, splits=splits)
    big_k = torch.full((3, *kp.shape), float("nan"), device=DEV, dtype=dt)
    big_v = torch.full_like(big_k, float("nan"))
    big_k[1].copy_(kp)
    big_v[2].copy_(vp)
    assert big_k[1].data_ptr() != big_k.data_ptr()
    o1, l1 = ops.decode_attention_paged(q, big_k[1], big_v[2], table, lens, splits=splits)
    assert torch.equal(o1, o0) and torch.equal(l1, l0)
    # a table that is a row sub-view of a larger one
    wide = torch.zeros(B + 2, table.shape[1] + 3, dtype=torch.int32, device=DEV)
    wide[1:1 + B, :table.shape[1]] = table
    o2, l2 = ops.decode_attention_paged(q, kp, vp, wide[1:1 + B, :table.shape[1]], lens, splits=splits)
    assert torch.equal(o2, o0) and torch.equal(l2, l0)


def test_64bit_pool_offsets():
    """The used pages of a (16400, 2, 256, 128) bf16 pool start beyond a 2 GiB byte offset."""
    d, n, P, num_pages = 128, 300, 256, 16400
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    kp = torch.empty(num_pages, 2, P, d, device=DEV, dtype=dt)
    vp = torch.empty(num_pages, 2, P, d, device=DEV, dtype=dt)
    ids = [num_pages - 1, num_pages - 3]  # the top of the pool, out of order
    assert min(ids) * kp.stride(0) * kp.element_size() > 2**31
    k = torch.randn(1, 2, 2 * P, d, device=DEV, generator=g).to(dt)
    v = torch.randn(1, 2, 2 * P, d, device=DEV, generator=g).to(dt)
    k[:, :, n:] = float("nan")
    v[:, :, n:] = float("nan")
    for i, page in enumerate(ids):
        kp[page] = k[0, :, i * P:(i + 1) * P]
        vp[page] = v[0, :, i * P:(i + 1) * P]
    kp[0] = float("nan")  # where a 32-bit offset would wrap to
    vp[0] = float("nan")
    table = torch.tensor([ids + [0, 0]], dtype=torch.int32, device=DEV)
    q = torch.randn(1, 2, d, device=DEV, generator=g).to(dt)
    lens = torch.tensor([n], dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, (n,), 1.0 / math.sqrt(d))
    for splits in (0, 1):
        o, lse = ops.decode_attention_paged(q, kp, vp, table, lens, splits=splits)
        _check(o, lse, ref_o, ref_l, dt, f"64-bit splits {splits}:")


@pytest.mark.parametrize("guard", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_kv_append_rope_paged(dt, d, n, guard):
    """pos (0, 15, 30) at page size 16 with a 2-page table (max_len 32): n = 3 crosses a page boundary
    in sequence 1 and runs past max_len in sequence 2 (slot 32 stores nothing, q row zeroed). Only the
    addressed rows change. ``guard``: the pool is the middle slice of a larger sentinel allocation and
    two table entries are -1 and num_pages, which then land inside that allocation: a missing id guard
    shows as a changed sentinel."""
    from cs336_systems.models import RotaryEmbedding

    P, T, NP = 16, 2, 8
    g = torch.Generator(device=DEV).manual_seed(d + n)
    re = RotaryEmbedding(64, d, 10000.0).to(DEV)
    qkv = torch.randn(B, n, 3 * H * d, device=DEV, generator=g).to(dt)
    sent_k, sent_v = 3.0, -5.0
    big_k = torch.full((NP + 2, H, P, d), sent_k, device=DEV, dtype=dt)
    big_v = torch.full((NP + 2, H, P, d), sent_v, device=DEV, dtype=dt)
    kp, vp = big_k[1:-1], big_v[1:-1]
    tab = [[5, 2], [7, 0], [3, 6]]
    if guard:
        tab[1][1], tab[2][1] = NP, -1
    table = torch.tensor(tab, dtype=torch.int32, device=DEV)
    pos_l = [0, 15, 30]
    pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
    arg = qkv[:, 0] if n == 1 else qkv
    q = ops.kv_append_rope_paged(arg, re.cos, re.sin, pos, kp, vp, table)
    assert q.shape == ((B, H, d) if n == 1 else (B, n, H, d)) and q.dtype == dt and q.is_contiguous()
    q = q.reshape(B, n, H, d)
    q_in, k_in, v_in = qkv.view(B, n, 3, H, d).unbind(2)  # (B, n, H, d)
    tol = 1e-5 if dt == torch.float32 else 1e-2
    untouched = torch.ones(NP + 2, H, P, dtype=torch.bool, device=DEV)
    stored = 0
    for b in range(B):
        for i in range(n):
            slot = pos_l[b] + i
            page = tab[b][slot // P] if slot < T * P else -1
            ok = slot < T * P and 0 <= page < NP
            if not ok:
                assert torch.equal(q[b, i], torch.zeros_like(q[b, i])), (b, i)
                continue
            p = torch.tensor([slot], device=DEV)
            q_ref = ops.rope_ref(q_in[b, i].float().unsqueeze(1), re.cos, re.sin, p).squeeze(1)
            k_ref = ops.rope_ref(k_in[b, i].float().unsqueeze(1), re.cos, re.sin, p).squeeze(1)
            torch.testing.assert_close(q[b, i].float(), q_ref, rtol=tol, atol=tol)
            torch.testing.assert_close(kp[page, :, slot % P].float(), k_ref, rtol=tol, atol=tol)
            assert torch.equal(vp[page, :, slot % P], v_in[b, i])
            untouched[1 + page, :, slot % P] = False
            stored += 1
    assert stored >= 2  # (the case is not vacuous)
    assert (big_k[untouched] == sent_k).all() and (big_v[untouched] == sent_v).all()


def test_unsupported_inputs_raise():
    dt, P = torch.bfloat16, 16
    q, _, _, lens, _, _ = _case(dt, 64, KV_LENS[0])
    kp, vp, table = _paged(dt, 64, KV_LENS[0], P)
    hip = torch.ops.cs336
    with pytest.raises(RuntimeError):  # head dim the kernel does not take
        hip.fa_decode_paged(q[..., :48].contiguous(), kp[..., :48].contiguous(), vp[..., :48].contiguous(), table, lens,
                            0.1, 300, 0)
    with pytest.raises(RuntimeError):  # kv_len must be int32
        hip.fa_decode_paged(q, kp, vp, table, lens.long(), 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # the table must be int32
        hip.fa_decode_paged(q, kp, vp, table.long(), lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # pool dtype
        hip.fa_decode_paged(q, kp.float(), vp.float(), table, lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # max_kv_len beyond table columns * page size
        hip.fa_decode_paged(q, kp, vp, table, lens, 0.1, table.shape[1] * P + 1, 0)
    with pytest.raises(RuntimeError):  # a page size the kernel does not take
        hip.fa_decode_paged(q, kp[:, :, :8], vp[:, :, :8], table, lens, 0.1, 8, 0)
    cs = torch.zeros(64, 32, device=DEV)
    qkv = torch.zeros(B, 1, 3 * H * 64, device=DEV, dtype=dt)
    with pytest.raises(RuntimeError):
        hip.kv_append_rope_paged(qkv, cs, cs, lens, kp, vp, table.long())
    with pytest.raises(RuntimeError):
        hip.kv_append_rope_paged(qkv, cs, cs, lens.long(), kp, vp, table)
    with pytest.raises(RuntimeError):
        hip.kv_append_rope_paged(qkv, cs, cs, lens, kp.float(), vp.float(), table)
    # the wrapper runs the reference for other head dims
    o, lse = ops.decode_attention_paged(q[..., :48].contiguous(), kp[..., :48].contiguous(), vp[..., :48].contiguous(),
                                        table, lens)
    assert o.shape == (B, H, 48) and torch.isfinite(o).all()


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        q = torch.empty(2, 5, 80, device=DEV, dtype=torch.bfloat16)
        pool = torch.empty(3, 7, 5, 16, 80, device=DEV, dtype=torch.bfloat16)
        table = torch.empty(2, 4, device=DEV, dtype=torch.int32)
        lens = torch.empty(2, device=DEV, dtype=torch.int32)
        o, lse = torch.ops.cs336.fa_decode_paged(q, pool[1], pool[2], table, lens, 0.1, 64, 0)
        assert o.shape == (2, 5, 80) and o.dtype == torch.bfloat16
        assert lse.shape == (2, 5) and lse.dtype == torch.float32
        qkv = torch.empty(2, 3, 3 * 5 * 80, device=DEV, dtype=torch.bfloat16)
        cs = torch.empty(64, 40, device=DEV, dtype=torch.float32)
        qo = torch.ops.cs336.kv_append_rope_paged(qkv, cs, cs, lens, pool[1], pool[2], table)
        assert qo.shape == (2, 3, 5, 80) and qo.dtype == torch.bfloat16
