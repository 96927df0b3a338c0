"""Decode attention (``csrc/flash_attn/fa_decode.hip``) and the KV-append kernel on the GPU.

Oracle: fp64 ``softmax(q.K[:len]^T * scale).V[:len]`` and its LSE from the same rounded inputs.
Tolerances are the project's own for the FA2 forward against fp64 (``test_flash_long_gpu.py``):
max |o - ref| < 2e-2 for 16-bit inputs, < 1e-4 for fp32, and the same bounds for the LSE. The append
kernel is held to the RoPE kernel's tolerances (1e-5 fp32, 1e-2 bf16; ``test_kernels_gpu.py``)."""

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
def _case(dt, d, kv_len, qmul=1.0, batch=B, max_len=MAX_LEN):
    """Inputs (cache rows at and beyond kv_len[b] are NaN) and their oracle, built once per case and
    shared by every split count; nothing modifies them."""
    g = torch.Generator(device=DEV).manual_seed(1234 + d)
    q = (torch.randn(batch, H, d, device=DEV, generator=g) * qmul).to(dt)
    k = torch.randn(batch, H, max_len, d, device=DEV, generator=g).to(dt)
    v = torch.randn(batch, H, max_len, d, device=DEV, generator=g).to(dt)
    for b, n in enumerate(kv_len):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, kv_len, 1.0 / math.sqrt(d))
    return q, k, v, lens, ref_o, ref_l


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


def test_extension_has_decode_ops():
    assert _ext.load_ext(), _ext.load_error()
    assert hasattr(torch.ops.cs336, "fa_decode") and hasattr(torch.ops.cs336, "kv_append_rope")


@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("kv_len", KV_LENS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_attention_grid(dt, d, kv_len, splits):
    q, k, v, lens, ref_o, ref_l = _case(dt, d, kv_len)
    o, lse = ops.decode_attention(q, k, v, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} {kv_len} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_attention_peaky(dt, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k, v, lens, ref_o, ref_l = _case(dt, 64, KV_LENS[0], 8.0)
    o, lse = ops.decode_attention(q, k, v, lens, splits=splits)
    _check(o, lse, ref_o, ref_l, dt, f"peaky {dt} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 1, 5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_empty_sequence(dt, splits):
    q, k, v, lens, ref_o, ref_l = _case(dt, 64, (0, 7), batch=2)
    o, lse = ops.decode_attention(q, k, v, lens, splits=splits)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    assert torch.equal(o[0], torch.zeros_like(o[0]))
    assert torch.isinf(lse[0]).all() and (lse[0] < 0).all()
    _check(o, lse, ref_o, ref_l, dt, f"empty {dt} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("d", [64, 80])
def test_strided_cache_views_bitwise(d, splits):
    """A layer slice of an (L, B, H, max_len, d) cache and a batch sub-view are read in place and give
    the bits of the contiguous call."""
    dt = torch.bfloat16
    q, k, v, lens, ref_o, ref_l = _case(dt, d, KV_LENS[0])
    o0, l0 = ops.decode_attention(q, k, v, lens, splits=splits)
    big_k = torch.full((2, B, H, MAX_LEN, d), float("nan"), device=DEV, dtype=dt)
    big_v = torch.full_like(big_k, float("nan"))
    big_k[1].copy_(k)
    big_v[1].copy_(v)
    assert not big_k[1].is_contiguous() or big_k[1].data_ptr() != big_k.data_ptr()
    o1, l1 = ops.decode_attention(q, big_k[1], big_v[1], lens, splits=splits)
    assert torch.equal(o1, o0) and torch.equal(l1, l0)
    # batch sub-view: sequences 1..2 of a larger batch
    o2, l2 = ops.decode_attention(q[1:3], k[1:3], v[1:3], lens[1:3], splits=splits)
    o3, l3 = ops.decode_attention(q[1:3].clone(), k[1:3].clone(), v[1:3].clone(), lens[1:3].clone(), splits=splits)
    assert torch.equal(o2, o3) and torch.equal(l2, l3)
    _check(o2, l2, ref_o[1:3], ref_l[1:3], dt, f"batch sub-view d{d} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
def test_run_to_run_bitwise(splits):
    q, k, v, lens, _, _ = _case(torch.bfloat16, 128, KV_LENS[0])
    o0, l0 = ops.decode_attention(q, k, v, lens, splits=splits)
    o1, l1 = ops.decode_attention(q, k, v, lens, splits=splits)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def test_64bit_cache_offsets():
    """Head 1 of a (1, 2, 2^23 + 8, 128) bf16 cache starts beyond a 2 GiB byte offset."""
    d, n, max_len = 128, 300, 2**23 + 8
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    k = torch.empty(1, 2, max_len, d, device=DEV, dtype=dt)
    v = torch.empty(1, 2, max_len, d, device=DEV, dtype=dt)
    assert k.stride(1) * k.element_size() > 2**31
    k[:, :, :n] = torch.randn(1, 2, n, d, device=DEV, generator=g).to(dt)
    v[:, :, :n] = torch.randn(1, 2, n, d, device=DEV, generator=g).to(dt)
    q = torch.randn(1, 2, d, device=DEV, generator=g).to(dt)
    lens = torch.tensor([n], dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, k, v, (n,), 1.0 / math.sqrt(d))
    for splits in (0, 1):  # 0: the host sizes the split count from max_kv_len = max_len
        o, lse = ops.decode_attention(q, k, v, lens, splits=splits)
        _check(o, lse, ref_o, ref_l, dt, f"64-bit splits {splits}:")
    o, lse = ops.decode_attention(q, k, v, lens, max_kv_len=n)
    _check(o, lse, ref_o, ref_l, dt, "64-bit max_kv_len 300:")


def test_unsupported_inputs_raise():
    q, k, v, lens, _, _ = _case(torch.bfloat16, 64, KV_LENS[0])
    hip = torch.ops.cs336
    with pytest.raises(RuntimeError):  # head dim the kernel does not take
        hip.fa_decode(q[..., :48].contiguous(), k[..., :48].contiguous(), v[..., :48].contiguous(), lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # kv_len must be int32 on the device
        hip.fa_decode(q, k, v, lens.long(), 0.1, 300, 0)
    with pytest.raises(RuntimeError):
        hip.fa_decode(q, k, v, lens, 0.1, MAX_LEN + 1, 0)
    with pytest.raises(RuntimeError):
        hip.fa_decode(q, k.float(), v.float(), lens, 0.1, 300, 0)
    # the wrapper runs the reference for other head dims
    o, lse = ops.decode_attention(q[..., :48].contiguous(), k[..., :48].contiguous(), v[..., :48].contiguous(), lens)
    assert o.shape == (B, H, 48) and torch.isfinite(o).all()


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        q = torch.empty(2, 5, 80, device=DEV, dtype=torch.bfloat16)
        cache = torch.empty(3, 2, 5, 40, 80, device=DEV, dtype=torch.bfloat16)
        lens = torch.empty(2, device=DEV, dtype=torch.int32)
        o, lse = torch.ops.cs336.fa_decode(q, cache[1], cache[2], lens, 0.1, 40, 0)
        assert o.shape == (2, 5, 80) and o.dtype == torch.bfloat16
        assert lse.shape == (2, 5) and lse.dtype == torch.float32
        qkv = torch.empty(2, 3 * 5 * 80, device=DEV, dtype=torch.bfloat16)
        cs = torch.empty(40, 40, device=DEV, dtype=torch.float32)
        qo = torch.ops.cs336.kv_append_rope(qkv, cs, cs, lens, cache[1], cache[2])
        assert qo.shape == (2, 5, 80) and qo.dtype == torch.bfloat16


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_kv_append_rope(dt, d):
    from cs336_systems.models import RotaryEmbedding

    max_len = 16
    g = torch.Generator(device=DEV).manual_seed(d)
    re = RotaryEmbedding(max_len, d, 10000.0).to(DEV)
    qkv = torch.randn(B, 3 * H * d, device=DEV, generator=g).to(dt)
    # caches are layer slices of a larger tensor, pre-filled with a sentinel
    sent_k, sent_v = 3.0, -5.0
    big_k = torch.full((2, B, H, max_len, d), sent_k, device=DEV, dtype=dt)
    big_v = torch.full((2, B, H, max_len, d), sent_v, device=DEV, dtype=dt)
    pos_l = [0, 7, 15]
    pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
    q = ops.kv_append_rope(qkv, re.cos, re.sin, pos, big_k[1], big_v[1])
    assert q.shape == (B, H, d) and q.dtype == dt and q.is_contiguous()
    q_in, k_in, v_in = qkv.view(B, 3, H, d).unbind(1)
    p = pos.long()[:, None, None]
    tol = 1e-5 if dt == torch.float32 else 1e-2
    q_ref = ops.rope_ref(q_in.float().unsqueeze(2), re.cos, re.sin, p).squeeze(2)
    k_ref = ops.rope_ref(k_in.float().unsqueeze(2), re.cos, re.sin, p).squeeze(2)
    torch.testing.assert_close(q.float(), q_ref, rtol=tol, atol=tol)
    rows = torch.arange(B, device=DEV)
    k_new = big_k[1][rows, :, pos.long()]  # (B, H, d)
    v_new = big_v[1][rows, :, pos.long()]
    torch.testing.assert_close(k_new.float(), k_ref, rtol=tol, atol=tol)
    assert torch.equal(v_new, v_in)
    untouched = torch.ones(2, B, H, max_len, dtype=torch.bool, device=DEV)
    for b, pb in enumerate(pos_l):
        untouched[1, b, :, pb] = False
    assert (big_k[untouched] == sent_k).all() and (big_v[untouched] == sent_v).all()
