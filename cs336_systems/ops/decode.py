"""Single-token attention against a KV cache and the append of the new token's K / V row, eager
references + HIP kernels (``csrc/flash_attn/fa_decode.hip``).

``decode_attention``: one query row per (batch, head), ``q`` (B, H, d), against keys
``[0, kv_len[b])`` of ``(B, H, max_len, d)`` cache views (any batch / head strides: a layer slice of
a larger cache tensor is passed as is). ``kv_len`` is an int32 device tensor; nothing synchronizes
the host. Returns ``o`` (B, H, d) in q's dtype and the natural-log ``lse`` (B, H) fp32. A sequence
with ``kv_len == 0`` gives ``o = 0`` and ``lse = -inf``. Rows at and beyond ``kv_len[b]`` are never
used and may hold anything.

``kv_append_rope``: the new token's fused projection row ``qkv`` (B, 3*H*d; q|k|v) -> rotated q
(B, H, d); rotated k and plain v are written into row ``pos[b]`` of every (b, h) cache plane. A
``pos[b]`` outside the cache stores nothing.

``decode_attention_chunk`` / ``kv_append_rope_chunk`` (``csrc/flash_attn/fa_decode_chunk.hip``): the
same for ``n >= 1`` tokens per sequence -- a follow-up prompt, a prefill in chunks or the verify step
of speculative decoding. ``q`` is (B, n, H, d) and ``kv_len[b]`` counts the keys AFTER the chunk's own
rows were appended: query ``i`` sees keys ``[0, kv_len[b] - (n - 1 - i))``, clamped to
``[0, max_len]`` (bottom-right-aligned causality); a query whose bound is <= 0 gives ``o = 0``,
``lse = -inf``. ``qkv`` is (B, n, 3*H*d), ``pos[b]`` the slot of the chunk's first token; token ``i``
is rotated at and written to ``pos[b] + i``, and a token without a slot stores nothing.

The HIP kernels take head dims 32 / 64 / 80 / 128 (the ones the model's fused attention path takes);
other head dims run the reference. On a GPU with the HIP backend a missing extension raises.

FP8 cache (``csrc/flash_attn/fa_decode_kv8.hip``, ``fa_decode_chunk_kv8.hip``): the four ops also take
``torch.float8_e4m3fn`` cache planes with the keyword-only ``k_scale`` / ``v_scale`` (B, H, max_len)
fp32 planes, one scale per cached row: the row is ``bytes * scale[row]``. A row is quantized when it
is written and never again: ``amax = max |x|`` over its d fp32 values, ``scale = amax / 448`` (1 for
an all-zero row), ``bytes = RNE(clamp(x / scale, -448, 448))`` -- the clamp before the cast, as in
``quantize_fp8_rows_``, because e4m3fn turns overflow into the NaN byte. An appended K row is
quantized from its fp32 rotated value (one rounding, not two through the compute dtype).
``kv_quantize_rows`` is the prefill's store of whole (B, H, n, d) K / V tensors. q / o stay bf16,
fp16 or fp32. An FP8 cache without both scales, or scales with any other cache, raise ``ValueError``.

Paged cache (``csrc/flash_attn/fa_decode_paged.hip``): ``decode_attention_paged`` / ``kv_append_rope_paged``
take ``(num_pages, H, P, d)`` page pools and an int32 ``block_table`` ``(B, T)`` instead of the dense
planes: row ``j`` of sequence ``b`` is row ``j % P`` of page ``block_table[b, j // P]``. The references
gather the rows by the table and apply the dense rules; bf16 / fp16 / fp32 only.
"""

from __future__ import annotations

import math

import torch

from ._ext import ops, use_hip
from .rope import rope_ref

_DECODE_D = (32, 64, 80, 128)
_E4M3 = torch.float8_e4m3fn
FP8_MAX = 448.0  # largest finite e4m3 value


def _kv8(k_cache, v_cache, k_scale, v_scale) -> bool:
    """Whether the caches are the FP8 format; the argument errors of the four ops."""
    if k_cache.dtype != _E4M3 and v_cache.dtype != _E4M3:
        if k_scale is not None or v_scale is not None:
            raise ValueError(f"k_scale / v_scale go with a float8_e4m3fn cache, not {k_cache.dtype}")
        return False
    if k_cache.dtype != v_cache.dtype:
        raise ValueError("k_cache and v_cache must both be float8_e4m3fn")
    if k_scale is None or v_scale is None:
        raise ValueError("a float8_e4m3fn cache needs k_scale and v_scale")
    for s, c in ((k_scale, k_cache), (v_scale, v_cache)):
        if s.dtype != torch.float32 or tuple(s.shape) != tuple(c.shape[:-1]):
            raise ValueError("k_scale / v_scale must be fp32 (B, H, max_len) planes of the caches")
    return True


def _scale_layout_ok(s: torch.Tensor) -> bool:
    return s.stride(-1) == 1 and s.data_ptr() % 4 == 0


def kv_quantize_ref(x):
    """Rows ``x`` (..., d) -> e4m3 bytes (..., d) and fp32 scales (...), by the formula above."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # (a tensor divisor: by a Python scalar torch multiplies by the reciprocal on a GPU, one ulp off)
    s = torch.where(amax > 0, amax / torch.full_like(amax, FP8_MAX), torch.ones_like(amax))
    return (xf / s[..., None]).clamp_(-FP8_MAX, FP8_MAX).to(_E4M3), s


def kv_dequantize(plane, scale):
    """fp32 ``bytes * scale[row]`` of a plane (rows nobody wrote may hold NaN bytes: mask, as the refs do)."""
    return plane.float() * scale[..., None]


def kv_quantize_rows_ref(x, plane, scale):
    n = x.shape[2]
    q, s = kv_quantize_ref(x)
    plane[:, :, :n].copy_(q)
    scale[:, :, :n].copy_(s)


def kv_quantize_rows(x, plane, scale) -> None:
    """Quantize the rows of ``x`` (B, H, n, d; bf16 / fp16 / fp32, last dim contiguous, any other
    strides) into rows ``[0, n)`` of the e4m3 ``plane`` (B, H, max_len, d) and its fp32 ``scale``
    plane (B, H, max_len): what a prefill stores instead of ``copy_``."""
    if plane.dtype != _E4M3 or scale.dtype != torch.float32 or tuple(scale.shape) != tuple(plane.shape[:-1]):
        raise ValueError("kv_quantize_rows takes a float8_e4m3fn plane (B, H, max_len, d) and its fp32 scale plane")
    if x.dim() != 4 or tuple(x.shape[:2]) != tuple(plane.shape[:2]) or x.shape[3] != plane.shape[3] \
            or x.shape[2] > plane.shape[2]:
        raise ValueError("kv_quantize_rows: x must be (B, H, n <= max_len, d) for the plane")
    d = x.shape[-1]
    if (use_hip(x, plane, scale) and d in _DECODE_D and x.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and _cache_layout_ok(plane) and _scale_layout_ok(scale)):
        es = x.element_size()
        if x.stride(-1) != 1 or x.data_ptr() % 16 or any((x.stride(i) * es) % 16 for i in range(3)):
            x = x.contiguous()
        ops().kv_quantize_rows(x, plane, scale)
        return
    kv_quantize_rows_ref(x, plane, scale)


def decode_attention_ref(q, k_cache, v_cache, kv_len, scale=None):
    """Masked softmax over the first ``kv_len[b]`` keys, fp32 (or fp64) math. Cache rows beyond the
    valid range are replaced before any arithmetic, so NaNs there cannot leak."""
    B, H, d = q.shape
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    n = k_cache.shape[2]
    valid = torch.arange(n, device=q.device)[None, :] < kv_len.to(torch.int64)[:, None]  # (B, n)
    vm = valid[:, None, :, None]
    k = torch.where(vm, k_cache.to(ct), 0.0)
    v = torch.where(vm, v_cache.to(ct), 0.0)
    s = torch.einsum("bhd,bhnd->bhn", q.to(ct), k) * scale
    s = torch.where(valid[:, None, :], s, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isinf(lse), 0.0, lse)[..., None])  # empty row: exp(-inf) = 0
    o = torch.einsum("bhn,bhnd->bhd", p, v)
    return o.to(q.dtype), lse.float()


def kv_append_rope_ref(qkv, cos, sin, pos, k_cache, v_cache):
    B, H, max_len, d = k_cache.shape
    q, k, v = qkv.reshape(B, 3, H, d).unbind(1)
    ok = (pos >= 0) & (pos < min(max_len, cos.shape[0]))
    p = pos.to(torch.int64).clamp(0, min(max_len, cos.shape[0]) - 1)
    # rope_ref rotates (..., seq, d) at positions broadcastable to x[..., 0]: (B, H, 1, d) at (B, 1, 1)
    q_rot = rope_ref(q.unsqueeze(2), cos, sin, p[:, None, None]).squeeze(2)
    k_rot = rope_ref(k.unsqueeze(2), cos, sin, p[:, None, None]).squeeze(2)
    idx = p[:, None, None, None].expand(B, H, 1, d)
    keep = ok[:, None, None, None]
    k_cache.scatter_(2, idx, torch.where(keep, k_rot.unsqueeze(2).to(k_cache.dtype), k_cache.gather(2, idx)))
    v_cache.scatter_(2, idx, torch.where(keep, v.unsqueeze(2).to(v_cache.dtype), v_cache.gather(2, idx)))
    return torch.where(ok[:, None, None], q_rot, torch.zeros_like(q_rot)).contiguous()


def _cache_layout_ok(t: torch.Tensor) -> bool:
    es = t.element_size()
    return (t.dim() == 4 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0
            and all((t.stride(i) * es) % 16 == 0 for i in range(3)))


def decode_attention(q, k_cache, v_cache, kv_len, scale=None, max_kv_len=None, splits=0, *, k_scale=None, v_scale=None):
    """``max_kv_len``: host-known upper bound of ``kv_len`` (default: the cache's ``max_len``), used
    only to choose the split count; ``splits``: 0 = choose, n = exactly n key splits. ``k_scale`` /
    ``v_scale``: the scale planes of a ``float8_e4m3fn`` cache."""
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
    if _kv8(k_cache, v_cache, k_scale, v_scale):
        if (use_hip(q, k_cache, v_cache) and d in _DECODE_D and q.dtype in (torch.bfloat16, torch.float16, torch.float32)
                and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)
                and _scale_layout_ok(k_scale) and _scale_layout_ok(v_scale)):
            max_len = k_cache.shape[2]
            bound = max_len if max_kv_len is None else min(int(max_kv_len), max_len)
            if kv_len.dtype != torch.int32:
                kv_len = kv_len.to(torch.int32)
            return ops().fa_decode_kv8(q, k_cache, v_cache, k_scale, v_scale, kv_len.contiguous(), scale, bound,
                                       int(splits))
        return decode_attention_ref(q, kv_dequantize(k_cache, k_scale), kv_dequantize(v_cache, v_scale), kv_len, scale)
    if (use_hip(q, k_cache, v_cache) and d in _DECODE_D and q.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)):
        max_len = k_cache.shape[2]
        bound = max_len if max_kv_len is None else min(int(max_kv_len), max_len)
        if kv_len.dtype != torch.int32:
            kv_len = kv_len.to(torch.int32)
        return ops().fa_decode(q, k_cache, v_cache, kv_len.contiguous(), scale, bound, int(splits))
    return decode_attention_ref(q, k_cache, v_cache, kv_len, scale)


def kv_append_rope_kv8_ref(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale):
    return kv_append_rope_chunk_kv8_ref(qkv[:, None], cos, sin, pos, k_cache, v_cache, k_scale, v_scale)[:, 0]


def kv_append_rope(qkv, cos, sin, pos, k_cache, v_cache, *, k_scale=None, v_scale=None):
    d = k_cache.shape[-1]
    if _kv8(k_cache, v_cache, k_scale, v_scale):
        if (use_hip(qkv, k_cache, v_cache) and d in _DECODE_D
                and qkv.dtype in (torch.bfloat16, torch.float16, torch.float32) and qkv.dim() == 2 and qkv.stride(-1) == 1
                and qkv.data_ptr() % 16 == 0 and (qkv.stride(0) * qkv.element_size()) % 16 == 0
                and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)
                and _scale_layout_ok(k_scale) and _scale_layout_ok(v_scale)):
            if pos.dtype != torch.int32:
                pos = pos.to(torch.int32)
            return ops().kv_append_rope_kv8(qkv, cos.float().contiguous(), sin.float().contiguous(), pos.contiguous(),
                                            k_cache, v_cache, k_scale, v_scale)
        return kv_append_rope_kv8_ref(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    if (use_hip(qkv, k_cache, v_cache) and d % 8 == 0 and 8 <= d <= 256
            and qkv.dtype in (torch.bfloat16, torch.float16, torch.float32) and qkv.dim() == 2 and qkv.stride(-1) == 1
            and qkv.data_ptr() % 16 == 0 and (qkv.stride(0) * qkv.element_size()) % 16 == 0
            and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)):
        if pos.dtype != torch.int32:
            pos = pos.to(torch.int32)
        return ops().kv_append_rope(qkv, cos.float().contiguous(), sin.float().contiguous(), pos.contiguous(),
                                    k_cache, v_cache)
    return kv_append_rope_ref(qkv, cos, sin, pos, k_cache, v_cache)


def decode_attention_chunk_ref(q, k_cache, v_cache, kv_len, scale=None):
    """``q`` (B, n, H, d): masked softmax of query ``i`` over its first ``kv_len[b] - (n - 1 - i)``
    keys, fp32 (or fp64) math. Cache rows no query reads are replaced before any arithmetic, so NaNs
    there cannot leak. Returns ``o`` (B, n, H, d) and ``lse`` (B, n, H) fp32."""
    B, n, H, d = q.shape
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    N = k_cache.shape[2]
    back = torch.arange(n - 1, -1, -1, device=q.device)  # n - 1 - i
    bound = (kv_len.to(torch.int64)[:, None] - back[None, :]).clamp(0, N)  # (B, n)
    valid = torch.arange(N, device=q.device)[None, None, :] < bound[:, :, None]  # (B, n, N)
    vm = valid[:, -1][:, None, :, None]  # the last query's range holds every other one
    k = torch.where(vm, k_cache.to(ct), 0.0)
    v = torch.where(vm, v_cache.to(ct), 0.0)
    s = torch.einsum("bnhd,bhkd->bnhk", q.to(ct), k) * scale
    s = torch.where(valid[:, :, None, :], s, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isinf(lse), 0.0, lse)[..., None])  # empty row: exp(-inf) = 0
    o = torch.einsum("bnhk,bhkd->bnhd", p, v)
    return o.to(q.dtype), lse.float()


def kv_append_rope_chunk_ref(qkv, cos, sin, pos, k_cache, v_cache):
    """No per-token loop and no host sync: every cache row picks its token (or keeps its value)."""
    B, H, max_len, d = k_cache.shape
    n = qkv.shape[1]
    q, k, v = (t.transpose(1, 2) for t in qkv.reshape(B, n, 3, H, d).unbind(2))  # (B, H, n, d)
    lim = min(max_len, cos.shape[0])
    slot = pos.to(torch.int64)[:, None] + torch.arange(n, device=qkv.device)[None, :]  # (B, n)
    ok = (slot >= 0) & (slot < lim)
    p = slot.clamp(0, lim - 1)
    q_rot = rope_ref(q, cos, sin, p[:, None, :])
    k_rot = rope_ref(k, cos, sin, p[:, None, :])
    # cache row r of sequence b takes token r - pos[b] if that is one of the chunk's and r has a slot
    r = torch.arange(max_len, device=qkv.device)[None, :]
    t = r - pos.to(torch.int64)[:, None]  # (B, max_len)
    take = ((t >= 0) & (t < n) & (r < lim))[:, None, :, None]
    idx = t.clamp(0, n - 1)[:, None, :, None].expand(B, H, max_len, d)
    k_cache.copy_(torch.where(take, k_rot.gather(2, idx).to(k_cache.dtype), k_cache))
    v_cache.copy_(torch.where(take, v.gather(2, idx).to(v_cache.dtype), v_cache))
    q_rot = torch.where(ok[:, None, :, None], q_rot, torch.zeros_like(q_rot))
    return q_rot.transpose(1, 2).contiguous()  # (B, n, H, d)


def kv_append_rope_chunk_kv8_ref(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale):
    """:func:`kv_append_rope_chunk_ref` on the FP8 format: K is rotated in fp32 and rounded once, by
    the quantizer; q is the sibling's."""
    B, H, max_len, d = k_cache.shape
    n = qkv.shape[1]
    q, k, v = (t.transpose(1, 2) for t in qkv.reshape(B, n, 3, H, d).unbind(2))  # (B, H, n, d)
    lim = min(max_len, cos.shape[0])
    slot = pos.to(torch.int64)[:, None] + torch.arange(n, device=qkv.device)[None, :]  # (B, n)
    ok = (slot >= 0) & (slot < lim)
    p = slot.clamp(0, lim - 1)
    q_rot = rope_ref(q, cos, sin, p[:, None, :])
    k_rot = rope_ref(k.float(), cos.float(), sin.float(), p[:, None, :])
    r = torch.arange(max_len, device=qkv.device)[None, :]
    t = r - pos.to(torch.int64)[:, None]  # (B, max_len)
    take = ((t >= 0) & (t < n) & (r < lim))[:, None, :, None]
    idx = t.clamp(0, n - 1)[:, None, :, None].expand(B, H, max_len, d)
    for x, plane, sp in ((k_rot, k_cache, k_scale), (v, v_cache, v_scale)):
        xq, xs = kv_quantize_ref(x)
        pb = plane.view(torch.uint8)  # (where / gather have no fp8 kernels)
        pb.copy_(torch.where(take, xq.view(torch.uint8).gather(2, idx), pb))
        sp.copy_(torch.where(take[..., 0], xs.gather(2, idx[..., 0]), sp))
    q_rot = torch.where(ok[:, None, :, None], q_rot, torch.zeros_like(q_rot))
    return q_rot.transpose(1, 2).contiguous()  # (B, n, H, d)


def decode_attention_chunk(q, k_cache, v_cache, kv_len, scale=None, max_kv_len=None, splits=0, *, k_scale=None,
                           v_scale=None):
    """``q`` (B, n, H, d) -> ``o`` (B, n, H, d), ``lse`` (B, n, H). ``max_kv_len``, ``splits`` and the
    scale planes as in :func:`decode_attention`."""
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
    if _kv8(k_cache, v_cache, k_scale, v_scale):
        if (use_hip(q, k_cache, v_cache) and d in _DECODE_D and q.dtype in (torch.bfloat16, torch.float16, torch.float32)
                and q.dim() == 4 and q.shape[1] >= 1 and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)
                and _scale_layout_ok(k_scale) and _scale_layout_ok(v_scale)):
            max_len = k_cache.shape[2]
            bound = max_len if max_kv_len is None else min(int(max_kv_len), max_len)
            if kv_len.dtype != torch.int32:
                kv_len = kv_len.to(torch.int32)
            return ops().fa_decode_chunk_kv8(q, k_cache, v_cache, k_scale, v_scale, kv_len.contiguous(), scale, bound,
                                             int(splits))
        return decode_attention_chunk_ref(q, kv_dequantize(k_cache, k_scale), kv_dequantize(v_cache, v_scale), kv_len,
                                          scale)
    if (use_hip(q, k_cache, v_cache) and d in _DECODE_D and q.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and q.dim() == 4 and q.shape[1] >= 1 and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)):
        max_len = k_cache.shape[2]
        bound = max_len if max_kv_len is None else min(int(max_kv_len), max_len)
        if kv_len.dtype != torch.int32:
            kv_len = kv_len.to(torch.int32)
        return ops().fa_decode_chunk(q, k_cache, v_cache, kv_len.contiguous(), scale, bound, int(splits))
    return decode_attention_chunk_ref(q, k_cache, v_cache, kv_len, scale)


def kv_append_rope_chunk(qkv, cos, sin, pos, k_cache, v_cache, *, k_scale=None, v_scale=None):
    d = k_cache.shape[-1]
    es = qkv.element_size()
    if _kv8(k_cache, v_cache, k_scale, v_scale):
        if (use_hip(qkv, k_cache, v_cache) and d in _DECODE_D
                and qkv.dtype in (torch.bfloat16, torch.float16, torch.float32) and qkv.dim() == 3 and qkv.shape[1] >= 1
                and qkv.stride(-1) == 1 and qkv.data_ptr() % 16 == 0
                and (qkv.stride(0) * es) % 16 == 0 and (qkv.stride(1) * es) % 16 == 0
                and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)
                and _scale_layout_ok(k_scale) and _scale_layout_ok(v_scale)):
            if pos.dtype != torch.int32:
                pos = pos.to(torch.int32)
            return ops().kv_append_rope_chunk_kv8(qkv, cos.float().contiguous(), sin.float().contiguous(),
                                                  pos.contiguous(), k_cache, v_cache, k_scale, v_scale)
        return kv_append_rope_chunk_kv8_ref(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    if (use_hip(qkv, k_cache, v_cache) and d % 8 == 0 and 8 <= d <= 256
            and qkv.dtype in (torch.bfloat16, torch.float16, torch.float32) and qkv.dim() == 3 and qkv.shape[1] >= 1
            and qkv.stride(-1) == 1 and qkv.data_ptr() % 16 == 0
            and (qkv.stride(0) * es) % 16 == 0 and (qkv.stride(1) * es) % 16 == 0
            and _cache_layout_ok(k_cache) and _cache_layout_ok(v_cache)):
        if pos.dtype != torch.int32:
            pos = pos.to(torch.int32)
        return ops().kv_append_rope_chunk(qkv, cos.float().contiguous(), sin.float().contiguous(), pos.contiguous(),
                                          k_cache, v_cache)
    return kv_append_rope_chunk_ref(qkv, cos, sin, pos, k_cache, v_cache)


# ---- paged cache (csrc/flash_attn/fa_decode_paged.hip) ----
_PAGE_SIZES = (16, 32, 64, 128, 256)


def paged_gather(pool, block_table):
    """The sequences' rows as a dense ``(B, H, T * P, d)`` tensor: ``pool`` ``(num_pages, H, P, d)``
    read through ``block_table`` ``(B, T)``. An entry outside ``[0, num_pages)`` reads some page of the
    pool (callers mask those rows by the length)."""
    NP, H, P, d = pool.shape
    B, T = block_table.shape
    g = pool[block_table.to(torch.int64).clamp(0, NP - 1)]  # (B, T, H, P, d)
    return g.permute(0, 2, 1, 3, 4).reshape(B, H, T * P, d)


def decode_attention_paged_ref(q, k_pool, v_pool, block_table, kv_len, scale=None):
    """:func:`decode_attention_ref` on the rows gathered by the table."""
    return decode_attention_ref(q, paged_gather(k_pool, block_table), paged_gather(v_pool, block_table), kv_len, scale)


def kv_append_rope_paged_ref(qkv, cos, sin, pos, k_pool, v_pool, block_table):
    """The rule of :func:`kv_append_rope_chunk_ref` with the slot looked up in the table: token ``i`` of
    sequence ``b`` is rotated at ``pos[b] + i`` and stored in row ``slot % P`` of page
    ``block_table[b, slot // P]``; a slot outside ``[0, min(T * P, ctx))`` or an entry outside
    ``[0, num_pages)`` stores nothing and zeroes the token's q. (The mask indexing reads back: this is the
    reference.)"""
    two_d = qkv.dim() == 2
    if two_d:
        qkv = qkv[:, None]
    NP, H, P, d = k_pool.shape
    B, n = qkv.shape[:2]
    T = block_table.shape[1]
    q, k, v = (t.transpose(1, 2) for t in qkv.reshape(B, n, 3, H, d).unbind(2))  # (B, H, n, d)
    lim = min(T * P, cos.shape[0])
    slot = pos.to(torch.int64)[:, None] + torch.arange(n, device=qkv.device)[None, :]  # (B, n)
    p = slot.clamp(0, lim - 1)
    page = block_table.to(torch.int64).gather(1, p // P)
    ok = (slot >= 0) & (slot < lim) & (page >= 0) & (page < NP)
    q_rot = rope_ref(q, cos, sin, p[:, None, :])
    k_rot = rope_ref(k, cos, sin, p[:, None, :])
    k_pool[page[ok], :, (p % P)[ok]] = k_rot.transpose(1, 2)[ok].to(k_pool.dtype)  # (tokens, H, d)
    v_pool[page[ok], :, (p % P)[ok]] = v.transpose(1, 2)[ok].to(v_pool.dtype)
    q_rot = torch.where(ok[:, None, :, None], q_rot, torch.zeros_like(q_rot)).transpose(1, 2).contiguous()
    return q_rot[:, 0] if two_d else q_rot  # (B, (n,) H, d)


def _paged_layout_ok(k_pool, v_pool, block_table) -> bool:
    return (_cache_layout_ok(k_pool) and _cache_layout_ok(v_pool) and k_pool.shape == v_pool.shape
            and k_pool.shape[2] in _PAGE_SIZES and block_table.dim() == 2 and block_table.stride(-1) == 1)


def decode_attention_paged(q, k_pool, v_pool, block_table, kv_len, scale=None, max_kv_len=None, splits=0):
    """:func:`decode_attention` on a paged cache: ``k_pool`` / ``v_pool`` ``(num_pages, H, P, d)`` views
    (``P`` in 16 ... 256; any page / head strides), ``block_table`` ``(B, T)`` int32 on the device, row
    ``j`` of sequence ``b`` being row ``j % P`` of page ``block_table[b, j // P]``. The table is read up
    to entry ``(kv_len[b] - 1) // P`` only; later entries may hold ``-1`` or stale ids. The result is a
    function of the logical rows: any placement of the pages gives the same bits. ``max_kv_len``
    (default ``T * P``) and ``splits`` as in :func:`decode_attention`."""
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
    if (use_hip(q, k_pool, v_pool) and d in _DECODE_D and q.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and _paged_layout_ok(k_pool, v_pool, block_table)):
        max_len = block_table.shape[1] * k_pool.shape[2]
        bound = max_len if max_kv_len is None else min(int(max_kv_len), max_len)
        if kv_len.dtype != torch.int32:
            kv_len = kv_len.to(torch.int32)
        if block_table.dtype != torch.int32:
            block_table = block_table.to(torch.int32)
        return ops().fa_decode_paged(q, k_pool, v_pool, block_table, kv_len.contiguous(), scale, bound, int(splits))
    return decode_attention_paged_ref(q, k_pool, v_pool, block_table, kv_len, scale)


def kv_append_rope_paged(qkv, cos, sin, pos, k_pool, v_pool, block_table):
    """``qkv`` ``(B, 3*H*d)`` (one token, the decode step) or ``(B, n, 3*H*d)`` -> rotated q ``(B, H, d)``
    / ``(B, n, H, d)``; rotated k and plain v are written through the table (see
    :func:`kv_append_rope_paged_ref` for what is not stored)."""
    d = k_pool.shape[-1]
    es = qkv.element_size()
    q3 = qkv[:, None] if qkv.dim() == 2 else qkv
    if (use_hip(qkv, k_pool, v_pool) and d in _DECODE_D
            and qkv.dtype in (torch.bfloat16, torch.float16, torch.float32) and q3.dim() == 3 and q3.shape[1] >= 1
            and q3.stride(-1) == 1 and q3.data_ptr() % 16 == 0
            and (q3.stride(0) * es) % 16 == 0 and (q3.stride(1) * es) % 16 == 0
            and _paged_layout_ok(k_pool, v_pool, block_table)):
        if pos.dtype != torch.int32:
            pos = pos.to(torch.int32)
        if block_table.dtype != torch.int32:
            block_table = block_table.to(torch.int32)
        out = ops().kv_append_rope_paged(q3, cos.float().contiguous(), sin.float().contiguous(), pos.contiguous(),
                                         k_pool, v_pool, block_table)
        return out[:, 0] if qkv.dim() == 2 else out
    return kv_append_rope_paged_ref(qkv, cos, sin, pos, k_pool, v_pool, block_table)
