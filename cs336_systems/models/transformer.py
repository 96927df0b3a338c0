"""Transformer LM (pre-norm, RMSNorm, RoPE, SwiGLU, causal MHA) with MI355X kernel dispatch.

Architecture and parameter layout are identical to the reference's bundled model
(``cs336-basics/cs336_basics/model.py:22-397``) so state dicts and the on-disk checkpoint format
(``model_config.json`` + ``model.pt``, ``model.py:312-327``) interchange. What differs is the
execution path on GPU:

* every projection is ``F.linear`` → hipBLASLt bf16 GEMM under autocast;
* RMSNorm / RoPE / SwiGLU gate / cross-entropy are the fused HIP kernels of ``cs336_systems.ops``;
  RMSNorm writes its output straight in the autocast dtype;
* attention never materializes N x N and never transposes: Q/K/V stay in the ``(B, N, H, D)``
  memory order the projections produce, RoPE writes ``(B, N, H, D)``, the HIP FlashAttention-2
  kernels read/write strided ``(B, H, N, D)`` views of it, and the output projection consumes the
  result as a plain ``(B, N, H*D)`` view.

On CPU everything falls back to the eager reference math (naive masked softmax attention), which
is what the CPU plumbing config of BASELINE.json exercises.
"""

from __future__ import annotations

import json
import logging
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops import gemm as _gemm
from ..ops.rope import _normalize_pos
from ..utils.profiling import annotate
from . import compiled, fused

logger = logging.getLogger(__name__)

# tests only: take the torch.compile custom-op path on CPU too (the ops run their reference math)
_COMPILE_CPU_OPS = False

# "auto": HIP flash attention on GPU, naive on CPU; "naive": always materialize; "flash": always
# the FA2 path (HIP on GPU, tiled PyTorch on CPU).
_ATTN_IMPL = os.environ.get("CS336_ATTN_IMPL", "auto")


def set_attention_impl(name: str) -> None:
    global _ATTN_IMPL
    if name not in ("auto", "naive", "flash"):
        raise ValueError(name)
    _ATTN_IMPL = name


def get_attention_impl() -> str:
    return _ATTN_IMPL


def _trunc_normal(shape, std, device=None, dtype=None):
    t = torch.empty(shape, device=device, dtype=dtype or torch.float32)
    return nn.init.trunc_normal_(t, std=std, a=-3 * std, b=3 * std)


class Linear(nn.Module):
    """Bias-free linear, weight ``(d_out, d_in)``, trunc-normal std sqrt(2/(d_in+d_out)) (``model.py:22-44``)."""

    def __init__(self, d_in: int, d_out: int, device=None, dtype=None):
        super().__init__()
        std = math.sqrt(2 / (d_in + d_out))
        self.weight = nn.Parameter(_trunc_normal((d_out, d_in), std, device, dtype), requires_grad=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.compiler.is_compiling() and (x.is_cuda or _COMPILE_CPU_OPS):
            # traced by torch.compile: the opaque custom op (models/compiled.py), not the eager
            # autograd Function (shadow / stream bookkeeping Dynamo cannot trace)
            cdt = torch.get_autocast_dtype(x.device.type) if torch.is_autocast_enabled(x.device.type) else self.weight.dtype
            y = compiled.linear(x.reshape(-1, x.shape[-1]), [self.weight], cdt)
            return y.view(*x.shape[:-1], y.shape[-1])
        if x.is_cuda:
            return fused.fused_linear(x, self.weight)
        y = _gemm.quantized_linear(x, self.weight)  # inside gemm.skinny_decode(weights=...): the quantized copy
        if y is not None:
            return y
        return F.linear(x, self.weight)

    def extra_repr(self):
        return f"d_out={self.weight.shape[0]}, d_in={self.weight.shape[1]}"


class _GraphSafeEmbedding(torch.autograd.Function):
    """Embedding lookup whose backward does not depend on the token set's size: on GPU the
    deterministic HIP kernel (``csrc/ops/embedding.hip``: stable sort of the ids, one workgroup per
    vocabulary row summing its positions' gradient rows in order), else one ``index_add_`` into a
    zeroed table. ATen's embedding backward sorts and partitions the token ids with data-dependent
    sizes; replaying a HIP graph captured around it faulted in rocprim's partition kernel at the XL
    shape. The HIP form is used for every GPU lookup (eager and captured steps then produce the same
    bits: ``tests/test_graphs_gpu.py``) and writes into the DDP bucket view when there is one
    (``parallel/ddp.py``: no adopt copy of the 64 MB XL table gradient)."""

    @staticmethod
    def forward(ctx, ids, weight):
        ctx.save_for_backward(ids)
        ctx.wshape, ctx.wdtype = weight.shape, weight.dtype
        ctx.wparam = weight
        return F.embedding(ids, weight)

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        V, D = ctx.wshape
        g2 = g.reshape(-1, D)
        if D % 4 == 0 and ops.use_hip(g2):
            if not g2.is_contiguous():
                g2 = g2.contiguous()
            sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True)
            tgt = getattr(ctx.wparam, "_cs336_grad_out", None)
            if (tgt is not None and ctx.wparam.grad is None and tgt.dtype == torch.float32 and tgt.is_contiguous()
                    and tuple(tgt.shape) == (V, D)):
                torch.ops.cs336.embedding_bwd_into(g2, sorted_ids, perm, tgt)
                return None, tgt.view_as(tgt)  # a fresh alias: adopted as .grad without a copy
            gw = torch.ops.cs336.embedding_bwd(g2, sorted_ids, perm, V)
        else:
            gw = torch.zeros(ctx.wshape, dtype=torch.float32, device=g.device)
            gw.index_add_(0, ids.reshape(-1), g2.float())
        return None, gw if ctx.wdtype == torch.float32 else gw.to(ctx.wdtype)


class Embedding(nn.Module):
    """Token embedding table ``(vocab, d_model)``, trunc-normal std 1 (``model.py:47-60``)."""

    def __init__(self, vocab_size: int, d_model: int, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(_trunc_normal((vocab_size, d_model), 1.0, device, dtype), requires_grad=True)

    def forward(self, token_ids: torch.Tensor) -> torch.Tensor:
        if torch.compiler.is_compiling():
            if token_ids.is_cuda and ops.get_backend() != "torch":
                return compiled.embedding(token_ids, self.weight)  # the same HIP backward, traceable
            return F.embedding(token_ids, self.weight)
        if token_ids.is_cuda and (ops.get_backend() != "torch" or torch.cuda.is_current_stream_capturing()):
            return _GraphSafeEmbedding.apply(token_ids, self.weight)
        return F.embedding(token_ids, self.weight)

    def extra_repr(self):
        return f"vocab_size={self.weight.shape[0]}, d={self.weight.shape[1]}"


class RMSNorm(nn.Module):
    """RMSNorm (``model.py:63-110``); HIP kernel on GPU (``csrc/ops/rmsnorm.hip``)."""

    def __init__(self, hidden_size: int, eps: float = 1e-5, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.eps = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.eps)

    def extra_repr(self):
        return f"hidden_size={self.weight.shape[0]}, eps={self.eps}"


class RotaryEmbedding(nn.Module):
    """RoPE with a ``(2, ctx, d/2)`` cos/sin cache (``model.py:113-150``)."""

    def __init__(self, context_length: int, dim: int, theta: float = 10000.0, device=None):
        super().__init__()
        self.register_buffer("_freq_cis_cache", RotaryEmbedding._init_cache(context_length, dim, theta, device), persistent=False)

    @staticmethod
    def _init_cache(context_length: int, dim: int, theta: float, device=None) -> torch.Tensor:
        assert dim % 2 == 0
        d = torch.arange(0, dim, 2, device=device) / dim
        freqs = theta**-d
        t = torch.arange(context_length, device=device)
        freqs = torch.outer(t, freqs)
        return torch.stack((torch.cos(freqs), torch.sin(freqs)))

    @property
    def cos(self):
        return self._freq_cis_cache[0]

    @property
    def sin(self):
        return self._freq_cis_cache[1]

    def forward(self, x: torch.Tensor, pos_ids: torch.Tensor | None = None) -> torch.Tensor:
        return ops.rope(x, self.cos, self.sin, pos_ids)

    def extra_repr(self):
        return f"context_length={self._freq_cis_cache.shape[1]}, dim/2={self._freq_cis_cache.shape[2]}"


def silu(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(x)


class SwiGLU(nn.Module):
    """``w2(silu(w1 x) * w3 x)`` (``model.py:389-397``); the gate is one HIP kernel on GPU."""

    def __init__(self, d_model: int, d_ff: int, device=None, dtype=None):
        super().__init__()
        self.w1 = Linear(d_model, d_ff, device, dtype)
        self.w2 = Linear(d_ff, d_model, device, dtype)
        self.w3 = Linear(d_model, d_ff, device, dtype)

    def _fused_ffn_ok(self, x) -> bool:
        """bf16 compute (autocast or bf16 weights) on the HIP path and a tiling gemm8 takes: tokens a
        multiple of 256, d_ff of 160 or 128; anything else runs GEMM + the separate gate kernel."""
        cdt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else self.w1.weight.dtype
        tokens = x.numel() // x.shape[-1]
        d_ff, d_model = self.w1.weight.shape
        return (cdt == torch.bfloat16 and tokens % 256 == 0 and (d_ff % 160 == 0 or d_ff % 128 == 0)
                and d_model % 64 == 0 and ops.ext_available())

    def group_(self) -> None:
        """Store w1 and w3 as one (2*d_ff, d_model) block so the gate projections are one GEMM."""
        fused.group_params_([self.w1.weight, self.w3.weight])

    def forward(self, x):
        if x.is_cuda and ops.use_hip(x) and fused.grouped_view([self.w1.weight, self.w3.weight]) is not None:
            if fused.swiglu_fused_enabled() and self._fused_ffn_ok(x):
                # gate in the GEMM epilogues: y/h from one kernel, [da|db] from the W2 input-grad GEMM
                return fused.SwiGLUFFNFn.apply(x, self.w1.weight, self.w3.weight, self.w2.weight)
            y = fused.fused_linear(x, self.w1.weight, self.w3.weight)  # [a | b], (..., 2*d_ff)
            return self.w2(fused.SwiGLUGate.apply(y))
        return self.w2(ops.silu_mul(self.w1(x), self.w3(x)))


def softmax(x: torch.Tensor, dim: int = -1) -> torch.Tensor:
    rescaled = x - torch.max(x, dim=dim, keepdim=True)[0]
    e = torch.exp(rescaled)
    return e / torch.sum(e, dim=dim, keepdim=True)


def scaled_dot_product_attention(Q, K, V, mask=None):
    """Materializing SDPA (``model.py:400-432``): mask==False positions get -inf."""
    d_k = K.shape[-1]
    scores = torch.matmul(Q, K.transpose(-1, -2)) / math.sqrt(d_k)
    if mask is not None:
        scores = torch.where(mask, scores, float("-inf"))
    return torch.matmul(softmax(scores, dim=-1), V)


class CausalMultiHeadSelfAttention(nn.Module):
    """Causal MHA with RoPE on Q and K (``model.py:435-524``)."""

    def __init__(self, d_model: int, num_heads: int, positional_encoder: RotaryEmbedding, device=None, dtype=None):
        super().__init__()
        assert d_model % num_heads == 0
        self.d_model = d_model
        self.num_heads = num_heads
        self.d_k = d_model // num_heads
        self.d_v = self.d_k
        self.q_proj = Linear(d_model, num_heads * self.d_k, device, dtype)
        self.k_proj = Linear(d_model, num_heads * self.d_k, device, dtype)
        self.v_proj = Linear(d_model, num_heads * self.d_v, device, dtype)
        self.output_proj = Linear(num_heads * self.d_v, d_model, device, dtype)
        self.positional_encoder = positional_encoder
        # (process group, layout) once parallel.context_parallel.enable_context_parallel() is applied
        self.context_parallel = None

    def group_(self) -> None:
        """Store q/k/v projections as one (3*d_model, d_model) block (one QKV GEMM)."""
        fused.group_params_([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight])

    def _fused_path(self, x3, pos, B, N):
        """GPU path over the grouped QKV weight: one GEMM -> RoPE + FA2 on strided views -> o."""
        w = [self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]
        if _ATTN_IMPL == "naive" or not ops.use_hip(x3) or self.d_k not in (32, 64, 80, 128):
            return None
        cdt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else x3.dtype
        if self.d_k == 80 and cdt not in (torch.bfloat16, torch.float16):
            return None  # d_head 80 is native for 16-bit only; fp32 takes the padded FA2 path below
        if fused.grouped_view(w) is None:
            return None
        p = _normalize_pos(pos, B, N)
        if isinstance(p, str):
            return None
        cos, sin = self.positional_encoder.cos.float().contiguous(), self.positional_encoder.sin.float().contiguous()
        if p is None and N > cos.shape[0]:
            return None
        with annotate("qkv_proj"):
            # (the Function falls back to GEMM + in-place RoPE where gemm8 does not take the shape)
            prerot = cdt == torch.bfloat16 and self.d_k % 8 == 0 and _gemm.qkv_rope_enabled()
            if prerot:  # RoPE on q|k inside the QKV GEMM's store
                qkv = fused.QKVRopeLinearFn.apply(x3, cos, sin, p, self.num_heads, *w)
            else:
                qkv = fused.fused_linear(x3, *w)  # (B, N, 3*H*dk)
        with annotate("attention"):
            want_ot = (
                fused.attn_out_transposed()
                and qkv.dtype in (torch.bfloat16, torch.float16)
                and self.output_proj.weight.requires_grad
                and torch.is_grad_enabled()
            )
            return fused.AttentionCore.apply(qkv, cos, sin, p, self.num_heads, want_ot, prerot)

    def _context_parallel_forward(self, x3, token_positions, B, N):
        """Ring attention over the context-parallel group (``parallel/context_parallel.py``): x3 is
        this rank's part of the sequence; RoPE uses the tokens' global positions."""
        from ..parallel.context_parallel import _world_rank, ring_attention, sequence_positions, ulysses_attention

        group, layout = self.context_parallel
        H, dk = self.num_heads, self.d_k
        with annotate("qkv_proj"):
            q = self.q_proj(x3).view(B, N, H, dk).transpose(1, 2)
            k = self.k_proj(x3).view(B, N, H, dk).transpose(1, 2)
            v = self.v_proj(x3).view(B, N, H, dk).transpose(1, 2)
        if token_positions is None:
            world, rank = _world_rank(group)
            pos = sequence_positions(N * world, rank, world, layout, device=x3.device)
        else:
            pos = token_positions.reshape(-1, N) if token_positions.numel() != N else token_positions.reshape(N)
        with annotate("rope"):
            q = self.positional_encoder(q, pos)
            k = self.positional_encoder(k, pos)
        if layout == "ulysses":
            with annotate("ulysses_attention"):
                return ulysses_attention(q, k.to(q.dtype), v.to(q.dtype), group, True)
        with annotate("ring_attention"):
            return ring_attention(q, k.to(q.dtype), v.to(q.dtype), group, True, layout)

    def forward(self, x: torch.Tensor, token_positions: torch.Tensor | None = None) -> torch.Tensor:
        *b, N, d_model = x.shape
        assert d_model == self.d_model
        B = int(math.prod(b)) if b else 1
        H, dk = self.num_heads, self.d_k
        x3 = x.reshape(B, N, d_model)
        if self.context_parallel is not None:
            o = self._context_parallel_forward(x3, token_positions, B, N)
            o = o.transpose(1, 2).reshape(*b, N, H * dk) if b else o.transpose(1, 2).reshape(N, H * dk)
            with annotate("out_proj"):
                return self.output_proj(o)
        if x.is_cuda:
            res = self._fused_path(x3, token_positions, B, N)
            if res is not None:
                o, ot = res
                o = o.transpose(1, 2).reshape(*b, N, H * dk) if b else o.transpose(1, 2).reshape(N, H * dk)
                with annotate("out_proj"):
                    op = self.output_proj
                    if (ot is not None and type(op).forward is Linear.forward and not op._forward_pre_hooks
                            and not op._forward_hooks):
                        return fused.fused_linear(o, op.weight, xt=ot)
                    return self.output_proj(o)
        # (B, N, H, dk) memory, viewed as (B, H, N, dk): no transpose copies on the GPU path
        with annotate("qkv_proj"):
            w = [self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]
            if x.is_cuda and fused.grouped_view(w) is not None:
                # head dims the fused attention core does not take (e.g. 80 in the 2.7b model) still
                # get the single grouped QKV GEMM; q/k/v are strided views of its output
                qkv = fused.fused_linear(x3, *w).view(B, N, 3, H, dk)
                q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
            else:
                q = self.q_proj(x3).view(B, N, H, dk).transpose(1, 2)
                k = self.k_proj(x3).view(B, N, H, dk).transpose(1, 2)
                v = self.v_proj(x3).view(B, N, H, dk).transpose(1, 2)
        pos = token_positions
        if pos is not None:
            pos = pos.reshape(-1, N) if pos.numel() != N else pos.reshape(N)
        with annotate("rope"):
            q = self.positional_encoder(q, pos)
            k = self.positional_encoder(k, pos)
        impl = _ATTN_IMPL
        with annotate("attention"):
            if impl == "naive" or (impl == "auto" and not x.is_cuda):
                seq = torch.arange(N, device=x.device)
                mask = seq[:, None] >= seq[None, :]
                o = scaled_dot_product_attention(q, k, v, mask)
            elif x.is_cuda:
                o = ops.flash_attention(q, k.to(q.dtype), v.to(q.dtype), is_causal=True)
            else:
                o = ops.FlashAttentionTorch.apply(q, k, v, True)
        o = o.transpose(1, 2).reshape(*b, N, H * dk) if b else o.transpose(1, 2).reshape(N, H * dk)
        with annotate("out_proj"):
            return self.output_proj(o)

    def forward_cached(self, x3, k_cache, v_cache, start: int, pos=None, kv_len=None, max_kv_len=None,
                       k_scale=None, v_scale=None, block_table=None) -> torch.Tensor:
        """Attention of ``forward_cached`` (inference only). ``x3`` (B, n, d_model); ``k_cache`` /
        ``v_cache`` this layer's (B, H, max_len, dk) cache views. ``start == 0``: prefill -- the
        ordinary causal attention over the n tokens at positions 0..n-1, whose rotated K and V are
        copied into cache rows [0, n). Otherwise one decode step (n == 1): ``pos`` (B,) int32 is the
        new token's slot and RoPE position, ``kv_len = pos + 1`` its key count; or a chunk step
        (n > 1) over the chunk ops: ``pos`` is the slot of the chunk's first token, ``kv_len = pos + n``
        the key count of its last. ``max_kv_len``: the host-side bound of ``kv_len`` that picks the
        decode kernel's split count (default ``start + n``; a captured step passes a fixed one).
        ``k_scale`` / ``v_scale``: this layer's (B, H, max_len) scale views of an FP8 cache
        (``float8_e4m3fn`` planes): the steps append and read quantized rows, and the prefill, which
        attends to its own unquantized K / V, stores them through ``ops.kv_quantize_rows``.
        ``block_table`` (B, pages per sequence) int32: ``k_cache`` / ``v_cache`` are this layer's
        (num_pages, H, page_size, dk) pool views of a ``PagedKVCache`` whose pages for the new rows are
        reserved; the step runs the paged ops and the prefill stores its rows through the table."""
        B, n, _ = x3.shape
        H, dk = self.num_heads, self.d_k
        w = [self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]
        with annotate("qkv_proj"):
            if x3.is_cuda and fused.grouped_view(w) is not None:
                qkv = fused.fused_linear(x3, *w)  # one grouped QKV GEMM, (B, n, 3*H*dk)
            else:
                qkv = torch.cat([self.q_proj(x3), self.k_proj(x3), self.v_proj(x3)], dim=-1)
        fp8 = k_cache.dtype == torch.float8_e4m3fn
        if fp8 and (k_scale is None or v_scale is None):
            raise ValueError("an FP8 KV cache needs its k_scale / v_scale views")
        sc = dict(k_scale=k_scale, v_scale=v_scale) if fp8 else {}
        if not fp8 and qkv.dtype != k_cache.dtype:
            raise ValueError(f"KV cache dtype {k_cache.dtype} does not match the compute dtype {qkv.dtype}")
        if block_table is not None and start > 0:
            if n > 1:
                raise NotImplementedError("a paged KV cache has no chunk step (n > 1 on a non-empty cache)")
            with annotate("kv_append_rope_paged"):
                q = ops.kv_append_rope_paged(qkv.view(B, 3 * H * dk), self.positional_encoder.cos,
                                             self.positional_encoder.sin, pos, k_cache, v_cache, block_table)
            with annotate("decode_attention_paged"):
                o, _ = ops.decode_attention_paged(q, k_cache, v_cache, block_table, kv_len,
                                                  max_kv_len=start + 1 if max_kv_len is None else max_kv_len)
            o = o.reshape(B, 1, H * dk)
        elif start > 0 and n > 1:
            with annotate("kv_append_rope_chunk"):
                q = ops.kv_append_rope_chunk(qkv, self.positional_encoder.cos, self.positional_encoder.sin, pos,
                                             k_cache, v_cache, **sc)
            with annotate("decode_attention_chunk"):
                o, _ = ops.decode_attention_chunk(q, k_cache, v_cache, kv_len,
                                                  max_kv_len=start + n if max_kv_len is None else max_kv_len, **sc)
            o = o.reshape(B, n, H * dk)
        elif start > 0:
            with annotate("kv_append_rope"):
                q = ops.kv_append_rope(qkv.view(B, 3 * H * dk), self.positional_encoder.cos, self.positional_encoder.sin,
                                       pos, k_cache, v_cache, **sc)
            with annotate("decode_attention"):
                o, _ = ops.decode_attention(q, k_cache, v_cache, kv_len,
                                            max_kv_len=start + 1 if max_kv_len is None else max_kv_len, **sc)
            o = o.reshape(B, 1, H * dk)
        else:
            q, k, v = (qkv.view(B, n, 3, H, dk)[:, :, i].transpose(1, 2) for i in range(3))
            with annotate("rope"):
                q = self.positional_encoder(q, None)
                k = self.positional_encoder(k, None)
            if block_table is not None:
                # one index_put_ per plane over (page of row r, :, r % P): no host sync
                P = k_cache.shape[2]
                r = torch.arange(n, device=x3.device)
                pages = block_table[:, r // P].to(torch.int64)  # (B, n)
                slots = (r % P)[None, :].expand(B, n)
                k_cache[pages, :, slots] = k.transpose(1, 2).to(k_cache.dtype)  # (B, n, H, dk)
                v_cache[pages, :, slots] = v.transpose(1, 2).to(v_cache.dtype)
            elif fp8:
                with annotate("kv_quantize_rows"):
                    ops.kv_quantize_rows(k, k_cache, k_scale)
                    ops.kv_quantize_rows(v, v_cache, v_scale)
            else:
                k_cache[:, :, :n].copy_(k)
                v_cache[:, :, :n].copy_(v)
            impl = _ATTN_IMPL
            with annotate("attention"):
                if impl == "naive" or (impl == "auto" and not x3.is_cuda):
                    seq = torch.arange(n, device=x3.device)
                    o = scaled_dot_product_attention(q, k, v, seq[:, None] >= seq[None, :])
                elif x3.is_cuda:
                    o = ops.flash_attention(q, k.to(q.dtype), v.to(q.dtype), is_causal=True)
                else:
                    o = ops.FlashAttentionTorch.apply(q, k, v, True)
            o = o.transpose(1, 2).reshape(B, n, H * dk)
        with annotate("out_proj"):
            return self.output_proj(o)


class TransformerBlock(nn.Module):
    """Pre-norm block: ``x + attn(ln1(x))`` then ``+ ffn(ln2(.))`` (``model.py:330-386``)."""

    def __init__(self, d_model: int, num_heads: int, d_ff: int, positional_encoder: RotaryEmbedding, device=None, dtype=None):
        super().__init__()
        self.attn = CausalMultiHeadSelfAttention(d_model, num_heads, positional_encoder, device, dtype)
        self.ffn = SwiGLU(d_model, d_ff, device, dtype)
        self.ln1 = RMSNorm(d_model, device=device, dtype=dtype)
        self.ln2 = RMSNorm(d_model, device=device, dtype=dtype)

    def forward(self, x: torch.Tensor, token_positions: torch.Tensor | None = None):
        with annotate("block.attn"):
            h = x + self.attn(self.ln1(x), token_positions)
        with annotate("block.ffn"):
            return h + self.ffn(self.ln2(h))


class BasicsTransformerLM(nn.Module):
    """Transformer LM with the reference constructor (``model.py:153-191``).

    ``self.config`` holds exactly the constructor kwargs (serialized to ``model_config.json``).
    """

    def __init__(
        self,
        vocab_size: int,
        context_length: int,
        d_model: int,
        num_layers: int,
        num_heads: int,
        d_ff: int,
        rope_theta: float = 10000.0,
        *,
        device=None,
        dtype=None,
        fused_layout: bool = True,
    ):
        self.config = dict(
            vocab_size=vocab_size,
            context_length=context_length,
            d_model=d_model,
            num_layers=num_layers,
            num_heads=num_heads,
            d_ff=d_ff,
            rope_theta=rope_theta,
        )
        super().__init__()
        self._fused_layout = fused_layout
        self.vocab_size = vocab_size
        self.context_length = context_length
        self.d_model = d_model
        self.token_embeddings = Embedding(vocab_size, d_model, device, dtype)
        self.positional_encoder = RotaryEmbedding(context_length, d_model // num_heads, rope_theta, device)
        self.layers = nn.ModuleList(
            [TransformerBlock(d_model, num_heads, d_ff, self.positional_encoder, device, dtype) for _ in range(num_layers)]
        )
        self.ln_final = RMSNorm(d_model, device=device, dtype=dtype)
        self.lm_head = Linear(d_model, vocab_size, device, dtype)
        if fused_layout:
            self.regroup_()
        logger.info(f"number of non-embedding parameters: {self.get_num_params() / 1e6:.2f}M")

    def regroup_(self) -> "BasicsTransformerLM":
        """(Re)establish the grouped QKV / W1|W3 storage (e.g. after ``.to(device)``, which gives
        every parameter its own storage). Parameter objects, names and values are unchanged."""
        for layer in self.layers:
            layer.attn.group_()
            layer.ffn.group_()
        return self

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if getattr(self, "_fused_layout", False) and hasattr(self, "layers"):
            self.regroup_()
        return out

    def get_num_params(self, non_embedding: bool = True) -> int:
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.lm_head.weight.numel()
        return n

    def forward(self, x: torch.Tensor, token_positions: torch.Tensor | None = None) -> torch.Tensor:
        with annotate("embed"):
            h = self.token_embeddings(x)
        if torch.compiler.is_compiling() and token_positions is None and self._compiled_path_ok(h):
            return self._forward_compiled(h)
        if self._fused_residual_ok(h):
            return self._forward_fused_residual(h, token_positions)
        for i, layer in enumerate(self.layers):
            with annotate(f"layer{i}"):
                h = layer(h, token_positions)
        with annotate("lm_head"):
            return self.lm_head(self.ln_final(h))

    def register_param_read_hook(self, fn) -> None:
        """``fn(module)`` runs right before the fused-residual path reads ``module``'s parameters
        WITHOUT calling its forward (the ln2 / next-ln1 / ln_final gains consumed by the fused
        add+RMSNorm kernel), so forward pre-hooks would never see those reads. ZeRO-2 uses it to
        wait for the all-gather of the bucket those weights live in (parallel/zero.py)."""
        self.__dict__.setdefault("_param_read_hooks", []).append(fn)

    def _reading(self, module: nn.Module) -> None:
        for fn in self.__dict__.get("_param_read_hooks", ()):
            fn(module)

    def _fused_residual_ok(self, h: torch.Tensor) -> bool:
        """The chained add+norm path needs the stock block/norm modules (no overridden forward,
        e.g. the annotated or user-patched variants) and the HIP kernels (or, for tests, an
        explicit ``_force_fused_residual`` on CPU where ``ops.add_rmsnorm`` runs the eager ops)."""
        if self.__dict__.get("_force_fused_residual") and len(self.layers):
            return True
        if not (len(self.layers) and ops.use_hip(h)):
            return False
        norms = [self.ln_final] + [m for layer in self.layers for m in (layer.ln1, layer.ln2)]
        return all(type(layer).forward is TransformerBlock.forward for layer in self.layers) and all(
            type(n).forward is RMSNorm.forward for n in norms
        )

    def _compiled_path_ok(self, h: torch.Tensor) -> bool:
        """torch.compile path over the custom ops of models/compiled.py: bf16 autocast (or bf16
        weights), the stock modules and the grouped QKV / W1|W3 layout (the ops' inputs are the
        parameters themselves), HIP tensors (or, for the CPU tests, ``_COMPILE_CPU_OPS``)."""
        if not (len(self.layers) and (h.is_cuda or _COMPILE_CPU_OPS)):
            return False
        dev = h.device.type
        cdt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else self.lm_head.weight.dtype
        if cdt != torch.bfloat16 or (not self._fused_residual_ok(h) and not _COMPILE_CPU_OPS):
            return False
        a0 = self.layers[0].attn
        return a0.d_k % 8 == 0 and a0.d_k <= 128 and a0.context_parallel is None and all(
            type(layer.attn).forward is CausalMultiHeadSelfAttention.forward
            and type(layer.ffn).forward is SwiGLU.forward for layer in self.layers)

    def _forward_compiled(self, h: torch.Tensor) -> torch.Tensor:
        """The fused-residual block loop of :meth:`_forward_fused_residual` over the custom ops of
        ``models/compiled.py`` (fused QKV + RoPE GEMM, FA2, output projection, SwiGLU FFN with the
        gate in the GEMM epilogues), which torch.compile traces with no graph break."""
        B, N, D = h.shape
        cos = self.positional_encoder.cos.float().contiguous()
        sin = self.positional_encoder.sin.float().contiguous()
        n_layers = len(self.layers)
        y = self.layers[0].ln1(h)
        for i, layer in enumerate(self.layers):
            at = layer.attn
            qkv = compiled.qkv_rope(y.reshape(B * N, D), [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight],
                                    cos, sin, N, at.num_heads)
            o, _ = compiled.attn(qkv.view(B, N, -1), cos, sin, at.num_heads)
            o = o.transpose(1, 2).reshape(B * N, at.num_heads * at.d_k)
            a = compiled.linear(o, [at.output_proj.weight], torch.bfloat16).view(B, N, D)
            self._reading(layer.ln2)
            h, y = ops.add_rmsnorm(h, a, layer.ln2.weight, layer.ln2.eps)
            ff = layer.ffn
            f, _, _ = compiled.swiglu_ffn(y.reshape(B * N, D), ff.w1.weight, ff.w3.weight, ff.w2.weight)
            nxt = self.layers[i + 1].ln1 if i + 1 < n_layers else self.ln_final
            self._reading(nxt)
            h, y = ops.add_rmsnorm(h, f.view(B, N, D), nxt.weight, nxt.eps)
        logits = compiled.linear(y.reshape(B * N, D), [self.lm_head.weight], torch.bfloat16)
        return logits.view(B, N, -1)

    def _forward_fused_residual(self, h: torch.Tensor, token_positions: torch.Tensor | None) -> torch.Tensor:
        """Same math as the block loop, but each residual add is fused with the norm that reads
        its result (``ln2`` of the same block, ``ln1`` of the next, ``ln_final`` after the last):
        the fp32 residual stream is read once per add instead of twice, and in backward the
        residual gradient is accumulated inside the RMSNorm-backward kernel."""
        n_layers = len(self.layers)
        y = self.layers[0].ln1(h)
        for i, layer in enumerate(self.layers):
            with annotate(f"layer{i}"):
                with annotate("block.attn"):
                    a = layer.attn(y, token_positions)
                    self._reading(layer.ln2)
                    h, y = ops.add_rmsnorm(h, a, layer.ln2.weight, layer.ln2.eps)
                with annotate("block.ffn"):
                    f = layer.ffn(y)
                    nxt = self.layers[i + 1].ln1 if i + 1 < n_layers else self.ln_final
                    self._reading(nxt)
                    h, y = ops.add_rmsnorm(h, f, nxt.weight, nxt.eps)
        with annotate("lm_head"):
            return self.lm_head(y)

    @torch.no_grad()
    def forward_cached(self, x: torch.Tensor, cache, chunk: bool = False) -> torch.Tensor:
        """Logits ``(B, n, vocab)`` of the ``n`` tokens ``x`` that follow the ``cache.length`` tokens
        already in ``cache`` (a :class:`~cs336_systems.models.kv_cache.KVCache`); the cache then
        holds them too. On an empty cache this is the prefill (any ``n >= 1``: the ordinary forward,
        with every layer's rotated K and V copied into the cache); afterwards one token per call
        (``n == 1``): per layer the QKV projection of that token alone, ``ops.kv_append_rope`` and
        ``ops.decode_attention`` over the cached keys -- O(1) projection and O(length) attention work
        per token instead of a forward over the whole window.

        ``chunk=True`` also takes ``n > 1`` tokens on a non-empty cache (a follow-up prompt, a prefill
        in chunks, the verify step of speculative decoding): per layer the QKV projection of the n
        tokens, ``ops.kv_append_rope_chunk`` and ``ops.decode_attention_chunk``, in which token ``i``
        attends to the cached keys and the chunk's tokens up to itself. ``n == 1`` and the prefill
        take the same paths whatever ``chunk`` is.

        ``cache`` may be a :class:`~cs336_systems.models.kv_cache.PagedKVCache`: the pages for the new
        tokens are reserved first (``cache.reserve(n)``; ``RuntimeError`` when the pool is exhausted),
        the prefill stores its rows through the block table and a step runs ``ops.kv_append_rope_paged``
        and ``ops.decode_attention_paged``. ``chunk=True`` raises ``NotImplementedError`` on it."""
        if getattr(self, "tensor_parallel", None) is not None or any(
                layer.attn.context_parallel is not None for layer in self.layers):
            raise NotImplementedError("forward_cached does not support tensor / context parallelism")
        if x.dim() != 2:
            raise ValueError("forward_cached takes (B, n) token ids")
        B, n = x.shape
        if B != cache.batch:
            raise ValueError(f"batch {B} does not match the cache's {cache.batch}")
        if cache.num_layers != len(self.layers):
            raise ValueError("cache was built for a different number of layers")
        start = cache.length
        if n < 1:
            raise ValueError("forward_cached needs at least one token")
        if start > 0 and n > 1 and not chunk:
            raise NotImplementedError("chunked prefill (n > 1 on a non-empty cache) is not supported")
        if start + n > min(cache.max_len, self.context_length):
            raise ValueError(f"{start} cached + {n} new tokens exceed the cache (max_len {cache.max_len}, "
                             f"context_length {self.context_length})")
        if getattr(cache, "block_table", None) is not None:
            if chunk:
                raise NotImplementedError("forward_cached(chunk=True) is not supported on a PagedKVCache")
            cache.reserve(n)
        return self._forward_cached(x, cache, start)

    def _forward_cached(self, x: torch.Tensor, cache, start: int, max_kv_len: int | None = None) -> torch.Tensor:
        """The body of :meth:`forward_cached` after its checks: the prefill (``start == 0``) or one
        decode / chunk step (``start > 0``) over the layers, the cache advanced by the tokens of ``x``.
        ``max_kv_len``: see ``CausalMultiHeadSelfAttention.forward_cached``. Nothing here reads the
        host mirror ``cache.length`` or synchronizes the host, so a decode step can be captured into
        a HIP graph (``models/decode_graph.py``)."""
        n = x.shape[1]
        pos = kv_len = None
        if start > 0:  # once per step, shared by all layers
            pos = cache.lengths
            kv_len = cache.lengths + n
        ks, vs = getattr(cache, "k_scale", None), getattr(cache, "v_scale", None)

        table = getattr(cache, "block_table", None)  # a PagedKVCache: cache.k[i] is the layer's page pool

        def scales(i):  # the layer's scale views of an FP8 cache (and the table of a paged one)
            return (None, None, table) if ks is None else (ks[i], vs[i], table)
        with annotate("embed"):
            h = self.token_embeddings(x)
        n_layers = len(self.layers)
        if n_layers and self._fused_residual_ok(h):
            y = self.layers[0].ln1(h)
            for i, layer in enumerate(self.layers):
                with annotate(f"layer{i}"):
                    a = layer.attn.forward_cached(y, cache.k[i], cache.v[i], start, pos, kv_len, max_kv_len,
                                                  *scales(i))
                    self._reading(layer.ln2)
                    h, y = ops.add_rmsnorm(h, a, layer.ln2.weight, layer.ln2.eps)
                    f = layer.ffn(y)
                    nxt = self.layers[i + 1].ln1 if i + 1 < n_layers else self.ln_final
                    self._reading(nxt)
                    h, y = ops.add_rmsnorm(h, f, nxt.weight, nxt.eps)
        else:
            for i, layer in enumerate(self.layers):
                with annotate(f"layer{i}"):
                    h = h + layer.attn.forward_cached(layer.ln1(h), cache.k[i], cache.v[i], start, pos, kv_len,
                                                      max_kv_len, *scales(i))
                    h = h + layer.ffn(layer.ln2(h))
            y = self.ln_final(h)
        cache.advance(n)
        with annotate("lm_head"):
            return self.lm_head(y)

    @torch.no_grad()
    def generate(
        self,
        x: torch.Tensor,
        max_new_tokens: int,
        temperature: float = 1.0,
        top_k: int | None = None,
        eos_token_id: int | None = None,
        use_cache: bool = False,
        graph=False,
        draft=None,
        draft_tokens: int = 4,
        weights=None,
        kv_fp8: bool = False,
        sample_on_device: bool = False,
        generator=None,
        sync_every: int = 16,
        paged: bool = False,
        page_size: int = 64,
        share_prompt: bool = False,
    ) -> torch.Tensor:
        """Autoregressive sampling (``model.py:255-310``) with a working top-k filter (the
        reference's ``masked_fill`` is not in place and its threshold broadcast is wrong for B>1).

        ``use_cache=True``: prefill a KV cache on the prompt (its last ``context_length`` tokens),
        then one :meth:`forward_cached` step per token while the sequence fits the window; once the
        window is full the remaining tokens take the uncached sliding-window step (a window that
        slides re-positions every key, which only a full recomputation defines).

        ``graph=True`` (GPU models, with ``use_cache=True``): after the prefill the cached step is
        captured into a HIP graph over the skinny-M GEMM kernel (:class:`DecodeGraph`) and every
        cached step is one replay. ``graph=<DecodeGraph>`` reuses a caller-owned graph of this model
        and batch size (its cache is reset and prefilled), which saves the capture per call.
        Sampling stays eager.

        ``weights=qw`` (an ``Fp8DecodeWeights`` or ``Mxfp4DecodeWeights`` of this model, with ``graph=True``):
        the graph is built with the quantized weight copy, so every replayed step streams 8-bit (4-bit) weights. The prefill is
        unchanged and reads the 16-bit weights, as do the sliding-window steps once the window is
        full. With ``graph=<DecodeGraph>`` the graph's own weights are used; ``weights=`` without a
        graph raises.

        ``kv_fp8=True`` (with ``use_cache=True``): the cache is an FP8 one (``KVCache(fp8=True)``: e4m3
        rows with per-row scales, about half the bytes), and with ``draft=`` the draft's cache too. With
        ``graph=<DecodeGraph>`` the graph's own cache is used, whatever its format.

        ``draft=<model>``: greedy speculative decoding (``models/speculative.py``): the draft proposes
        ``draft_tokens`` tokens per round and this model verifies them in one chunk step; the output
        is exactly the greedy one. Needs ``use_cache=True``, ``top_k == 1`` and a bool ``graph``;
        sampling from a draft is not supported.

        ``sample_on_device=True`` (with ``use_cache=True``): every token is sampled by the fused sampler
        (``ops.sample_logits``, the rule of ``ops/sample.py``) from ONE table ``u = torch.rand(max_new_tokens,
        B, generator=generator)`` drawn up front, token ``s`` from row ``u[s]`` whichever path computes its
        logits: the prefill, the cached steps (with ``graph=`` inside the graph, ``DecodeGraph(sampler=)``:
        the host issues one replay per token and reads nothing back) and the sliding-window tail. The
        tokens are a function of the weights, the prompt and the table, whatever the batch. With
        ``eos_token_id`` the host polls every ``sync_every`` tokens and stops once every row has ended. At
        B == 1 the result is cut before the first end token, as without this switch; at B > 1 a row that has
        ended keeps emitting ``eos_token_id`` and the result is rectangular, up to and including the column
        in which the last row ended. ``draft=`` raises: speculation stays greedy.

        ``paged=True`` (with ``use_cache=True``): the cache is a ``PagedKVCache`` of ``page_size``-row pages
        with ``max_len = context_length``, filled page by page as the sequences grow. ``share_prompt=True``
        (with it, or with a ``graph=<DecodeGraph>`` on a paged cache; every row of ``x`` the same prompt, else
        ``ValueError``): the prompt is prefilled once, through ``cache.row(0)``, and ``cache.fork(0)`` gives
        the other rows its pages, so B sampled continuations pay one prefill and store the prompt once.
        ``kv_fp8=True`` and ``draft=`` raise with ``paged=True``; with ``graph=<DecodeGraph>`` the graph's own
        cache is used, whatever its kind."""
        from .decode_graph import DecodeGraph

        if (paged or share_prompt) and not use_cache:
            raise ValueError("generate(paged=True / share_prompt=True) needs use_cache=True")
        if paged and kv_fp8:
            raise ValueError("generate(paged=True) does not take kv_fp8=True: there is no FP8 paged format")
        if paged and draft is not None:
            raise NotImplementedError("generate(paged=True) does not take draft=: a paged cache has no chunk step")
        if share_prompt and not paged and not isinstance(graph, DecodeGraph):
            raise ValueError("generate(share_prompt=True) needs paged=True (or a DecodeGraph on a paged cache)")
        if share_prompt and x.dim() == 2 and not bool((x == x[:1]).all()):
            raise ValueError("generate(share_prompt=True) needs every row of x to be the same prompt")

        if kv_fp8 and not use_cache:
            raise ValueError("generate(kv_fp8=True) needs use_cache=True")
        if sample_on_device:
            if draft is not None:
                raise ValueError("generate(sample_on_device=True) does not take draft=: speculation is greedy")
            if not use_cache:
                raise ValueError("generate(sample_on_device=True) needs use_cache=True")
            return self._generate_on_device(x, max_new_tokens, temperature, top_k, eos_token_id, graph, weights, kv_fp8,
                                            generator, sync_every, paged, page_size, share_prompt)
        if draft is not None:
            from .speculative import speculative_generate

            if not use_cache:
                raise ValueError("generate(draft=...) needs use_cache=True")
            if top_k != 1:
                raise ValueError("generate(draft=...) is greedy: it needs top_k == 1")
            if not isinstance(graph, bool):
                raise ValueError("generate(draft=...) takes graph=True or False")
            if weights is not None:
                raise ValueError("generate(draft=...) does not take weights=")
            return speculative_generate(self, draft, x, max_new_tokens, draft_tokens, eos_token_id, graph,
                                        kv_fp8=kv_fp8)[0]

        if x.dim() == 1:
            x = x.unsqueeze(0)
        orig = x.size(-1)
        cache = dg = None
        if weights is not None and (graph is False or graph is None):
            raise ValueError("generate(weights=...) needs graph=True or a DecodeGraph: only graph steps read FP8 weights")
        if graph is not False and graph is not None:
            if not use_cache:
                raise ValueError("generate(graph=...) needs use_cache=True")
            if isinstance(graph, DecodeGraph):
                if graph.model is not self:
                    raise ValueError("the DecodeGraph belongs to a different model")
                if graph.cache.batch != x.size(0):
                    raise ValueError(f"batch {x.size(0)} does not match the DecodeGraph's {graph.cache.batch}")
                dg = graph
            elif graph is not True:
                raise ValueError("graph must be a bool or a DecodeGraph")
            elif not self.lm_head.weight.is_cuda:
                raise ValueError("generate(graph=True) captures a HIP graph: the model must be on a GPU")
        if use_cache and max_new_tokens > 0:
            if dg is not None:
                cache = dg.cache
                cache.reset()
            else:
                cache = self._new_cache(x.size(0), kv_fp8, paged, page_size)
            if share_prompt and getattr(cache, "block_table", None) is None:
                raise ValueError("generate(share_prompt=True) needs a paged cache")
        for _ in range(max_new_tokens):
            ctx = x[:, -self.context_length :] if x.size(1) > self.context_length else x
            if cache is not None and cache.length == 0:
                logits = self._prefill(ctx, cache, share_prompt)
            elif cache is not None and cache.length + 1 == x.size(1) <= self.context_length:
                if graph is True and dg is None:
                    dg = DecodeGraph(self, cache, capture=True, weights=weights)
                logits = dg.step(x[:, -1:]) if dg is not None else self.forward_cached(x[:, -1:], cache)
            else:
                cache = None  # the window is full (and slides from here on): full recomputation
                logits = self.forward(ctx)
            logits = logits[:, -1].float() / temperature
            if top_k:
                vals, _ = torch.topk(logits, min(top_k, logits.size(-1)))
                logits = logits.masked_fill(logits < vals[:, -1:], float("-inf"))
            probs = softmax(logits, dim=-1)
            nxt = torch.multinomial(probs, 1)
            if eos_token_id is not None and x.size(0) == 1 and nxt.item() == eos_token_id:
                break
            x = torch.cat((x, nxt), dim=-1)
        return x[:, orig:]

    def _new_cache(self, batch: int, kv_fp8: bool, paged: bool, page_size: int):
        """The cache ``generate`` builds for itself: the compute dtype is autocast's if it is on."""
        from .kv_cache import KVCache, PagedKVCache

        w = self.lm_head.weight
        dev = w.device.type
        cdt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else w.dtype
        if paged:
            return PagedKVCache(self, batch, page_size=page_size, max_len=self.context_length, device=w.device, dtype=cdt)
        return KVCache(self, batch, device=w.device, dtype=cdt, fp8=kv_fp8)

    def _prefill(self, ctx, cache, share_prompt: bool) -> torch.Tensor:
        """The prompt's last-position logits (B, 1, vocab) (all positions without ``share_prompt``). With
        ``share_prompt`` (a paged cache, equal rows) row 0 alone is prefilled and forked to the others."""
        if not share_prompt:
            return self.forward_cached(ctx, cache)
        logits = self.forward_cached(ctx[:1], cache.row(0))
        cache.fork(0)
        return logits[:, -1:].expand(ctx.size(0), -1, -1).contiguous()

    def _generate_on_device(self, x, max_new_tokens, temperature, top_k, eos_token_id, graph, weights, kv_fp8,
                            generator, sync_every, paged=False, page_size=64, share_prompt=False) -> torch.Tensor:
        """``generate(sample_on_device=True)``: see there."""
        from .decode_graph import DecodeGraph, Sampler

        sampler = Sampler(temperature, top_k, eos_token_id)
        if int(sync_every) != sync_every or sync_every < 1:
            raise ValueError("generate(sync_every=...) needs an integer >= 1")
        if x.dim() == 1:
            x = x.unsqueeze(0)
        B, P = x.shape
        use_graph = graph is not False and graph is not None
        dg = None
        if weights is not None and not use_graph:
            raise ValueError("generate(weights=...) needs graph=True or a DecodeGraph: only graph steps read FP8 weights")
        if isinstance(graph, DecodeGraph):
            if graph.model is not self:
                raise ValueError("the DecodeGraph belongs to a different model")
            if graph.cache.batch != B:
                raise ValueError(f"batch {B} does not match the DecodeGraph's {graph.cache.batch}")
            if graph.sampler != sampler:
                raise ValueError("generate(sample_on_device=True, graph=<DecodeGraph>) needs a DecodeGraph built with "
                                 "sampler=Sampler(temperature, top_k, eos_token_id) of this call")
            dg = graph
        elif use_graph and graph is not True:
            raise ValueError("graph must be a bool or a DecodeGraph")
        elif use_graph and not self.lm_head.weight.is_cuda:
            raise ValueError("generate(graph=True) captures a HIP graph: the model must be on a GPU")
        if max_new_tokens <= 0:
            return x[:, P:]
        L = self.context_length
        u = torch.rand(max_new_tokens, B, device=x.device, generator=generator)
        if dg is not None:
            cache = dg.cache
            cache.reset()
        else:
            cache = self._new_cache(B, kv_fp8, paged, page_size)
        if share_prompt and getattr(cache, "block_table", None) is None:
            raise ValueError("generate(share_prompt=True) needs a paged cache")
        eos = eos_token_id

        def pick(logits, s, done):  # token s of every row, (B, 1); a row that has ended stays at eos
            t = ops.sample_logits(logits[:, -1], u[s], temperature, top_k)
            if eos is not None:
                if done is not None:
                    t = torch.where(done, torch.full_like(t, eos), t)
                done = (t == eos) if done is None else done | (t == eos)
            return t[:, None], done

        # token 0: the prefill on the prompt's last context_length tokens
        logits = self._prefill(x[:, -L:] if P > L else x, cache, share_prompt)
        tok, done = pick(logits, 0, None)
        out = tok
        # cached steps while the sequence fits the window (and the cache)
        n_cached = min(max_new_tokens - 1, min(cache.max_len, L) - cache.length) if P <= L else 0
        finished = False
        if n_cached > 0 and use_graph:
            if dg is None:
                dg = DecodeGraph(self, cache, capture=True, weights=weights, sampler=sampler)
            dg.begin(tok, 1 + n_cached, table=u[:1 + n_cached])
            while dg._step < 1 + n_cached and not finished:
                dg.advance(min(sync_every, 1 + n_cached - dg._step))
                finished = dg.all_done()
            out = dg.tokens()
            done = dg.done != 0 if eos is not None else None
        elif n_cached > 0:
            toks = [tok]
            for s in range(1, 1 + n_cached):
                tok, done = pick(self.forward_cached(tok, cache), s, done)
                toks.append(tok)
                if eos is not None and s % sync_every == 0 and bool(done.all().item()):
                    finished = True
                    break
            out = torch.cat(toks, dim=-1)
        # the window is full (and slides from here on): full recomputation
        if out.size(1) < max_new_tokens and not finished:
            seq = torch.cat((x, out), dim=-1)
            for s in range(out.size(1), max_new_tokens):
                tok, done = pick(self.forward(seq[:, -L:] if seq.size(1) > L else seq), s, done)
                seq = torch.cat((seq, tok), dim=-1)
                if eos is not None and s % sync_every == 0 and bool(done.all().item()):
                    break
            out = seq[:, P:]
        if eos is None:
            return out
        hit = out == eos
        ended = hit.any(dim=-1)
        first = torch.where(ended, hit.to(torch.int8).argmax(dim=-1), out.size(1))  # the first eos of each row
        if B == 1:
            return out[:, :int(first[0])]
        return out[:, :int(first.max()) + 1] if bool(ended.all()) else out

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, map_location=None):
        with open(os.path.join(pretrained_model_path, "model_config.json")) as f:
            config = json.load(f)
        model = cls(**config)
        state_dict = torch.load(os.path.join(pretrained_model_path, "model.pt"), map_location=map_location, weights_only=True)
        prefix = "_orig_mod."
        for k in list(state_dict.keys()):
            if k.startswith(prefix):
                state_dict[k[len(prefix) :]] = state_dict.pop(k)
        model.load_state_dict(state_dict)
        return model

    def save_pretrained(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "model_config.json"), "w") as f:
            json.dump(self.config, f, indent=2)
        torch.save(self.state_dict(), os.path.join(path, "model.pt"))
