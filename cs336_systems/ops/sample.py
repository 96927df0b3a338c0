"""Temperature / top-k sampling of one token per row of logits, eager reference + HIP kernel
(``csrc/ops/sample.hip``): what ``generate`` does with ``topk`` / ``masked_fill`` / ``softmax`` /
``multinomial``, as one launch whose random number is an INPUT.

The rule, shared by the kernel, the reference and the tests. One row of logits ``x[0..V)`` (bf16, fp16
or fp32, read as fp32), one uniform ``u`` in ``[0, 1)``, ``temperature > 0`` and ``top_k`` (``None``, 0
or ``>= V``: no filter) give one token:

* kept set: with a filter ``keep_i = x_i >= (k-th largest value of the row)`` on the raw logits, so
  ties at the threshold are all kept (what ``masked_fill(logits < kth)`` does) and ``-0.0 == +0.0``;
  ``-inf`` entries have probability 0;
* weights: ``w_i = exp((x_i - max) / temperature)`` for kept ``i`` in fp32, ``S = sum w_i``;
* choice, the inverse CDF in index order: the smallest kept ``i`` whose inclusive prefix sum exceeds
  ``u * S``; if rounding leaves none, the last kept ``i`` with ``w_i > 0``. ``top_k = 1`` is argmax, exact
  ties split by ``u``;
* the same inputs give the same token bit for bit (fixed summation order, no float atomics);
* a row with NaN, or with only ``-inf``, returns some index in ``[0, V)`` and nothing else is promised.

The kernel and the reference add the fp32 weights in different (each fixed) orders, so on a few rows
in a thousand, where ``u * S`` falls within rounding of a prefix sum, they pick neighbouring tokens;
both are within ``1e-5`` of the fp64 CDF (``tests/test_sample_gpu.py``).

There is no RNG here: draw ``u`` with ``torch.rand`` (one ``(steps, B)`` table per generation, row ``s``
for token ``s``), and the output is a pure function of the logits and a table the caller can reproduce.

``sample_advance`` is the sampler inside a decode loop that never returns to the host
(``models/decode_graph.py``): with ``s = step[0]`` and ``u = u_table[s, b]`` it samples row ``b``
(``eos_id`` instead where ``done[b]``), writes ``tok[b]`` and ``out[b, s]`` and sets ``done[b]`` once the
token is ``eos_id`` (``eos_id < 0``: never). ``s`` outside ``[0, S)`` stores nothing at all, the rule of
the append kernels for a slot outside the cache. ``step`` is only read: the loop adds 1 itself.

On a GPU with the HIP backend a missing extension raises.
"""

from __future__ import annotations

import torch

from ._ext import ops, use_hip

_FLOATS = (torch.bfloat16, torch.float16, torch.float32)
_MAX_V = 1 << 30  # the kernel's 32-bit indices


def _check(logits, u, table, temperature, top_k, what):
    """The argument errors of both ops; returns top_k as the kernel takes it (0 = no filter)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"{what} takes logits (B, V) with V >= 1")
    if not logits.is_floating_point():
        raise ValueError(f"{what} takes floating-point logits, not {logits.dtype}")
    if not temperature > 0:
        raise ValueError(f"{what} needs temperature > 0 (got {temperature})")
    k = 0 if top_k is None else int(top_k)
    if k < 0 or (top_k is not None and k != top_k):
        raise ValueError(f"{what} needs top_k None or an integer >= 0 (got {top_k})")
    B = logits.shape[0]
    if (not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or u.dim() != (2 if table else 1)
            or u.shape[-1] != B):
        raise ValueError(f"{what} takes fp32 u of shape {'(S, B)' if table else '(B,)'} with B = {B}")
    return 0 if k >= logits.shape[1] else k


def sample_logits_ref(logits, u, temperature=1.0, top_k=None, dtype=torch.float32):
    """The rule in eager torch, in ``dtype`` math (fp32; the tests also run it in fp64). No host sync."""
    x = logits.to(dtype)
    V = x.shape[-1]
    k = 0 if top_k is None or top_k >= V else int(top_k)
    if k:
        keep = x >= torch.topk(x, k, dim=-1).values[:, -1:]
    else:
        keep = torch.ones_like(x, dtype=torch.bool)
    m = x.amax(dim=-1, keepdim=True)
    t = torch.full((), float(temperature), dtype=dtype, device=x.device)  # (a tensor divisor: see ops/decode.py)
    w = torch.where(keep, torch.exp((x - m) / t), torch.zeros_like(x))
    c = torch.cumsum(w, dim=-1)
    pos = w > 0
    hit = (c > u.to(dtype)[:, None] * c[:, -1:]) & pos
    first = hit.to(torch.int8).argmax(dim=-1)  # the first maximum: the smallest index that hits
    last = V - 1 - pos.flip(-1).to(torch.int8).argmax(dim=-1)
    return torch.where(hit.any(dim=-1), first, last)


def sample_logits(logits, u, temperature: float = 1.0, top_k: int | None = None) -> torch.Tensor:
    """``logits`` (B, V) bf16 / fp16 / fp32 with a contiguous last dim and any row stride (the
    ``logits[:, -1]`` of a (B, n, V) tensor is passed as is), ``u`` (B,) fp32 in [0, 1) -> tokens (B,)
    int64. Nothing synchronizes the host."""
    k = _check(logits, u, False, temperature, top_k, "sample_logits")
    if use_hip(logits, u) and logits.dtype in _FLOATS and logits.shape[1] <= _MAX_V:
        if logits.stride(-1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < 0):
            logits = logits.contiguous()
        return ops().sample_logits(logits, u.contiguous(), float(temperature), k)
    return sample_logits_ref(logits, u, temperature, k)


def sample_advance_ref(logits, u_table, step, temperature, top_k, eos_id, tok, out, done) -> None:
    """:func:`sample_advance` in eager torch; no host sync either (every store is a ``where``)."""
    B = logits.shape[0]
    S = u_table.shape[0]
    s = step.reshape(()).to(torch.int64)
    ok = (s >= 0) & (s < S)
    sc = s.clamp(0, max(S - 1, 0))
    if S == 0:
        return
    t = sample_logits_ref(logits, u_table.index_select(0, sc.reshape(1))[0], temperature, top_k)
    fin = done != 0
    t = torch.where(fin, torch.full_like(t, int(eos_id)), t)
    if eos_id >= 0:
        fin = fin | (t == eos_id)
    col = sc.reshape(1, 1).expand(B, 1)
    tok.copy_(torch.where(ok, t, tok.reshape(B)).reshape(tok.shape))
    out.scatter_(1, col, torch.where(ok, t, out.gather(1, col)[:, 0])[:, None])
    done.copy_(torch.where(ok, fin.to(done.dtype), done))


def sample_advance(logits, u_table, step, temperature, top_k, eos_id, tok, out, done) -> None:
    """``logits`` (B, V), ``u_table`` (S, B) fp32, ``step`` int32 with one element, ``tok`` (B, 1) int64,
    ``out`` (B, S) int64, ``done`` (B,) int32, all on the logits' device; ``eos_id`` an int (< 0: none).
    In place on ``tok``, ``out`` and ``done``; see the module docstring."""
    k = _check(logits, u_table, True, temperature, top_k, "sample_advance")
    B, S = logits.shape[0], u_table.shape[0]
    if (step.dtype != torch.int32 or step.numel() != 1 or tok.dtype != torch.int64 or tuple(tok.shape) != (B, 1)
            or out.dtype != torch.int64 or tuple(out.shape) != (B, S) or done.dtype != torch.int32
            or tuple(done.shape) != (B,)):
        raise ValueError("sample_advance takes step int32[1], tok (B, 1) int64, out (B, S) int64 and done (B,) int32")
    eos_id = -1 if eos_id is None else int(eos_id)
    if (use_hip(logits, u_table) and logits.dtype in _FLOATS and logits.shape[1] <= _MAX_V and u_table.is_contiguous()
            and tok.is_contiguous() and out.is_contiguous() and done.is_contiguous()):
        if logits.stride(-1) != 1 or (B > 1 and logits.stride(0) < 0):
            logits = logits.contiguous()
        ops().sample_advance(logits, u_table, step, float(temperature), k, eos_id, tok, out, done)
        return
    sample_advance_ref(logits, u_table, step, temperature, k, eos_id, tok, out, done)
