"""Linear layers with at most 16 input rows: the M = batch projections of a decode step.

``skinny_linear(x, w)`` is ``x @ w.T`` for ``x`` (..., K) and a weight ``w`` (N, K). On a GPU, 16-bit
operands with at most 16 rows in total, K % 8 == 0 and 16-B aligned rows run the weight-streaming
HIP kernel (``csrc/gemm/gemm_skinny.hip``: W read once, straight to registers, MFMA dot products,
bitwise reproducible); anything else -- fp32, more rows, odd K, misaligned views -- runs the existing
projection path ``gemm.mm_nt``. On the CPU ``F.linear`` is the only path. On a GPU with the HIP
backend a missing extension raises.

FP8 weights (weight-only, W8A16). ``quantize_fp8_rows(w)`` gives ``(wq, scale)``: OCP e4m3 bytes
(``torch.float8_e4m3fn``) with one fp32 scale per output row, the dequantized weight being
``wq[n, k] * scale[n]``. ``skinny_linear_fp8(x, wq, scale)`` is ``(x @ wq.T) * scale`` with the
activations left in 16 bits: on a GPU, at most 16 rows run the e4m3 format of
``csrc/gemm/gemm_skinny.hip``, which streams half the bytes of the 16-bit format, converts W in registers (exactly) and applies the scale
to the fp32 sum before its one rounding.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import gemm
from ._ext import use_hip

FP8_MAX = 448.0  # largest finite e4m3 value


def skinny_linear_ref(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return F.linear(x, w)


def skinny_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if not use_hip(x, w):
        return skinny_linear_ref(x, w)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[0] <= gemm.SKINNY_MAX_M and gemm.skinny_ok(x2, w):
        y = gemm.skinny_mm(x2, w)
    else:
        y = gemm.mm_nt(x2, w)
    return y.view(*x.shape[:-1], w.shape[0])


@torch.no_grad()
def quantize_fp8_rows_(w: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> None:
    """:func:`quantize_fp8_rows` into existing ``wq`` (N, K) float8_e4m3fn and ``scale`` (N,) fp32
    (views are fine); neither is re-allocated."""
    if w.dim() != 2:
        raise ValueError("quantize_fp8_rows takes a 2-D weight (N, K)")
    if wq.dtype != torch.float8_e4m3fn or tuple(wq.shape) != tuple(w.shape):
        raise ValueError("wq must be float8_e4m3fn of w's shape")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (w.shape[0],):
        raise ValueError("scale must be fp32 with one element per row of w")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_fp8_rows: the weight holds inf or NaN")
    amax = wf.abs().amax(dim=1) if w.shape[1] else wf.new_zeros(w.shape[0])
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    scale.copy_(s)
    # clamped before the round-to-nearest-even cast: a quotient a hair above 448 would otherwise
    # become the NaN byte (e4m3fn has no inf and saturates to NaN)
    wq.copy_((wf / s[:, None]).clamp_(-FP8_MAX, FP8_MAX))


def quantize_fp8_rows(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row symmetric FP8 quantization of a 2-D weight ``w`` (N, K) of any float dtype: ``wq``
    (N, K) ``torch.float8_e4m3fn``, contiguous, and ``scale`` (N,) fp32 with ``scale[n] =
    amax_k |w[n, k]| / 448`` computed in fp32, so that ``wq[n, k] * scale[n]`` is the dequantized
    weight and each row's largest element maps to +-448 exactly. An all-zero row gets scale 1 and
    zeros. No NaN byte (0x7f / 0xff) comes out of finite input; inf or NaN input raises ValueError."""
    if w.dim() != 2:
        raise ValueError("quantize_fp8_rows takes a 2-D weight (N, K)")
    wq = torch.empty(w.shape, dtype=torch.float8_e4m3fn, device=w.device)
    scale = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
    quantize_fp8_rows_(w, wq, scale)
    return wq, scale


def _as_fp8(wq: torch.Tensor) -> torch.Tensor:
    return wq.view(torch.float8_e4m3fn) if wq.dtype == torch.uint8 else wq


def skinny_linear_fp8_ref(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``((x.float() @ wq.float().T) * scale).to(x.dtype)``; an fp32 / fp64 ``x`` computes in its own
    dtype."""
    wq = _as_fp8(wq)
    cdt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    return ((x.to(cdt) @ wq.to(cdt).T) * scale.to(cdt)).to(x.dtype)


def _mm_nt_fp32(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``x @ w.T`` of 16-bit operands with an fp32 result."""
    try:
        return torch.mm(x, w.t(), out_dtype=torch.float32)
    except (TypeError, RuntimeError):
        return gemm.mm_nt(x, w).float()


def skinny_linear_fp8(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``(x @ wq.T) * scale`` for ``x`` (..., K) in bf16 / fp16, ``wq`` (N, K) e4m3 (or its uint8
    view) and ``scale`` (N,) fp32 (:func:`quantize_fp8_rows`).

    On a GPU with the HIP backend, at most 16 rows in total that ``gemm.skinny_w8_ok`` takes (K % 16
    == 0, 16-B aligned rows) run the FP8 weight-streaming kernel: fp32 accumulation, the scale applied
    to the fp32 sum, one rounding. More than 16 rows run the existing GEMM (hipBLASLt) on
    ``wq.to(x.dtype)``, an exact conversion, with an fp32 result, then the scale in fp32 and one
    rounding. Through ``gemm.mm_nt``'s 16-bit output that path would round twice, once to the GEMM
    output and once after the scale, and be off by up to a whole ulp of the output, which the tests'
    one-rounding rule does not pass; it is what runs only where ``torch.mm`` has no fp32 output.
    Anything else on the GPU, and the CPU, runs :func:`skinny_linear_fp8_ref`. A missing extension
    on a HIP-backend GPU raises."""
    wq = _as_fp8(wq)
    if not use_hip(x, wq):
        return skinny_linear_fp8_ref(x, wq, scale)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[0] <= gemm.SKINNY_MAX_M and gemm.skinny_w8_ok(x2, wq, scale):
        y = gemm.skinny_w8_mm(x2, wq, scale)
    elif x2.shape[0] > gemm.SKINNY_MAX_M and x2.dtype in (torch.bfloat16, torch.float16):
        y = (_mm_nt_fp32(x2, wq.to(x2.dtype)) * scale).to(x2.dtype)
    else:
        y = skinny_linear_fp8_ref(x2, wq, scale)
    return y.view(*x.shape[:-1], wq.shape[0])
