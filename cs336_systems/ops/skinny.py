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

MXFP4 weights (weight-only, W4A16). ``quantize_mxfp4_rows(w)`` gives ``(wq, scale)`` in the OCP
microscaling format: ``wq`` (N, K/2) uint8 with two e2m1 codes per byte (k = 2j in bits 3:0, k = 2j+1 in
bits 7:4: the packing of ``torch.float4_e2m1fn_x2``) and ``scale`` (N, K/32) uint8, one e8m0 power of
two per 32 values; the dequantized weight is ``val(code[n, k]) * 2^(scale[n, k // 32] - 127)``
(``dequantize_mxfp4_rows``). ``skinny_linear_mxfp4(x, wq, scale)`` is ``x @ dq.T``: on a GPU, at most 16
rows run ``csrc/gemm/gemm_skinny_w4.hip``, which streams 17/32 of a byte per weight and converts W in
registers with the block scale as the conversion's operand (exactly, for the scales the quantizer
emits).
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


# ---- OCP MXFP4: e2m1 codes with one e8m0 scale per 32 values ----
MXFP4_BLOCK = 32
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # val(code & 7); bit 3 of a code is the sign
MXFP4_MIN_EXP, MXFP4_MAX_EXP = -23, 13  # the scale exponents emitted: code * 2^X is exact in bf16 and fp16


def _as_u8(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _pow2_f32(byte: torch.Tensor) -> torch.Tensor:
    """``2^(byte - 127)`` as fp32 from e8m0 bytes, built from the bits (``pow`` / ``ldexp`` are not exact on
    every device): byte 0 is the subnormal 2^-127 and 255 the format's NaN."""
    b = byte.to(torch.int32)
    bits = torch.where(b == 0, torch.full_like(b, 0x00400000), b << 23)
    return torch.where(b == 255, torch.full_like(b, 0x7FC00000), bits).view(torch.float32)


def _mxfp4_check(wq: torch.Tensor, scale: torch.Tensor) -> None:
    if wq.dim() != 2 or scale.dim() != 2 or wq.element_size() != 1 or scale.element_size() != 1:
        raise ValueError("MXFP4 takes wq (N, K/2) and scale (N, K/32) of one-byte elements")
    if wq.dtype not in (torch.uint8, torch.float4_e2m1fn_x2) or scale.dtype not in (torch.uint8, torch.float8_e8m0fnu):
        raise ValueError("MXFP4 takes wq as uint8 / float4_e2m1fn_x2 and scale as uint8 / float8_e8m0fnu")
    if wq.shape[1] % (MXFP4_BLOCK // 2) or tuple(scale.shape) != (wq.shape[0], wq.shape[1] // (MXFP4_BLOCK // 2)):
        raise ValueError("MXFP4 takes wq (N, K/2) and scale (N, K/32) with K % 32 == 0")


@torch.no_grad()
def quantize_mxfp4_rows_(w: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> None:
    """:func:`quantize_mxfp4_rows` into existing ``wq`` (N, K/2) and ``scale`` (N, K/32), uint8 or their
    ``float4_e2m1fn_x2`` / ``float8_e8m0fnu`` views (views of larger tensors are fine); neither is
    re-allocated."""
    if w.dim() != 2 or not w.is_floating_point():
        raise ValueError("quantize_mxfp4_rows takes a 2-D float weight (N, K)")
    n, k = w.shape
    if k % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4_rows needs K % {MXFP4_BLOCK} == 0 (got {k})")
    _mxfp4_check(wq, scale)
    if tuple(wq.shape) != (n, k // 2):
        raise ValueError("wq must be (N, K/2) and scale (N, K/32) for w (N, K)")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_mxfp4_rows: the weight holds inf or NaN")
    blocks = wf.view(n, k // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blocks.abs().amax(dim=2)
    # amax = m * 2^e with m in [0.5, 1): floor(log2(amax)) is e - 1, from the exponent field, exactly
    e = torch.frexp(amax)[1]
    x = torch.where(amax > 0, e - 3, torch.zeros_like(e)).clamp_(MXFP4_MIN_EXP, MXFP4_MAX_EXP)
    a = (blocks * _pow2_f32(127 - x)[:, :, None]).abs_()  # a power-of-two division: exact
    # nearest grid value, ties to the even code: a midpoint above an even code stays, above an odd one goes
    # up; anything above 5 is 6 (saturation)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code |= torch.signbit(blocks).to(torch.uint8) << 3
    code = code.view(n, k // 2, 2)
    _as_u8(wq).copy_(code[:, :, 0] | (code[:, :, 1] << 4))
    _as_u8(scale).copy_((x + 127).to(torch.uint8))


def quantize_mxfp4_rows(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """OCP MXFP4 quantization of a 2-D weight ``w`` (N, K) of any float dtype, K % 32 == 0: ``wq`` (N, K/2)
    uint8, byte ``j`` of a row holding the code of ``k = 2j`` in bits 3:0 and of ``k = 2j+1`` in bits 7:4, a
    code being ``sign << 3 | m`` with ``m`` indexing {0, .5, 1, 1.5, 2, 3, 4, 6}; ``scale`` (N, K/32) uint8,
    e8m0: block ``b`` of row ``n`` is multiplied by ``2^(scale[n, b] - 127)``.

    Per 32-value block (the OCP rule): ``X = floor(log2(amax)) - 2`` from the fp32 exponent, clamped to
    [-23, 13]; the elements ``v / 2^X`` (exact) are rounded to the nearest grid value, ties to the even
    code, and saturate at +-6; the sign bit is the input's, also where the value rounds to zero. An
    all-zero block gets byte 127 and zero codes. Inside the clamp every ``code * 2^X`` is exact in bf16 and
    in fp16; a block outside it saturates or flushes. inf or NaN input raises ValueError."""
    if w.dim() != 2:
        raise ValueError("quantize_mxfp4_rows takes a 2-D float weight (N, K)")
    if w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4_rows needs K % {MXFP4_BLOCK} == 0 (got {w.shape[1]})")
    wq = torch.empty(w.shape[0], w.shape[1] // 2, dtype=torch.uint8, device=w.device)
    scale = torch.empty(w.shape[0], w.shape[1] // MXFP4_BLOCK, dtype=torch.uint8, device=w.device)
    quantize_mxfp4_rows_(w, wq, scale)
    return wq, scale


def dequantize_mxfp4_rows(wq: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``val(code[n, k]) * 2^(scale[n, k // 32] - 127)`` as (N, K) ``dtype``: the table lookup that inverts
    :func:`quantize_mxfp4_rows` (computed in fp32, fp64 for ``dtype`` fp64, then cast: exact for what the
    quantizer emits)."""
    _mxfp4_check(wq, scale)
    cdt = torch.float64 if dtype == torch.float64 else torch.float32
    b, sb = _as_u8(wq), _as_u8(scale)
    n, k = b.shape[0], 2 * b.shape[1]
    codes = torch.stack((b & 0xF, b >> 4), dim=2).view(n, k).long()
    table = torch.tensor(MXFP4_VALUES + tuple(-v for v in MXFP4_VALUES), dtype=cdt, device=b.device)
    mul = _pow2_f32(sb).to(cdt).repeat_interleave(MXFP4_BLOCK, dim=1)
    return (table[codes] * mul).to(dtype)  # times a power of two: exact


def skinny_linear_mxfp4_ref(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``(x.float() @ dequantize_mxfp4_rows(wq, scale).T).to(x.dtype)``: fp32 of the dequantized operands
    with one rounding; an fp32 / fp64 ``x`` computes in its own dtype."""
    cdt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    return (x.to(cdt) @ dequantize_mxfp4_rows(wq, scale, cdt).T).to(x.dtype)


def skinny_linear_mxfp4(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``x @ dq.T`` for ``x`` (..., K) in bf16 / fp16 and the MXFP4 weight ``wq`` (N, K/2), ``scale``
    (N, K/32) (:func:`quantize_mxfp4_rows`; their ``float4_e2m1fn_x2`` / ``float8_e8m0fnu`` views are
    accepted).

    On a GPU with the HIP backend, at most 16 rows in total that ``gemm.skinny_w4_ok`` takes (16-B
    aligned rows) run the MXFP4 weight-streaming kernel: fp32 accumulation, one rounding. More than 16
    rows run the existing GEMM on the dequantized weight in ``x``'s dtype (an exact conversion) with an
    fp32 result, rounded once. Anything else on the GPU, and the CPU, runs
    :func:`skinny_linear_mxfp4_ref`. A missing extension on a HIP-backend GPU raises."""
    if not use_hip(x, wq):
        return skinny_linear_mxfp4_ref(x, wq, scale)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[0] <= gemm.SKINNY_MAX_M and gemm.skinny_w4_ok(x2, wq, scale):
        y = gemm.skinny_w4_mm(x2, wq, scale)
    elif x2.shape[0] > gemm.SKINNY_MAX_M and x2.dtype in (torch.bfloat16, torch.float16):
        y = _mm_nt_fp32(x2, dequantize_mxfp4_rows(wq, scale, x2.dtype)).to(x2.dtype)
    else:
        y = skinny_linear_mxfp4_ref(x2, wq, scale)
    return y.view(*x.shape[:-1], wq.shape[0])
