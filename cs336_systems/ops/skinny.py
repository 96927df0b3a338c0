"""Linear layers with at most 16 input rows: the M = batch projections of a decode step.

``skinny_linear(x, w)`` is ``x @ w.T`` for ``x`` (..., K) and a weight ``w`` (N, K). On a GPU, 16-bit
operands with at most 16 rows in total, K % 8 == 0 and 16-B aligned rows run the weight-streaming
HIP kernel (``csrc/gemm/gemm_skinny.hip``: W read once, straight to registers, MFMA dot products,
bitwise reproducible); anything else -- fp32, more rows, odd K, misaligned views -- runs the existing
projection path ``gemm.mm_nt``. On the CPU ``F.linear`` is the only path. On a GPU with the HIP
backend a missing extension raises.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import gemm
from ._ext import use_hip


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
