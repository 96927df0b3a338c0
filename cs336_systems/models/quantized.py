"""FP8 and MXFP4 weight-only copies of a model's projection matrices for the decode step.

A replayed decode token streams every projection matrix from HBM once; on the large matrices its
time is the weight bytes. ``Fp8DecodeWeights(model)`` keeps a second copy of those matrices as OCP
e4m3 bytes with one fp32 scale per output row (``ops.quantize_fp8_rows``), in the layout the decode
step multiplies by: per layer the grouped QKV tensor, the attention output, the grouped W1|W3 and W2,
and the vocabulary head. Embeddings and norm weights stay as they are. The activations stay 16-bit
(W8A16): ``ops.skinny_linear_fp8`` converts W in registers and scales the fp32 sums.

The copy is used only where it is asked for: ``DecodeGraph(model, cache, weights=qw)`` (and
``generate(..., graph=True, weights=qw)``) runs its step inside ``gemm.skinny_decode(fp8=qw)``, in
which a projection whose 16-bit weight is in ``qw``'s table reads the FP8 copy. The prefill and
every other forward keep reading the 16-bit weights, and both copies stay alive: this trades memory
for decode speed, it does not save memory.

``Mxfp4DecodeWeights(model)`` is the same object in the OCP MXFP4 format (``ops.quantize_mxfp4_rows``: two
e2m1 codes per byte and one e8m0 power-of-two scale per 32 values, 17/32 of a byte per weight), read by
``ops.skinny_linear_mxfp4``. The two classes share everything but the format: ``_DecodeWeights`` holds the
tables, and a format supplies its buffers, quantizer, dequantizer and linear. ``gemm.skinny_decode`` and
the model's layers call ``qw.linear``, so the weights object says which kernel runs.
"""

from __future__ import annotations

import torch

from . import fused
from ..ops import skinny


class _DecodeWeights:
    """What the quantized copies share: ``qw = Fp8DecodeWeights(model)`` / ``Mxfp4DecodeWeights(model)`` for
    a ``BasicsTransformerLM`` held in bf16 or fp16. A format defines ``K_UNIT`` and ``WHY`` (K must be a
    multiple of the kernel's W load), ``_alloc``, ``_quantize_``, ``_dequantize`` and ``linear``.

    ``qw.lookup(w)`` maps the 16-bit operand tensor a projection hands to ``gemm.mm_nt`` -- the grouped
    QKV / W1|W3 view, or a single parameter -- to its ``(wq, scale)``. The table is keyed on address and
    shape and every entry holds the 16-bit tensor, so its storage, and with it the address, cannot be
    reused while ``qw`` lives. Re-allocating the parameters (``model.to(...)``) orphans the table: the
    lookups then miss and the step reads the 16-bit weights; build a new object.

    ``qw.refresh()`` requantizes in place from the current weights (after an in-place weight update);
    nothing is re-allocated, so a captured graph stays valid. ``qw.nbytes`` is the size of the
    quantized copy (bytes and scales)."""

    def __init__(self, model):
        if getattr(model, "tensor_parallel", None) is not None or any(
                layer.attn.context_parallel is not None for layer in model.layers):
            raise NotImplementedError(f"{type(self).__name__} does not support tensor / context parallelism")
        self.model = model
        self._groups: list[tuple[list[torch.Tensor], torch.Tensor, torch.Tensor]] = []
        self._table: dict[tuple, tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        for i, layer in enumerate(model.layers):
            at, ff = layer.attn, layer.ffn
            self._add(f"layers.{i}.attn.qkv", [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight])
            self._add(f"layers.{i}.attn.output_proj", [at.output_proj.weight])
            self._add(f"layers.{i}.ffn.w1|w3", [ff.w1.weight, ff.w3.weight])
            self._add(f"layers.{i}.ffn.w2", [ff.w2.weight])
        self._add("lm_head", [model.lm_head.weight])
        self.refresh()

    def _add(self, name: str, params: list[torch.Tensor]) -> None:
        p0 = params[0]
        for p in params:
            if p.dtype not in (torch.bfloat16, torch.float16):
                raise ValueError(f"{type(self).__name__} needs the model held in bf16 or fp16: {name} is {p.dtype}")
            if p.dim() != 2 or p.shape[1] != p0.shape[1] or p.dtype != p0.dtype or p.device != p0.device:
                raise ValueError(f"{name}: the matrices of a group must share width, dtype and device")
        k = p0.shape[1]
        if k < self.K_UNIT or k % self.K_UNIT:
            raise ValueError(f"{name}: K = {k} is not a multiple of {self.K_UNIT} ({self.WHY})")
        rows = sum(p.shape[0] for p in params)
        wq, scale = self._alloc(rows, k, p0.device)
        held = [p.detach() for p in params]
        self._groups.append((held, wq, scale))
        # each matrix on its own (the ungrouped and the CPU paths multiply by them one at a time) ...
        off = 0
        for t in held:
            n = t.shape[0]
            self._table[self._key(t)] = (t, wq[off:off + n], scale[off:off + n])
            off += n
        # ... and the row-adjacent group as the one operand the grouped GEMM gets
        g = fused.grouped_view(held) if len(held) > 1 else None
        if g is not None:
            self._table[self._key(g)] = (g, wq, scale)

    @staticmethod
    def _key(t: torch.Tensor) -> tuple:
        return (t.data_ptr(), tuple(t.shape))

    def lookup(self, w: torch.Tensor):
        """``(wq, scale)`` of the 16-bit weight ``w``, or None when it is not one of this model's."""
        e = self._table.get((w.data_ptr(), tuple(w.shape)))
        if e is None or e[0].dtype != w.dtype or e[0].stride() != w.stride() or e[0].device != w.device:
            return None
        return e[1], e[2]

    @torch.no_grad()
    def refresh(self):
        for held, wq, scale in self._groups:
            off = 0
            for t in held:
                n = t.shape[0]
                self._quantize_(t, wq[off:off + n], scale[off:off + n])
                off += n
        return self

    @property
    def nbytes(self) -> int:
        return sum(wq.numel() * wq.element_size() + scale.numel() * scale.element_size()
                   for _, wq, scale in self._groups)

    def dequantized_state_dict(self, dtype: torch.dtype = torch.float32) -> dict[str, torch.Tensor]:
        """The model's ``state_dict`` with every quantized matrix replaced by its dequantized copy in
        ``dtype`` (the other entries cast to it): the exact model a quantized step approximates."""
        sd = {k: v.detach().to(dtype) for k, v in self.model.state_dict().items()}
        names = {p.data_ptr(): k for k, p in self.model.named_parameters()}
        for held, wq, scale in self._groups:
            off = 0
            for t in held:
                n = t.shape[0]
                sd[names[t.data_ptr()]] = self._dequantize(wq[off:off + n], scale[off:off + n], dtype)
                off += n
        return sd


class Fp8DecodeWeights(_DecodeWeights):
    """OCP e4m3 bytes with one fp32 scale per output row (``ops.quantize_fp8_rows``): ``wq`` (N, K)
    ``float8_e4m3fn``, ``scale`` (N,); ``nbytes`` is elements + 4 bytes per row."""

    K_UNIT = 16
    WHY = "the FP8 kernel loads 16 k at a time"

    @staticmethod
    def _alloc(rows, k, device):
        return (torch.empty(rows, k, dtype=torch.float8_e4m3fn, device=device),
                torch.empty(rows, dtype=torch.float32, device=device))

    @staticmethod
    def _quantize_(w, wq, scale):
        skinny.quantize_fp8_rows_(w, wq, scale)

    @staticmethod
    def _dequantize(wq, scale, dtype):
        return wq.to(dtype) * scale.to(dtype)[:, None]

    @staticmethod
    def linear(x, wq, scale):
        return skinny.skinny_linear_fp8(x, wq, scale)


class Mxfp4DecodeWeights(_DecodeWeights):
    """OCP MXFP4 (``ops.quantize_mxfp4_rows``): ``wq`` (N, K/2) uint8 of two e2m1 codes, ``scale`` (N, K/32)
    uint8 e8m0; every K a multiple of 32; ``nbytes`` is elements x 17/32."""

    K_UNIT = 32
    WHY = "an MXFP4 block is 32 k"

    @staticmethod
    def _alloc(rows, k, device):
        return (torch.empty(rows, k // 2, dtype=torch.uint8, device=device),
                torch.empty(rows, k // 32, dtype=torch.uint8, device=device))

    @staticmethod
    def _quantize_(w, wq, scale):
        skinny.quantize_mxfp4_rows_(w, wq, scale)

    @staticmethod
    def _dequantize(wq, scale, dtype):
        return skinny.dequantize_mxfp4_rows(wq, scale, dtype)

    @staticmethod
    def linear(x, wq, scale):
        return skinny.skinny_linear_mxfp4(x, wq, scale)
