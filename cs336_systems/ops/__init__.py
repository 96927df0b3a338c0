"""Kernel layer: every hot op has an eager PyTorch reference (used on CPU and as the numerics
oracle in tests) and a hand-written HIP/CDNA4 kernel (used for GPU tensors)."""

from ._ext import backend, ext_available, get_backend, load_error, load_ext, set_backend, use_hip
from .adamw import FusedAdamW, clip_grad_norm_, multi_tensor_l2norm
from .cross_entropy import cross_entropy, cross_entropy_ref
from .decode import (decode_attention, decode_attention_chunk, decode_attention_chunk_ref, decode_attention_paged,
                     decode_attention_paged_ref, decode_attention_ref, kv_append_rope_paged, kv_append_rope_paged_ref,
                     paged_gather,
                     kv_append_rope, kv_append_rope_chunk, kv_append_rope_chunk_kv8_ref, kv_append_rope_chunk_ref,
                     kv_append_rope_kv8_ref, kv_append_rope_ref, kv_dequantize, kv_quantize_ref, kv_quantize_rows,
                     kv_quantize_rows_ref)
from .flash_attention import (
    FlashAttentionHIP,
    FlashAttentionTorch,
    FlashAttentionTriton,
    flash_attention,
    naive_attention,
)
from .rmsnorm import add_rmsnorm, add_rmsnorm_ref, rmsnorm, rmsnorm_ref
from .rope import rope, rope_ref
from .sample import sample_advance, sample_advance_ref, sample_logits, sample_logits_ref
from .skinny import (dequantize_mxfp4_rows, quantize_fp8_rows, quantize_fp8_rows_, quantize_mxfp4_rows,
                     quantize_mxfp4_rows_, skinny_linear, skinny_linear_fp8, skinny_linear_fp8_ref, skinny_linear_mxfp4,
                     skinny_linear_mxfp4_ref, skinny_linear_ref)
from .swiglu import silu, silu_mul, silu_mul_ref

__all__ = [
    "backend",
    "ext_available",
    "get_backend",
    "load_error",
    "load_ext",
    "set_backend",
    "use_hip",
    "FusedAdamW",
    "clip_grad_norm_",
    "multi_tensor_l2norm",
    "cross_entropy",
    "cross_entropy_ref",
    "decode_attention",
    "decode_attention_chunk",
    "decode_attention_chunk_ref",
    "decode_attention_paged",
    "decode_attention_paged_ref",
    "decode_attention_ref",
    "kv_append_rope_paged",
    "kv_append_rope_paged_ref",
    "paged_gather",
    "kv_append_rope",
    "kv_append_rope_chunk",
    "kv_append_rope_chunk_kv8_ref",
    "kv_append_rope_chunk_ref",
    "kv_append_rope_kv8_ref",
    "kv_append_rope_ref",
    "kv_dequantize",
    "kv_quantize_ref",
    "kv_quantize_rows",
    "kv_quantize_rows_ref",
    "FlashAttentionHIP",
    "FlashAttentionTorch",
    "FlashAttentionTriton",
    "flash_attention",
    "naive_attention",
    "add_rmsnorm",
    "add_rmsnorm_ref",
    "rmsnorm",
    "rmsnorm_ref",
    "rope",
    "rope_ref",
    "sample_advance",
    "sample_advance_ref",
    "sample_logits",
    "sample_logits_ref",
    "dequantize_mxfp4_rows",
    "quantize_fp8_rows",
    "quantize_fp8_rows_",
    "quantize_mxfp4_rows",
    "quantize_mxfp4_rows_",
    "skinny_linear",
    "skinny_linear_fp8",
    "skinny_linear_fp8_ref",
    "skinny_linear_mxfp4",
    "skinny_linear_mxfp4_ref",
    "skinny_linear_ref",
    "silu",
    "silu_mul",
    "silu_mul_ref",
]
