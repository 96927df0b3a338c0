"""Key / value cache of ``BasicsTransformerLM.forward_cached``.

``k`` and ``v`` are ``(L, B, H, max_len, d)``: ``cache.k[l]`` is the ``(B, H, max_len, d)`` view the
decode-attention kernel reads in place (layer and batch are the outer dims, so a layer slice or a
batch sub-view needs no copy). K rows are stored rotated (RoPE at the row's position). ``lengths``
is the per-sequence int32 length on the device (what the kernels read); ``length`` is its host
mirror: ``generate`` batches are rectangular, so one number describes them all and no step has to
read the device tensor back.

``fp8=True``: ``k`` and ``v`` are ``torch.float8_e4m3fn`` planes of the same shape and ``k_scale`` /
``v_scale`` ``(L, B, H, max_len)`` fp32 planes hold one scale per cached row, the row being
``bytes * scale[row]`` (``ops/decode.py``): ``d + 4`` bytes per row instead of ``2 d``. Rows are
quantized when they are written and never again. ``dtype`` stays the compute dtype (what q and the
attention output are)."""

from __future__ import annotations

import torch


class KVCache:
    def __init__(self, model_or_dims, batch: int, max_len: int | None = None, device=None, dtype=None,
                 fp8: bool = False):
        """``model_or_dims``: a ``BasicsTransformerLM`` (layers, heads, head dim, ``context_length``,
        device and parameter dtype are taken from it) or ``(num_layers, num_heads, d_head)``."""
        if isinstance(model_or_dims, (tuple, list)):
            L, H, d = (int(x) for x in model_or_dims)
            if max_len is None:
                raise ValueError("KVCache from dims needs max_len")
        else:
            m = model_or_dims
            attn = m.layers[0].attn
            L, H, d = len(m.layers), attn.num_heads, attn.d_k
            w = attn.q_proj.weight
            if max_len is None:
                max_len = m.context_length
            if device is None:
                device = w.device
            if dtype is None:
                dtype = w.dtype
        if batch < 1 or max_len < 1:
            raise ValueError("KVCache needs batch >= 1 and max_len >= 1")
        self.num_layers, self.batch, self.num_heads, self.max_len, self.d_head = L, int(batch), H, int(max_len), d
        self.fp8 = bool(fp8)
        self._dtype = torch.empty((), dtype=dtype).dtype  # (None: the default dtype, as torch.zeros takes it)
        if self.fp8:
            self.k = torch.zeros(L, batch, H, max_len, d, device=device, dtype=torch.uint8).view(torch.float8_e4m3fn)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.ones(L, batch, H, max_len, device=device, dtype=torch.float32)
            self.v_scale = torch.ones_like(self.k_scale)
        else:
            self.k = torch.zeros(L, batch, H, max_len, d, device=device, dtype=dtype)
            self.v = torch.zeros_like(self.k)
            self.k_scale = self.v_scale = None
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)
        self.length = 0

    @property
    def device(self):
        return self.k.device

    @property
    def dtype(self):
        """The compute dtype: the planes' own for a plain cache, the one given for an FP8 cache."""
        return self._dtype

    @property
    def nbytes(self) -> int:
        """Bytes of the K / V planes (and their scale planes)."""
        return sum(t.numel() * t.element_size() for t in (self.k, self.v, self.k_scale, self.v_scale) if t is not None)

    def reset(self) -> None:
        """Forget every cached token (the rows are not cleared: rows beyond ``length`` are never read)."""
        self.lengths.zero_()
        self.length = 0

    def truncate(self, length: int) -> None:
        """Forget the tokens at and beyond ``length`` (rejected draft tokens of a speculative round;
        their rows stay and are overwritten). In place and without a host sync, so a ``DecodeGraph``
        tied to this cache stays valid."""
        length = int(length)
        if length < 0 or length > self.length:
            raise ValueError(f"truncate({length}) on a cache of length {self.length}")
        self.lengths.fill_(length)
        self.length = length

    def advance(self, n: int) -> None:
        self.lengths += n
        self.length += n

    def __repr__(self):
        return (f"KVCache(layers={self.num_layers}, batch={self.batch}, heads={self.num_heads}, "
                f"max_len={self.max_len}, d_head={self.d_head}, length={self.length}, dtype={self.dtype}"
                f"{', format=e4m3 rows + fp32 row scales' if self.fp8 else ''})")
