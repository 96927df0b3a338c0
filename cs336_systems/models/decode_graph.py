"""One cached decode step of ``BasicsTransformerLM``, captured into a HIP graph and replayed.

An eager decode step is host-bound: Python issues about 190 GEMMs and 290 other launches per token
for roughly a millisecond of GPU work (``profiles/decode_attention.md``). Nothing in the step
synchronizes the host -- positions and lengths live in the device tensor ``cache.lengths`` -- so the
whole step is recorded once into a ``torch.cuda.CUDAGraph`` (hipGraph on ROCm) and replayed with one
launch per token. Its M = batch projections run the weight-streaming skinny-M kernel
(``csrc/gemm/gemm_skinny.hip``) through ``gemm.skinny_decode()``.

One step function serves both modes: the decode branch of ``forward_cached`` with the FIXED
decode-attention bound ``max_kv_len = cache.max_len`` (the key-split count is baked into a captured
launch and cannot follow the host's ``start + 1``). ``capture=False`` runs it eagerly on every
:meth:`DecodeGraph.step`: the fallback, the CPU path and the comparison arm of the tests
(``tests/test_decode_graph_gpu.py`` checks replays bitwise against it).

Contract: the graph is tied to this ``cache`` object and to the parameters' storage.
``cache.reset()`` followed by a new eager prefill of any length and then ``step`` is supported, and
in-place weight updates are picked up by the next replay; ``model.to(...)`` or anything else that
re-allocates the parameters invalidates the graph (not detected). An fp32 model under autocast works
(construct and step under the same autocast context: the weight casts are captured) but re-casts
every weight per token -- hold the model in bf16.

``tokens=n`` (n > 1) captures the n-token chunk step instead (``ops.kv_append_rope_chunk`` and
``ops.decode_attention_chunk``): the verify step of speculative decoding, or a fixed-size follow-up
chunk. Its projections have ``B * n`` rows; up to 16 they run the skinny kernel, which reads every
weight once whatever the row count, and above that the ordinary GEMM path. ``cache.truncate`` is, like
``reset``, an in-place update of ``cache.lengths`` and leaves the graph valid.

``weights=qw`` (an ``Fp8DecodeWeights`` of this model, ``models/quantized.py``): the step's projections
read the FP8 copy of their weights through ``gemm.skinny_decode(fp8=qw)`` -- the FP8 weight-streaming
kernel (the e4m3 weight format of ``csrc/gemm/gemm_skinny.hip``) at up to 16 rows -- in the captured, the
eager and the
``tokens=n`` step alike. Only the steps a ``DecodeGraph`` runs read FP8: the prefill is an ordinary
``forward_cached`` on the 16-bit weights. After an in-place weight update call ``qw.refresh()``, which
requantizes in place; the next replay picks it up.

An FP8 cache (``KVCache(fp8=True)``) needs no argument: the graph is tied to its cache, the step appends
and reads quantized rows (``csrc/flash_attn/fa_decode_kv8.hip``, ``fa_decode_chunk_kv8.hip``) and nothing
in it synchronizes the host either. ``weights=qw`` and an FP8 cache combine.
"""

from __future__ import annotations

import torch

from ..ops import gemm


class DecodeGraph:
    """``logits = dg.step(tok)``: ``tok`` (B, tokens) int64 -> (B, tokens, vocab), the cache advanced
    by ``tokens`` (default 1)."""

    def __init__(self, model, cache, capture: bool = True, warmup: int = 2, tokens: int = 1, weights=None):
        if getattr(model, "tensor_parallel", None) is not None or any(
                layer.attn.context_parallel is not None for layer in model.layers):
            raise NotImplementedError("DecodeGraph does not support tensor / context parallelism")
        if cache.num_layers != len(model.layers):
            raise ValueError("cache was built for a different number of layers")
        if capture and not cache.k.is_cuda:
            raise ValueError("DecodeGraph(capture=True) captures HIP graphs: the model and cache must be on a GPU")
        if int(tokens) != tokens or tokens < 1:
            raise ValueError("DecodeGraph needs tokens >= 1")
        if weights is not None and getattr(weights, "model", None) is not model:
            raise ValueError("weights= was built for a different model")
        self.model, self.cache, self.tokens, self.weights = model, cache, int(tokens), weights
        self.graph = None
        if not capture:
            return
        dev = cache.k.device
        self.tok = torch.zeros(cache.batch, self.tokens, dtype=torch.int64, device=dev)
        # Warm-up and capture leave the cache as they found it: a warm-up step writes its K / V rows
        # from index ``length`` on, which no one reads (past the cache's end the append kernels store nothing),
        # and lengths / length are put back; capturing executes nothing but the host bookkeeping.
        lengths, length = cache.lengths.clone(), cache.length
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            # eager steps on the capture stream: allocator pools, lazy initialisation and GEMM
            # selection, none of which may happen inside a capture
            for _ in range(max(1, warmup)):
                self._run(self.tok)
                cache.lengths.copy_(lengths)
                cache.length = length
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.logits = self._run(self.tok)
        cache.length = length

    @torch.no_grad()
    def _run(self, tok: torch.Tensor) -> torch.Tensor:
        """The step both modes run: the decode (or, for ``tokens > 1``, chunk) branch of
        ``forward_cached`` (also on an empty cache, where the warm-up's rows land at index 0, unread)
        with the fixed attention bound."""
        with gemm.skinny_decode(fp8=self.weights):
            return self.model._forward_cached(tok, self.cache, max(self.cache.length, 1), self.cache.max_len)

    def step(self, tok: torch.Tensor) -> torch.Tensor:
        """Logits (B, tokens, vocab) of the tokens ``tok`` (B, tokens) that follow the cached ones; the
        cache then holds them too. With ``capture=True`` the result is the graph's static output buffer: it
        stays valid until the next ``step``, which overwrites it. A failed check changes nothing."""
        cache = self.cache
        n = self.tokens
        if tok.dim() != 2 or tok.shape[0] != cache.batch or tok.shape[1] != n:
            raise ValueError(f"DecodeGraph.step takes (B, {n}) token ids with B = {cache.batch}")
        if cache.length < 1:
            raise ValueError("DecodeGraph.step on an empty cache: prefill first (forward_cached on the prompt)")
        if cache.length + n > min(cache.max_len, self.model.context_length):
            raise ValueError(f"{cache.length} cached + {n} new token{'s' if n > 1 else ''} exceed the cache "
                             f"(max_len {cache.max_len}, context_length {self.model.context_length})")
        if self.graph is None:
            return self._run(tok)
        self.tok.copy_(tok)
        self.graph.replay()
        cache.length += n  # the captured ``lengths += n`` advanced the device tensor
        return self.logits
