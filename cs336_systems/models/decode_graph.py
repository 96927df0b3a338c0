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
requantizes in place; the next replay picks it up. An ``Mxfp4DecodeWeights`` is taken the same way: the
step then reads the MXFP4 copy through ``csrc/gemm/gemm_skinny_w4.hip``; the weights object says which
linear runs.

An FP8 cache (``KVCache(fp8=True)``) needs no argument: the graph is tied to its cache, the step appends
and reads quantized rows (``csrc/flash_attn/fa_decode_kv8.hip``, ``fa_decode_chunk_kv8.hip``) and nothing
in it synchronizes the host either. ``weights=qw`` and an FP8 cache combine.

A ``PagedKVCache`` needs no argument either: the captured step reads ``cache.block_table`` and
``cache.lengths`` at their fixed addresses (``csrc/flash_attn/fa_decode_paged.hip``), and ``step`` /
``advance(n)`` call ``cache.reserve`` for every token they are about to replay -- host-side list work and
device-side fills, no read-back -- before replaying. ``weights=`` and ``sampler=`` combine with it;
``tokens > 1`` raises (there is no paged chunk kernel).

``sampler=Sampler(temperature, top_k, eos_token_id)`` (``tokens == 1`` only) puts the sampling into the
graph, so that the host neither sees the logits nor issues anything per token but the replay. The
captured sequence is the model step on ``self.tok``, ``ops.sample_advance`` on its logits
(``csrc/ops/sample.hip``: it writes the next ``self.tok`` and ``out[:, step]`` and latches ``done`` at
``eos_token_id``) and ``step += 1``. The random numbers are a ``(steps, B)`` table drawn by torch in
:meth:`DecodeGraph.begin`, row ``s`` for token ``s``; the kernel has no generator, so a run is reproduced
from the table. ``out``, the table, ``step`` and ``done`` are allocated once with ``cache.max_len`` columns
/ rows: the graph stays valid across ``begin`` calls. The interface is ``begin`` / ``advance`` /
``all_done`` / ``tokens``; ``step`` is not available. ``capture=False`` runs the same sequence eagerly and
emits identical tokens; ``weights=`` and FP8 caches combine with it unchanged.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..ops import gemm


@dataclass(frozen=True)
class Sampler:
    """How a ``DecodeGraph`` (or ``generate(sample_on_device=True)``) samples: the rule of
    ``ops/sample.py``. ``top_k`` ``None`` or 0: no filter; ``eos_token_id`` ``None``: no end token."""

    temperature: float = 1.0
    top_k: int | None = None
    eos_token_id: int | None = None

    def __post_init__(self):
        if not self.temperature > 0:
            raise ValueError(f"Sampler needs temperature > 0 (got {self.temperature})")
        if self.top_k is not None and (int(self.top_k) != self.top_k or self.top_k < 0):
            raise ValueError(f"Sampler needs top_k None or an integer >= 0 (got {self.top_k})")
        if self.eos_token_id is not None and (int(self.eos_token_id) != self.eos_token_id or self.eos_token_id < 0):
            raise ValueError(f"Sampler needs eos_token_id None or a token id (got {self.eos_token_id})")


class DecodeGraph:
    """``logits = dg.step(tok)``: ``tok`` (B, tokens) int64 -> (B, tokens, vocab), the cache advanced
    by ``tokens`` (default 1)."""

    def __init__(self, model, cache, capture: bool = True, warmup: int = 2, tokens: int = 1, weights=None,
                 sampler: Sampler | None = None):
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
        self.paged = getattr(cache, "block_table", None) is not None
        if self.paged and tokens != 1:
            raise NotImplementedError("DecodeGraph on a PagedKVCache takes tokens == 1: there is no paged chunk step")
        if sampler is not None and tokens != 1:
            raise ValueError("DecodeGraph(sampler=...) samples one token per step: it needs tokens == 1")
        self.model, self.cache, self.n_tokens, self.weights = model, cache, int(tokens), weights
        self.sampler = sampler
        self.graph = None
        dev = cache.k.device
        if sampler is not None:
            # fixed capacity (the cache cannot hold more steps than max_len): begin() never re-allocates
            cap = cache.max_len
            self.tok = torch.zeros(cache.batch, 1, dtype=torch.int64, device=dev)
            self.out = torch.zeros(cache.batch, cap, dtype=torch.int64, device=dev)
            self.u = torch.zeros(cap, cache.batch, dtype=torch.float32, device=dev)
            self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
            self.done = torch.zeros(cache.batch, dtype=torch.int32, device=dev)
            self._step = self._steps = 0  # host mirror of step_t; the length of the run begin() started
        if not capture:
            return
        if sampler is None:
            self.tok = torch.zeros(cache.batch, self.n_tokens, dtype=torch.int64, device=dev)
        run = self._run_sampled if sampler is not None else lambda: self._run(self.tok)
        # Warm-up and capture leave the cache as they found it: a warm-up step writes its K / V rows
        # from index ``length`` on, which no one reads (past the cache's end the append kernels store nothing),
        # and lengths / length are put back; capturing executes nothing but the host bookkeeping. On a paged
        # cache nothing is reserved here, so the table and the free list stay as they are: where the slot
        # has no page the append stores nothing (its guard), else the row lands in the sequence's own page.
        lengths, length = cache.lengths.clone(), cache.length
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            # eager steps on the capture stream: allocator pools, lazy initialisation and GEMM
            # selection, none of which may happen inside a capture
            for _ in range(max(1, warmup)):
                run()
                cache.lengths.copy_(lengths)
                cache.length = length
            if sampler is not None:  # the warm-up sampled into them
                for t in (self.tok, self.out, self.step_t, self.done):
                    t.zero_()
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.logits = run()
        cache.length = length

    @torch.no_grad()
    def _run(self, tok: torch.Tensor) -> torch.Tensor:
        """The step both modes run: the decode (or, for ``tokens > 1``, chunk) branch of
        ``forward_cached`` (also on an empty cache, where the warm-up's rows land at index 0, unread)
        with the fixed attention bound."""
        with gemm.skinny_decode(weights=self.weights):
            return self.model._forward_cached(tok, self.cache, max(self.cache.length, 1), self.cache.max_len)

    @torch.no_grad()
    def _run_sampled(self) -> torch.Tensor:
        """The step with a sampler, in both modes: the model step on ``self.tok``, the sampler on its
        logits (next ``self.tok``, ``out[:, step]``, ``done``), ``step += 1``. Nothing synchronizes the host."""
        sp = self.sampler
        logits = self._run(self.tok)
        ops.sample_advance(logits[:, -1], self.u, self.step_t, sp.temperature, sp.top_k,
                           -1 if sp.eos_token_id is None else sp.eos_token_id, self.tok, self.out, self.done)
        self.step_t.add_(1)
        return logits

    def begin(self, first_tok: torch.Tensor, steps: int, generator=None, table: torch.Tensor | None = None) -> None:
        """Start a run of ``steps`` tokens on the prefilled cache: ``first_tok`` (B, 1), the token sampled
        from the prefill's logits, is token 0 (``out[:, 0]``) and the next step's input; ``step = 1``;
        ``done`` is cleared (and set where ``first_tok`` already is the end token). Token ``s`` uses row ``s``
        of the ``(steps, B)`` fp32 table of uniforms: ``table`` if given, else ``torch.rand`` with
        ``generator``. A failed check changes nothing."""
        if self.sampler is None:
            raise ValueError("DecodeGraph.begin needs a DecodeGraph built with sampler=")
        B = self.cache.batch
        if int(steps) != steps or steps < 1 or steps > self.out.shape[1]:
            raise ValueError(f"DecodeGraph.begin takes 1 <= steps <= {self.out.shape[1]} (the cache's max_len)")
        if first_tok.dim() != 2 or tuple(first_tok.shape) != (B, 1):
            raise ValueError(f"DecodeGraph.begin takes first_tok (B, 1) with B = {B}")
        if table is None:
            table = torch.rand(steps, B, device=self.u.device, generator=generator)
        elif tuple(table.shape) != (steps, B) or table.dtype != torch.float32:
            raise ValueError(f"DecodeGraph.begin takes an fp32 table ({steps}, {B})")
        self.u[:steps].copy_(table)
        self.tok.copy_(first_tok)
        self.out[:, :1].copy_(first_tok)
        self.step_t.fill_(1)
        eos = self.sampler.eos_token_id
        if eos is None:
            self.done.zero_()
        else:
            self.done.copy_(self.tok[:, 0] == eos)
        self._step, self._steps = 1, int(steps)

    def advance(self, n: int = 1) -> None:
        """``n`` more tokens: n replays (or eager steps), nothing read back. A failed check changes nothing."""
        cache = self.cache
        if self.sampler is None or self._steps == 0:
            raise ValueError("DecodeGraph.advance needs sampler= and a begin() first")
        if int(n) != n or n < 0:
            raise ValueError("DecodeGraph.advance needs n >= 0")
        if self._step + n > self._steps:
            raise ValueError(f"{self._step} emitted + {n} new tokens exceed the {self._steps} steps begin() was given")
        if cache.length < 1:
            raise ValueError("DecodeGraph.advance on an empty cache: prefill first (forward_cached on the prompt)")
        if cache.length + n > min(cache.max_len, self.model.context_length):
            raise ValueError(f"{cache.length} cached + {n} new tokens exceed the cache "
                             f"(max_len {cache.max_len}, context_length {self.model.context_length})")
        if self.paged:
            cache.reserve(int(n))  # pages for every token about to be replayed: host-side, nothing read back
        for _ in range(int(n)):
            if self.graph is None:
                self._run_sampled()
            else:
                self.graph.replay()
                cache.length += 1  # the captured ``lengths += 1`` advanced the device tensor
        self._step += int(n)

    def all_done(self) -> bool:
        """Whether every sequence has emitted the end token: the one read-back (none without an end token)."""
        if self.sampler is None:
            raise ValueError("DecodeGraph.all_done needs a DecodeGraph built with sampler=")
        if self.sampler.eos_token_id is None:
            return False
        return bool((self.done != 0).all().item())

    def tokens(self) -> torch.Tensor:
        """The (B, emitted) tokens of the run so far, ``first_tok`` included; a finished row holds the end
        token from its first one on."""
        if self.sampler is None:
            raise ValueError("DecodeGraph.tokens needs a DecodeGraph built with sampler=")
        return self.out[:, :self._step].clone()

    def step(self, tok: torch.Tensor) -> torch.Tensor:
        """Logits (B, tokens, vocab) of the tokens ``tok`` (B, tokens) that follow the cached ones; the
        cache then holds them too. With ``capture=True`` the result is the graph's static output buffer: it
        stays valid until the next ``step``, which overwrites it. A failed check changes nothing."""
        if self.sampler is not None:
            raise ValueError("a DecodeGraph with sampler= samples inside the step: use begin() / advance()")
        cache = self.cache
        n = self.n_tokens
        if tok.dim() != 2 or tok.shape[0] != cache.batch or tok.shape[1] != n:
            raise ValueError(f"DecodeGraph.step takes (B, {n}) token ids with B = {cache.batch}")
        if cache.length < 1:
            raise ValueError("DecodeGraph.step on an empty cache: prefill first (forward_cached on the prompt)")
        if cache.length + n > min(cache.max_len, self.model.context_length):
            raise ValueError(f"{cache.length} cached + {n} new token{'s' if n > 1 else ''} exceed the cache "
                             f"(max_len {cache.max_len}, context_length {self.model.context_length})")
        if self.paged:
            cache.reserve(n)
        if self.graph is None:
            return self._run(tok)
        self.tok.copy_(tok)
        self.graph.replay()
        cache.length += n  # the captured ``lengths += n`` advanced the device tensor
        return self.logits
