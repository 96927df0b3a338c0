"""Greedy speculative decoding over two KV caches.

A small ``draft`` model proposes ``k`` tokens with ``k + 1`` single-token cached steps; the ``target``
scores ``[last, d1..dk]`` in ONE chunk step (``forward_cached(chunk=True)``: ``ops.kv_append_rope_chunk``
+ ``ops.decode_attention_chunk``) and keeps the proposals that equal its own argmax. The target's
projections have ``B * (k + 1) <= 16`` rows, which the skinny-M GEMM streams at the cost of one row,
so a verify step costs about one ordinary step and yields up to ``k + 1`` tokens. The output is
exactly what greedy cached decoding of the target emits, whatever the draft proposes.

One round, with ``P`` tokens in both caches and ``last`` the newest token, not yet cached:

1. the draft takes ``k + 1`` cached steps on ``last, d1, .., dk`` (the final step's output is unused:
   it only puts ``dk`` into the draft's cache, so the draft never needs a multi-token step);
2. the target takes one chunk step on ``[last, d1..dk]``; its argmaxes are ``t0..tk``;
3. ``m`` = the minimum over the batch of the number of leading ``i`` with ``d(i+1) == t(i)``; the
   round emits ``d1..dm, tm``;
4. both caches are truncated to ``P + m + 1``.

The batch stays rectangular (one ``m`` for all sequences), so ``cache.length`` stays valid. Near the
end of the window ``k`` shrinks to what fits; when not even ``last`` plus one proposal fits, the
remaining tokens take the ordinary cached and then sliding-window steps of ``generate``.

Greedy only: sampling-based acceptance and per-sequence (ragged) acceptance are out of scope.
"""

from __future__ import annotations

import torch

from .decode_graph import DecodeGraph
from .kv_cache import KVCache


def _new_cache(model, batch: int, fp8: bool = False) -> KVCache:
    w = model.lm_head.weight
    dev = w.device.type
    cdt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else w.dtype
    return KVCache(model, batch, device=w.device, dtype=cdt, fp8=fp8)


def _argmax(logits: torch.Tensor) -> torch.Tensor:
    return logits.float().argmax(dim=-1)


@torch.no_grad()
def speculative_generate(target, draft, x: torch.Tensor, max_new_tokens: int, draft_tokens: int = 4,
                         eos_token_id: int | None = None, graph: bool = False, kv_fp8: bool = False):
    """``(tokens, stats)``: the greedy continuation of ``x`` under ``target`` (B, <= max_new_tokens)
    and ``stats = dict(rounds, proposed, accepted)`` -- speculative rounds, draft tokens proposed and
    proposals accepted.

    ``graph=True`` (GPU models): the draft's steps replay a ``DecodeGraph(tokens=1)`` and the target's
    verify step a ``DecodeGraph(tokens=draft_tokens + 1)``; rounds with a shrunk ``k`` run eagerly.
    ``kv_fp8=True``: both caches are FP8 ones (``KVCache(fp8=True)``); the output is then the greedy
    decoding of the target over its FP8 cache."""
    if target.lm_head.weight.shape[0] != draft.lm_head.weight.shape[0]:
        raise ValueError("speculative decoding needs one vocabulary: the draft's differs from the target's")
    if draft.context_length < target.context_length:
        raise ValueError(f"the draft's context_length {draft.context_length} is below the target's "
                         f"{target.context_length}")
    if int(draft_tokens) != draft_tokens or not 1 <= draft_tokens <= 15:
        raise ValueError("draft_tokens must be in [1, 15] (a verify step has at most 16 rows per sequence)")
    if not isinstance(graph, bool):
        raise ValueError("speculative decoding takes graph=True or False")
    if graph and not (target.lm_head.weight.is_cuda and draft.lm_head.weight.is_cuda):
        raise ValueError("graph=True captures HIP graphs: both models must be on a GPU")
    if x.dim() == 1:
        x = x.unsqueeze(0)
    B, orig = x.shape
    stats = dict(rounds=0, proposed=0, accepted=0)
    if max_new_tokens <= 0:
        return x[:, orig:], stats
    window = target.context_length
    one = B == 1 and eos_token_id is not None

    def done() -> bool:
        return x.size(1) - orig >= max_new_tokens

    # prefill both caches on the prompt (its last ``window`` tokens); the target's last logits give
    # the first token
    ctx = x[:, -window:] if x.size(1) > window else x
    tc, dc = _new_cache(target, B, kv_fp8), _new_cache(draft, B, kv_fp8)
    last = _argmax(target.forward_cached(ctx, tc)[:, -1])[:, None]
    if one and int(last) == eos_token_id:
        return x[:, orig:], stats
    x = torch.cat((x, last), dim=1)
    stopped = False
    if not done() and x.size(1) <= window:
        draft.forward_cached(ctx, dc)
        lim = min(tc.max_len, window, dc.max_len)
        dgd = DecodeGraph(draft, dc, capture=True) if graph else None
        dgt = None
        while not done():
            P = tc.length  # == dc.length == x.size(1) - 1
            k = min(int(draft_tokens), lim - P - 1)
            if k < 1:
                break
            tok, props = last, []
            for i in range(k + 1):
                logits = dgd.step(tok) if dgd is not None else draft.forward_cached(tok, dc)
                if i < k:
                    tok = _argmax(logits[:, -1])[:, None]
                    props.append(tok)
            props = torch.cat(props, dim=1)  # (B, k)
            chunk = torch.cat((last, props), dim=1)
            if graph and k == draft_tokens:
                if dgt is None:
                    dgt = DecodeGraph(target, tc, capture=True, tokens=k + 1)
                t = _argmax(dgt.step(chunk))
            else:
                t = _argmax(target.forward_cached(chunk, tc, chunk=True))  # (B, k + 1)
            lead = (props == t[:, :k]).long().cumprod(dim=1).sum(dim=1)  # leading agreements per sequence
            m = int(lead.min())
            emit = torch.cat((props[:, :m], t[:, m:m + 1]), dim=1)
            tc.truncate(P + m + 1)
            dc.truncate(P + m + 1)
            stats["rounds"] += 1
            stats["proposed"] += k
            stats["accepted"] += m
            if one:
                hit = (emit[0] == eos_token_id).nonzero()
                if hit.numel():
                    emit = emit[:, :int(hit[0])]
                    stopped = True
            x = torch.cat((x, emit), dim=1)
            last = emit[:, -1:]
            if stopped:
                break
    # what the window has no room to speculate on: the cached, then sliding-window steps of generate
    cache = tc
    while not stopped and not done():
        ctx = x[:, -window:] if x.size(1) > window else x
        if cache is not None and cache.length + 1 == x.size(1) <= window:
            logits = target.forward_cached(x[:, -1:], cache)
        else:
            cache = None
            logits = target(ctx)
        nxt = _argmax(logits[:, -1])[:, None]
        if one and int(nxt) == eos_token_id:
            break
        x = torch.cat((x, nxt), dim=1)
    return x[:, orig:orig + max_new_tokens], stats
