"""Decode-attention kernel sweep and end-to-end generation with / without the KV cache.

Kernel sweep: ``ops.decode_attention`` (``csrc/flash_attn/fa_decode.hip``) timed with the HIP-event
``do_bench`` (L2 + Infinity Cache flushed before every call) at (H, d) in {(25, 64), (32, 80)} --
the xl and 2.7b head layouts -- x B x kv_len, bf16: the default split count against ``splits=1`` and
a sweep of forced split counts, in us and in GB/s of K+V bytes read, beside the 6.3 TB/s achievable
HBM rate of the MI355X and ``ops.naive_attention`` on the same tensors (q as (B, H, 1, d), the
cache sliced to kv_len), the only way to compute a decode step without the kernel.

Skinny-M GEMM table (``--skinny``): ``cs336::gemm_skinny`` (``csrc/gemm/gemm_skinny.hip``) on the five
projection shapes (qkv, o, w1|w3, w2, lm_head at the GPT-2 vocabulary 50257) of ``xl`` and ``2.7b`` at
M 1 / 8 / 16, bf16, under the same ``do_bench`` protocol: us and GB/s of W bytes against the achievable
HBM rate, with ``torch.mm`` on the same operands alongside. ``--fp8`` adds, per row, the FP8 weight-only
kernel ``cs336::gemm_skinny_w8`` (the same file, e4m3 weight format) on ``quantize_fp8_rows(w)``: median and
q20-q80 over the same 50 flushed calls, GB/s of FP8 bytes, and the ratio to the bf16 skinny kernel of
the same run. ``--fp4`` adds the MXFP4 weight-only kernel ``cs336::gemm_skinny_w4``
(``csrc/gemm/gemm_skinny_w4.hip``) on ``quantize_mxfp4_rows(w)`` the same way: median, q20-q80, GB/s of its own
bytes (17/32 per weight), the ratio to the FP8 kernel (with ``--fp8``) and to the bf16 kernel of the same run,
and a verdict against each by the spread rule.

End to end: tokens/s of ``generate`` with ``use_cache=True`` against ``use_cache=False`` (a full
forward over the window per token) and against ``use_cache=True, graph=True`` (the cached step
replayed from a HIP graph over the skinny-M kernel), model ``xl`` held in bf16. ``--arms`` picks the
arms (the uncached one takes minutes at context 4096); ``graph+fp8`` is the graph arm over
``Fp8DecodeWeights`` (``generate(..., graph=True, weights=qw)``) and ``graph+fp4`` over ``Mxfp4DecodeWeights``. The graph arms also report the replayed
step alone (HIP events around 50 replays on a cache holding the prompt, truncated back every time).

    python -m cs336_systems.bench.decode --json profiles/decode_attention.json
    python -m cs336_systems.bench.decode --no-e2e --batch 8 --kv-len 4096
    python -m cs336_systems.bench.decode --no-kernel --skinny --arms cached graph --json profiles/decode_graph.json
    python -m cs336_systems.bench.decode --no-kernel --skinny --fp8 --arms graph graph+fp8 --json profiles/decode_fp8.json
    python -m cs336_systems.bench.decode --no-kernel --skinny --fp8 --fp4 --arms graph graph+fp8 graph+fp4 --json profiles/decode_fp4.json

Chunk tables (``--chunk``): ``ops.decode_attention_chunk`` (``csrc/flash_attn/fa_decode_chunk.hip``) at
n in {1, 2, 4, 8, 16} query rows over the same (B, H, d, kv_len) points: us, GB/s of K+V bytes (read
once) and the time of the n sequential ``ops.decode_attention`` launches it replaces. With
``--arms verify``: the graph-replayed step of ``xl`` in bf16 at B = 1 for ``DecodeGraph(tokens=t)``,
t in {1, 2, 4, 8, 16}, timed interleaved on one cache (truncated back after every step) -- the cost of
a speculative verify step relative to an ordinary one.

    python -m cs336_systems.bench.decode --chunk --arms verify --json profiles/decode_chunk.json

FP8 KV cache (``--kv-fp8``; ``csrc/flash_attn/fa_decode_kv8.hip``, ``fa_decode_chunk_kv8.hip``): every
kernel row and chunk row also times the same call over the FP8 form of the same K / V (e4m3 rows with
one fp32 scale per row, written by ``ops.kv_quantize_rows``): median and q20-q80 over the same 50 flushed
calls, GB/s over the bytes it reads (d + 4 per row), its share of the achievable rate and its ratio to
the 16-bit kernel of the same row, faster / slower only beyond the q20-q80 spread of both sides. The
arms ``graph+kv8`` (``generate(..., graph=True, kv_fp8=True)``) and ``graph+fp8+kv8`` (with
``Fp8DecodeWeights`` as well) report like ``graph``, with the bytes of both caches; ``--kv-fp8`` adds the
end-to-end point context 4096, B 8, prompt 2048 + 512, where the cache is the larger stream of a step.

    python -m cs336_systems.bench.decode --kv-fp8 --chunk --no-e2e --json profiles/decode_kv8_chunk.json
    python -m cs336_systems.bench.decode --kv-fp8 --no-sweep --arms graph graph+kv8 graph+fp8+kv8 --json profiles/decode_kv8.json

Fused sampler (``--sample``; ``csrc/ops/sample.hip``): ``ops.sample_logits`` at B 1 / 8 / 64 x V 10000 /
50257 x top_k 1 / 50 / none on bf16 ``logits[:, -1]`` rows, against the eager pipeline of ``generate`` it
replaces (``float() / temperature``, ``topk``, ``masked_fill``, ``softmax``, ``multinomial``) in the same run:
median and q20-q80 over the same 50 flushed calls, faster / slower only beyond the spread of both sides.
The arms ``graph+sample`` and ``graph+fp8+sample`` are ``generate(..., graph=True, sample_on_device=True)``:
ms per token beside the ``graph`` arm of the same run; with ``--sample`` every arm is timed three times
(all runs are kept, the median is reported).

    python -m cs336_systems.bench.decode --sample --no-kernel --arms graph graph+sample graph+fp8 graph+fp8+sample --json profiles/decode_sample.json

Paged cache (``--paged [--page-size 16 64 256]``; ``csrc/flash_attn/fa_decode_paged.hip``): every kernel row also
times ``ops.decode_attention_paged`` on the same K / V rows held in a page pool, the pages placed by a seeded
random permutation of a pool with spare pages (a sorted placement would flatter the kernel). The contiguous
kernel is re-measured in the same run, the arms alternating in five rounds whose samples are pooled: median
and q20-q80 per arm, the ratio to the contiguous kernel and faster / slower only beyond the spread of both
sides; ``paged<P>_bitwise`` says whether the paged output has the contiguous kernel's bits (same split
rule, same rows). The arm ``graph+paged`` is ``generate(..., graph=True, paged=True)`` (page size: the first
of ``--page-size``, default 64), reported like ``graph`` with the replayed step beside it, and the pages /
bytes a ``share_prompt`` prefill of the point's prompt holds against the dense cache.

    python -m cs336_systems.bench.decode --paged --no-sweep --arms graph graph+paged --json profiles/decode_paged.json
"""

from __future__ import annotations

import argparse
import json
import time

import torch

from .. import ops
from ..utils.timing import do_bench

HBM_ACHIEVABLE_GBS = 6300.0  # MI355X achievable HBM read rate
SPLIT_SWEEP = (1, 2, 4, 8, 16, 32, 64)


def _kv8_planes(k: torch.Tensor, v: torch.Tensor):
    """The FP8 form of (B, H, n, d) K / V tensors: byte planes, scale planes and the bytes they hold."""
    planes = []
    for x in (k, v):
        p8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device).view(torch.float8_e4m3fn)
        sc = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
        ops.kv_quantize_rows(x, p8, sc)
        planes.append((p8, sc))
    (k8, ks), (v8, vs) = planes
    nbytes = float(sum(t.numel() * t.element_size() for t in (k8, ks, v8, vs)))
    return k8, v8, ks, vs, nbytes


def _kv8_columns(row: dict, base: str, fn, nbytes: float, warmup: int, rep: int) -> None:
    """Time ``fn`` (the FP8-cache call) into ``row`` beside the 16-bit columns ``{base}_us[_q20|_q80]``."""
    med, lo, hi = do_bench(fn, warmup=warmup, rep=rep)
    row["kv8_us"], row["kv8_us_q20"], row["kv8_us_q80"] = med * 1e3, lo * 1e3, hi * 1e3
    row["kv8_mbytes"] = nbytes / 2**20
    row["kv8_gbs"] = nbytes / (row["kv8_us"] * 1e-6) / 1e9
    row["kv8_hbm_frac"] = row["kv8_gbs"] / HBM_ACHIEVABLE_GBS
    row["kv8_vs_bf16"] = row["kv8_us"] / row[f"{base}_us"]  # below 1: the FP8 cache is faster
    row["kv8_verdict"] = ("faster" if row["kv8_us_q80"] < row[f"{base}_us_q20"] else
                          "slower" if row["kv8_us_q20"] > row[f"{base}_us_q80"] else "same")


def _paged_pool(k: torch.Tensor, v: torch.Tensor, P: int, seed: int = 0, spare: int = 8):
    """The (B, H, n, d) rows of ``k`` / ``v`` in ``(num_pages, H, P, d)`` pools with ``spare`` unused pages,
    the pages placed by a seeded random permutation -> (k_pool, v_pool, block_table)."""
    B, H, n, d = k.shape
    T = -(-n // P)
    num_pages = B * T + spare
    g = torch.Generator(device=k.device).manual_seed(seed)
    table = torch.randperm(num_pages, device=k.device, generator=g)[:B * T].view(B, T)
    pools = []
    for x in (k, v):
        if T * P != n:
            x = torch.nn.functional.pad(x, (0, 0, 0, T * P - n))
        pool = torch.zeros(num_pages, H, P, d, device=k.device, dtype=k.dtype)
        pool[table] = x.view(B, H, T, P, d).permute(0, 2, 1, 3, 4)
        pools.append(pool)
    return pools[0], pools[1], table.to(torch.int32)


def _alternating(fns: dict, warmup: int, rep: int, rounds: int = 5) -> dict:
    """Time the arms ``fns`` alternating, ``rounds`` times ``rep / rounds`` flushed calls each, and pool each
    arm's samples -> name -> (median, q20, q80) in us: drift of the box's clocks hits every arm alike."""
    samples = {name: [] for name in fns}
    per = max(1, rep // rounds)
    for r in range(rounds):
        for name, fn in fns.items():
            samples[name] += do_bench(fn, warmup=warmup if r == 0 else 2, rep=per, return_all=True)
    out = {}
    for name, ts in samples.items():
        ts = sorted(ts)
        out[name] = tuple(ts[min(len(ts) - 1, int(round(x * (len(ts) - 1))))] * 1e3 for x in (0.5, 0.2, 0.8))
    return out


def kernel_row(B: int, H: int, d: int, kv_len: int, warmup: int = 10, rep: int = 50, sweep: bool = True,
               kv_fp8: bool = False, paged=()) -> dict:
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    q = torch.randn(B, H, d, device=dev, dtype=dt)
    k = torch.randn(B, H, kv_len, d, device=dev, dtype=dt)
    v = torch.randn(B, H, kv_len, d, device=dev, dtype=dt)
    lens = torch.full((B,), kv_len, dtype=torch.int32, device=dev)
    kv_bytes = 2.0 * B * H * kv_len * d * k.element_size()
    row = dict(B=B, H=H, d=d, kv_len=kv_len, dtype="bf16", kv_mbytes=kv_bytes / 2**20)

    def t(fn):
        return do_bench(fn, warmup=warmup, rep=rep)[0] * 1e3  # us

    def gbs(us):
        return kv_bytes / (us * 1e-6) / 1e9

    row["default_splits"] = int(torch.ops.cs336.fa_decode_splits(B, H, d, k.element_size(), kv_len))
    row["default_us"] = t(lambda: ops.decode_attention(q, k, v, lens))
    row["splits1_us"] = t(lambda: ops.decode_attention(q, k, v, lens, splits=1))
    q4 = q.unsqueeze(2)
    row["naive_us"] = t(lambda: ops.naive_attention(q4, k, v, is_causal=False))
    for name in ("default", "splits1", "naive"):
        row[f"{name}_gbs"] = gbs(row[f"{name}_us"])
    row["default_hbm_frac"] = row["default_gbs"] / HBM_ACHIEVABLE_GBS
    row["speedup_vs_naive"] = row["naive_us"] / row["default_us"]
    if sweep:
        row["sweep_us"] = {str(s): t(lambda s=s: ops.decode_attention(q, k, v, lens, splits=s)) for s in SPLIT_SWEEP}
    o, _ = ops.decode_attention(q, k, v, lens)
    ref = ops.naive_attention(q4, k, v, is_causal=False)[:, :, 0]
    row["max_abs_diff_vs_naive"] = (o.float() - ref.float()).abs().max().item()
    if kv_fp8:
        med, lo, hi = do_bench(lambda: ops.decode_attention(q, k, v, lens), warmup=warmup, rep=rep)
        row["bf16_us"], row["bf16_us_q20"], row["bf16_us_q80"] = med * 1e3, lo * 1e3, hi * 1e3  # re-measured beside kv8
        k8, v8, ks, vs, nbytes = _kv8_planes(k, v)
        row["kv8_splits"] = int(torch.ops.cs336.fa_decode_kv8_splits(B, H, d, 1, kv_len))
        row["kv8_key_tile"] = int(torch.ops.cs336.fa_decode_kv8_key_tile(d, 1))
        _kv8_columns(row, "bf16", lambda: ops.decode_attention(q, k8, v8, lens, k_scale=ks, v_scale=vs), nbytes,
                     warmup, rep)
        o8, _ = ops.decode_attention(q, k8, v8, lens, k_scale=ks, v_scale=vs)
        row["kv8_max_abs_diff_vs_bf16"] = (o8.float() - o.float()).abs().max().item()
        del k8, v8, ks, vs
    if paged:
        arms = {"contig": lambda: ops.decode_attention(q, k, v, lens)}
        pools = {}
        for P in paged:
            pools[P] = _paged_pool(k, v, P)
            arms[f"paged{P}"] = lambda P=P: ops.decode_attention_paged(q, *pools[P], lens)
        stats = _alternating(arms, warmup, rep)
        for name, (med, lo, hi) in stats.items():
            row[f"{name}_us"], row[f"{name}_us_q20"], row[f"{name}_us_q80"] = med, lo, hi
        for P in paged:
            name = f"paged{P}"
            row[f"{name}_gbs"] = gbs(row[f"{name}_us"])
            row[f"{name}_vs_contig"] = row[f"{name}_us"] / row["contig_us"]  # above 1: the paged kernel is slower
            row[f"{name}_verdict"] = ("faster" if row[f"{name}_us_q80"] < row["contig_us_q20"] else
                                      "slower" if row[f"{name}_us_q20"] > row["contig_us_q80"] else "same")
            op, lp = ops.decode_attention_paged(q, *pools[P], lens)
            oc, lc = ops.decode_attention(q, k, v, lens)
            row[f"{name}_bitwise"] = bool(torch.equal(op, oc) and torch.equal(lp, lc))
        del pools, arms
    del q, k, v
    torch.cuda.empty_cache()
    return row


CHUNK_N = (1, 2, 4, 8, 16)


def chunk_row(B: int, H: int, d: int, kv_len: int, n: int, warmup: int = 10, rep: int = 50, kv_fp8: bool = False) -> dict:
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    q = torch.randn(B, n, H, d, device=dev, dtype=dt)
    k = torch.randn(B, H, kv_len, d, device=dev, dtype=dt)
    v = torch.randn(B, H, kv_len, d, device=dev, dtype=dt)
    lens = torch.full((B,), kv_len, dtype=torch.int32, device=dev)
    kv_bytes = 2.0 * B * H * kv_len * d * k.element_size()
    qt = int(torch.ops.cs336.fa_decode_chunk_qt(n))
    row = dict(B=B, H=H, d=d, kv_len=kv_len, n=n, dtype="bf16", kv_mbytes=kv_bytes / 2**20, query_tile=qt,
               splits=int(torch.ops.cs336.fa_decode_splits(B * ((n + qt - 1) // qt), H, d, k.element_size(), kv_len)))
    q1 = [q[:, i].contiguous() for i in range(n)]

    def sequential():
        for qi in q1:
            ops.decode_attention(qi, k, v, lens)

    for key, fn in (("chunk", lambda: ops.decode_attention_chunk(q, k, v, lens)), ("sequential", sequential)):
        med, lo, hi = do_bench(fn, warmup=warmup, rep=rep)
        row[f"{key}_us"], row[f"{key}_us_q20"], row[f"{key}_us_q80"] = med * 1e3, lo * 1e3, hi * 1e3
    row["chunk_gbs"] = kv_bytes / (row["chunk_us"] * 1e-6) / 1e9
    row["chunk_hbm_frac"] = row["chunk_gbs"] / HBM_ACHIEVABLE_GBS
    row["speedup_vs_sequential"] = row["sequential_us"] / row["chunk_us"]
    o, _ = ops.decode_attention_chunk(q, k, v, lens)
    o1, _ = ops.decode_attention(q1[-1], k, v, lens)  # the last query sees every key
    row["max_abs_diff_last_query_vs_decode"] = (o[:, -1].float() - o1.float()).abs().max().item()
    if kv_fp8:
        k8, v8, ks, vs, nbytes = _kv8_planes(k, v)
        row["kv8_splits"] = int(torch.ops.cs336.fa_decode_kv8_splits(B, H, d, n, kv_len))
        row["kv8_key_tile"] = int(torch.ops.cs336.fa_decode_kv8_key_tile(d, n))
        _kv8_columns(row, "chunk", lambda: ops.decode_attention_chunk(q, k8, v8, lens, k_scale=ks, v_scale=vs), nbytes,
                     warmup, rep)
        o8, _ = ops.decode_attention_chunk(q, k8, v8, lens, k_scale=ks, v_scale=vs)
        row["kv8_max_abs_diff_vs_bf16"] = (o8.float() - o.float()).abs().max().item()
        del k8, v8, ks, vs
    del q, k, v
    torch.cuda.empty_cache()
    return row


def verify_rows(model_size: str, ctx: int = 512, B: int = 1, prefix: int = 256, rep: int = 50) -> list[dict]:
    """Replayed step time of ``DecodeGraph(tokens=t)`` for every t of CHUNK_N on ONE cache of ``prefix``
    tokens, interleaved (t varies fastest; the cache is truncated back after every step), HIP events
    around the replay."""
    from ..models import DecodeGraph, build_model
    from ..models.kv_cache import KVCache

    torch.manual_seed(0)
    model = build_model(model_size, ctx, device="cuda").to(torch.bfloat16).eval()
    x = torch.randint(0, model.vocab_size, (B, prefix + max(CHUNK_N)), device="cuda")
    cache = KVCache(model, B)
    model.forward_cached(x[:, :prefix], cache)
    graphs = {t: DecodeGraph(model, cache, capture=True, tokens=t) for t in CHUNK_N}
    times = {t: [] for t in CHUNK_N}
    for r in range(rep + 5):
        for t, dg in graphs.items():
            tok = x[:, prefix:prefix + t]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dg.step(tok)
            b.record()
            b.synchronize()
            cache.truncate(prefix)
            if r >= 5:  # the first rounds warm clocks and caches
                times[t].append(a.elapsed_time(b))
    rows = []
    for t in CHUNK_N:
        ts = sorted(times[t])
        rows.append(dict(model=model_size, context_length=ctx, B=B, cached=prefix, tokens=t, dtype="bf16",
                         step_ms=ts[len(ts) // 2], step_ms_q20=ts[len(ts) // 5], step_ms_q80=ts[len(ts) * 4 // 5]))
    for r in rows:
        r["vs_one_token"] = r["step_ms"] / rows[0]["step_ms"]
        # a round of k = tokens - 1 proposals costs one verify step (plus the draft) and yields
        # 1 + accepted tokens: below this many accepted tokens per round it loses to plain steps
        r["break_even_accepted_per_round"] = r["vs_one_token"] - 1.0
    del graphs, model, cache
    torch.cuda.empty_cache()
    return rows


SKINNY_M = (1, 8, 16)
LM_HEAD_VOCAB = 50257  # the GPT-2 vocabulary: N is not a multiple of 16 (nor of 4)


def skinny_shapes(model_size: str) -> list[tuple[str, int, int]]:
    """(name, N, K) of the five projections of a decode step."""
    from ..models import get_model_config

    c = get_model_config(model_size)
    d, f = c["d_model"], c["d_ff"]
    return [("qkv", 3 * d, d), ("o", d, d), ("w1|w3", 2 * f, d), ("w2", d, f), ("lm_head", LM_HEAD_VOCAB, d)]


def skinny_row(model_size: str, name: str, M: int, N: int, K: int, warmup: int = 10, rep: int = 50,
               fp8: bool = False, fp4: bool = False) -> dict:
    from ..ops import gemm

    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    x = torch.randn(M, K, device=dev, dtype=dt)
    w = torch.randn(N, K, device=dev, dtype=dt) * K**-0.5
    out = torch.empty(M, N, device=dev, dtype=dt)
    w_bytes = float(N * K * w.element_size())
    row = dict(model=model_size, proj=name, M=M, N=N, K=K, dtype="bf16", w_mbytes=w_bytes / 2**20)

    def t(fn):
        med, lo, hi = do_bench(fn, warmup=warmup, rep=rep)
        return med * 1e3, lo * 1e3, hi * 1e3  # us: median, 20 % and 80 % quantiles

    assert gemm.skinny_ok(x, w)
    for key, fn in (("skinny", lambda: torch.ops.cs336.gemm_skinny(x, w, out)), ("mm", lambda: torch.mm(x, w.t()))):
        row[f"{key}_us"], row[f"{key}_us_q20"], row[f"{key}_us_q80"] = t(fn)
        row[f"{key}_gbs"] = w_bytes / (row[f"{key}_us"] * 1e-6) / 1e9
    row["skinny_hbm_frac"] = row["skinny_gbs"] / HBM_ACHIEVABLE_GBS
    row["speedup_vs_mm"] = row["mm_us"] / row["skinny_us"]
    torch.ops.cs336.gemm_skinny(x, w, out)
    row["max_abs_diff_vs_mm"] = (out.float() - torch.mm(x, w.t()).float()).abs().max().item()
    if fp8:
        wq, scale = ops.quantize_fp8_rows(w)
        assert gemm.skinny_w8_ok(x, wq, scale)
        q_bytes = float(N * K * wq.element_size() + N * scale.element_size())
        row["fp8_us"], row["fp8_us_q20"], row["fp8_us_q80"] = t(lambda: torch.ops.cs336.gemm_skinny_w8(x, wq, scale, out))
        row["fp8_mbytes"] = q_bytes / 2**20
        row["fp8_gbs"] = q_bytes / (row["fp8_us"] * 1e-6) / 1e9
        row["fp8_hbm_frac"] = row["fp8_gbs"] / HBM_ACHIEVABLE_GBS
        row["fp8_vs_skinny"] = row["fp8_us"] / row["skinny_us"]  # below 1: the FP8 kernel is faster
        # faster / slower only beyond the q20-q80 spread of both sides
        row["fp8_verdict"] = ("faster" if row["fp8_us_q80"] < row["skinny_us_q20"] else
                              "slower" if row["fp8_us_q20"] > row["skinny_us_q80"] else "same")
        ref = ops.skinny_linear_fp8_ref(x, wq, scale)
        row["fp8_max_abs_diff_vs_ref"] = (out.float() - ref.float()).abs().max().item()
        del wq, scale
    if fp4:
        wq, scale = ops.quantize_mxfp4_rows(w)
        assert gemm.skinny_w4_ok(x, wq, scale)
        q_bytes = float(wq.numel() + scale.numel())
        row["fp4_us"], row["fp4_us_q20"], row["fp4_us_q80"] = t(lambda: torch.ops.cs336.gemm_skinny_w4(x, wq, scale, out))
        row["fp4_mbytes"] = q_bytes / 2**20
        row["fp4_gbs"] = q_bytes / (row["fp4_us"] * 1e-6) / 1e9
        row["fp4_hbm_frac"] = row["fp4_gbs"] / HBM_ACHIEVABLE_GBS
        for base in ("skinny",) + (("fp8",) if fp8 else ()):  # below 1: the MXFP4 kernel is faster
            row[f"fp4_vs_{base}"] = row["fp4_us"] / row[f"{base}_us"]
            row[f"fp4_verdict_vs_{base}"] = ("faster" if row["fp4_us_q80"] < row[f"{base}_us_q20"] else
                                             "slower" if row["fp4_us_q20"] > row[f"{base}_us_q80"] else "same")
        ref = ops.skinny_linear_mxfp4_ref(x, wq, scale)
        row["fp4_max_abs_diff_vs_ref"] = (out.float() - ref.float()).abs().max().item()
        del wq, scale
    del x, w, out
    torch.cuda.empty_cache()
    return row


SAMPLE_B, SAMPLE_V, SAMPLE_K = (1, 8, 64), (10000, 50257), (1, 50, None)


def sample_row(B: int, V: int, top_k, warmup: int = 10, rep: int = 50) -> dict:
    """The fused sampler against the eager sampling of ``generate`` on the same logits."""
    torch.manual_seed(0)
    x = (torch.randn(B, 1, V, device="cuda") * 4).to(torch.bfloat16)[:, -1]
    u = torch.rand(B, device="cuda")
    temperature = 0.8

    def eager():
        logits = x.float() / temperature
        if top_k:
            vals, _ = torch.topk(logits, min(top_k, V))
            logits = logits.masked_fill(logits < vals[:, -1:], float("-inf"))
        return torch.multinomial(torch.softmax(logits, dim=-1), 1)

    row = dict(B=B, V=V, top_k=top_k, dtype="bf16", logits_kbytes=B * V * 2 / 1024)
    for key, fn in (("fused", lambda: ops.sample_logits(x, u, temperature, top_k)), ("eager", eager)):
        med, lo, hi = do_bench(fn, warmup=warmup, rep=rep)
        row[f"{key}_us"], row[f"{key}_us_q20"], row[f"{key}_us_q80"] = med * 1e3, lo * 1e3, hi * 1e3
    row["fused_vs_eager"] = row["fused_us"] / row["eager_us"]  # below 1: the fused kernel is faster
    row["verdict"] = ("faster" if row["fused_us_q80"] < row["eager_us_q20"] else
                      "slower" if row["fused_us_q20"] > row["eager_us_q80"] else "same")
    return row


ARMS = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "graph": dict(use_cache=True, graph=True),
        "graph+fp8": dict(use_cache=True, graph=True),  # (+ weights=Fp8DecodeWeights(model), built per model)
        "graph+fp4": dict(use_cache=True, graph=True),  # (+ weights=Mxfp4DecodeWeights(model))
        "graph+kv8": dict(use_cache=True, graph=True, kv_fp8=True),
        "graph+fp8+kv8": dict(use_cache=True, graph=True, kv_fp8=True),  # (+ weights)
        "graph+sample": dict(use_cache=True, graph=True, sample_on_device=True),
        "graph+fp8+sample": dict(use_cache=True, graph=True, sample_on_device=True),  # (+ weights)
        "graph+paged": dict(use_cache=True, graph=True, paged=True)}  # (+ page_size)
ARM_KEYS = {"graph": "cached_graph", "graph+paged": "cached_graph_paged", "graph+fp8": "cached_graph_fp8", "graph+fp4": "cached_graph_fp4", "graph+kv8": "cached_graph_kv8",
            "graph+fp8+kv8": "cached_graph_fp8_kv8"}


def replay_ms(model, x: torch.Tensor, weights=None, rep: int = 50, kv_fp8: bool = False,
              page_size: int | None = None) -> tuple[float, float, float]:
    """Median, q20 and q80 ms of one replayed decode step on a cache holding the prompt ``x`` (HIP
    events around the replay; the cache is truncated back after every step). ``page_size``: on a
    ``PagedKVCache``, holding one token more than the prompt, so that the timed step is the ordinary one
    inside a page and not the one in ``page_size`` that takes a new page."""
    from ..models import DecodeGraph
    from ..models.kv_cache import KVCache, PagedKVCache

    B, prompt = x.shape
    cache = KVCache(model, B, fp8=kv_fp8) if page_size is None else PagedKVCache(model, B, page_size=page_size)
    model.forward_cached(x, cache)
    dg = DecodeGraph(model, cache, capture=True, weights=weights)
    if page_size is not None:
        dg.step(x[:, -1:])
        prompt += 1
    tok, ts = x[:, -1:], []
    for r in range(rep + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dg.step(tok)
        b.record()
        b.synchronize()
        cache.truncate(prompt)
        if r >= 5:  # the first rounds warm clocks and caches
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[len(ts) // 5], ts[len(ts) * 4 // 5]


def e2e_row(model_size: str, ctx: int, B: int, prompt: int, new: int, arms=("cached", "uncached", "graph"),
            runs: int = 1, page_size: int = 64) -> dict:
    from ..models import build_model

    torch.manual_seed(0)
    model = build_model(model_size, ctx, device="cuda").to(torch.bfloat16).eval()
    x = torch.randint(0, model.vocab_size, (B, prompt), device="cuda")
    row = dict(model=model_size, context_length=ctx, B=B, prompt=prompt, new_tokens=new, dtype="bf16")
    qw = q4 = None
    for arm in arms:
        kw = dict(ARMS[arm])
        if arm == "graph+fp4":
            from ..models import Mxfp4DecodeWeights

            q4 = q4 or Mxfp4DecodeWeights(model)
            kw["weights"] = q4
            row["fp4_weight_mbytes"] = q4.nbytes / 2**20
        if arm in ("graph+fp8", "graph+fp8+kv8", "graph+fp8+sample"):
            from ..models import Fp8DecodeWeights

            qw = qw or Fp8DecodeWeights(model)
            kw["weights"] = qw
            row["fp8_weight_mbytes"] = qw.nbytes / 2**20
        if kw.get("paged"):
            kw["page_size"] = page_size
            row["page_size"] = page_size
        model.generate(x, 4, top_k=1, **kw)  # warm-up: GEMM selection, allocator
        dts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(x, new, top_k=1, **kw)  # (the graph arm's time includes its capture)
            torch.cuda.synchronize()
            dts.append(time.perf_counter() - t0)
            assert out.shape == (B, new)
        dt = sorted(dts)[len(dts) // 2]
        name = ARM_KEYS.get(arm, arm.replace("graph", "cached_graph").replace("+", "_"))
        if runs > 1:
            row[f"{name}_ms_per_step_runs"] = [t / new * 1e3 for t in dts]
        row[f"{name}_s"] = dt
        row[f"{name}_tok_s"] = B * new / dt
        row[f"{name}_ms_per_step"] = dt / new * 1e3
        if arm in ARM_KEYS:
            med, lo, hi = replay_ms(model, x, kw.get("weights"), kv_fp8=kw.get("kv_fp8", False),
                                    page_size=page_size if kw.get("paged") else None)
            row[f"{name}_replay_ms"], row[f"{name}_replay_ms_q20"], row[f"{name}_replay_ms_q80"] = med, lo, hi
        if kw.get("paged"):  # what a shared prompt holds: one prefill through row 0, forked to the others
            from ..models.kv_cache import PagedKVCache

            pc = PagedKVCache(model, B, page_size=page_size)
            model.forward_cached(x[:1], pc.row(0))
            pc.fork(0)
            row["shared_prompt_pages_in_use"], row["paged_pool_pages"] = pc.pages_in_use, pc.num_pages
            row["shared_prompt_mbytes"] = pc.pages_in_use / pc.num_pages * (pc.k.numel() + pc.v.numel()) * 2 / 2**20
            row["unshared_prompt_pages"] = B * -(-prompt // page_size)
            row["dense_cache_mbytes"] = 2.0 * len(model.layers) * B * pc.num_heads * ctx * pc.d_head * 2 / 2**20
            del pc
        if kw.get("kv_fp8") and "kv8_cache_mbytes" not in row:
            from ..models.kv_cache import KVCache

            attn = model.layers[0].attn
            dims = (len(model.layers), attn.num_heads, attn.d_k)
            sizes = [KVCache(dims, 1, max_len=1, device="cuda", dtype=torch.bfloat16, fp8=f).nbytes for f in (False, True)]
            row["kv_cache_mbytes"], row["kv8_cache_mbytes"] = (s * B * ctx / 2**20 for s in sizes)
            row["kv8_cache_vs_bf16"] = sizes[1] / sizes[0]
    if "cached_s" in row and "uncached_s" in row:
        row["speedup"] = row["uncached_s"] / row["cached_s"]
    if "cached_s" in row and "cached_graph_s" in row:
        row["graph_speedup_vs_cached"] = row["cached_s"] / row["cached_graph_s"]
    if "cached_graph_s" in row and "cached_graph_fp8_s" in row:
        row["fp8_speedup_vs_graph"] = row["cached_graph_s"] / row["cached_graph_fp8_s"]
        row["fp8_replay_vs_graph"] = row["cached_graph_fp8_replay_ms"] / row["cached_graph_replay_ms"]
    for base in ("cached_graph", "cached_graph_fp8"):  # the MXFP4 step against the 16-bit and the FP8 step of this run
        if "cached_graph_fp4_s" in row and f"{base}_s" in row:
            tag = "graph" if base == "cached_graph" else "fp8"
            row[f"fp4_speedup_vs_{tag}"] = row[f"{base}_s"] / row["cached_graph_fp4_s"]
            row[f"fp4_replay_vs_{tag}"] = row["cached_graph_fp4_replay_ms"] / row[f"{base}_replay_ms"]
            row[f"fp4_replay_verdict_vs_{tag}"] = (
                "faster" if row["cached_graph_fp4_replay_ms_q80"] < row[f"{base}_replay_ms_q20"] else
                "slower" if row["cached_graph_fp4_replay_ms_q20"] > row[f"{base}_replay_ms_q80"] else "same")
    for name, base in (("cached_graph_sample", "cached_graph"), ("cached_graph_fp8_sample", "cached_graph_fp8")):
        if f"{name}_s" in row and f"{base}_s" in row:
            row[f"{name}_vs_{base[7:]}"] = row[f"{name}_s"] / row[f"{base}_s"]  # below 1: sampling in the graph is faster
            row[f"{name}_saves_ms_per_step"] = row[f"{base}_ms_per_step"] - row[f"{name}_ms_per_step"]
            if runs > 1:  # faster / slower only when every run of one side beats every run of the other
                a, b = row[f"{name}_ms_per_step_runs"], row[f"{base}_ms_per_step_runs"]
                row[f"{name}_verdict"] = "faster" if max(a) < min(b) else "slower" if min(a) > max(b) else "same"
    for name in ("cached_graph_kv8", "cached_graph_fp8_kv8", "cached_graph_paged"):
        if "cached_graph_s" in row and f"{name}_s" in row:
            row[f"{name}_speedup_vs_graph"] = row["cached_graph_s"] / row[f"{name}_s"]
            row[f"{name}_replay_vs_graph"] = row[f"{name}_replay_ms"] / row["cached_graph_replay_ms"]
            row[f"{name}_replay_verdict"] = (
                "faster" if row[f"{name}_replay_ms_q80"] < row["cached_graph_replay_ms_q20"] else
                "slower" if row[f"{name}_replay_ms_q20"] > row["cached_graph_replay_ms_q80"] else "same")
    del model
    torch.cuda.empty_cache()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["25x64", "32x80"], help="HxD head layouts")
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 8, 64])
    ap.add_argument("--kv-len", nargs="+", type=int, default=[512, 4096, 16384])
    ap.add_argument("--rep", type=int, default=50)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-sweep", action="store_true", help="skip the forced split counts")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--model", default="xl")
    ap.add_argument("--skinny", action="store_true", help="the skinny-M GEMM table (xl and 2.7b projections)")
    ap.add_argument("--fp8", action="store_true", help="with --skinny: add the FP8 weight-only kernel to every row")
    ap.add_argument("--fp4", action="store_true", help="with --skinny: add the MXFP4 weight-only kernel to every row")
    ap.add_argument("--kv-fp8", action="store_true",
                    help="add the FP8 KV cache kernels to every kernel / chunk row, and the end-to-end point "
                         "context 4096, B 8, prompt 2048 + 512")
    ap.add_argument("--sample", action="store_true",
                    help="the fused sampler table (sample_logits against the eager sampling of generate), and three "
                         "timed runs per end-to-end arm")
    ap.add_argument("--paged", action="store_true",
                    help="add the paged decode-attention kernel to every kernel row (pages in a seeded random "
                         "permutation, the contiguous kernel re-measured alternating)")
    ap.add_argument("--page-size", nargs="+", type=int, default=[16, 64, 256],
                    help="with --paged: the page sizes of the kernel rows; the first is the graph+paged arm's")
    ap.add_argument("--chunk", action="store_true",
                    help="the multi-token tables: decode_attention_chunk rows instead of the single-token sweep, and "
                         "(with --arms verify) the replayed n-token step; no generate arms")
    ap.add_argument("--arms", nargs="+", default=["cached", "uncached", "graph"], choices=sorted(ARMS) + ["verify"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench.decode needs a GPU")
    if not ops.load_ext():
        raise SystemExit(ops.load_error())
    out = dict(hbm_achievable_gbs=HBM_ACHIEVABLE_GBS, kernel=[], skinny=[], e2e=[])
    if a.chunk:
        from ..utils.gpu_monitor import GpuSampler

        out.update(chunk=[], verify=[])
        with GpuSampler(torch.device("cuda", torch.cuda.current_device())) as sampler:  # the box's clocks
            if not a.no_kernel:
                for shape in a.shapes:
                    H, d = (int(s) for s in shape.split("x"))
                    for B in a.batch:
                        for kv in a.kv_len:
                            for n in CHUNK_N:
                                r = chunk_row(B, H, d, kv, n, rep=a.rep, kv_fp8=a.kv_fp8)
                                out["chunk"].append(r)
                                print(json.dumps(r), flush=True)
            if "verify" in a.arms:
                for r in verify_rows(a.model, rep=a.rep):
                    out["verify"].append(r)
                    print(json.dumps(r), flush=True)
        out["gpu_clocks"] = sampler.summary()
        print(json.dumps(dict(gpu_clocks=out["gpu_clocks"])), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return out
    if "verify" in a.arms:
        raise SystemExit("--arms verify needs --chunk")
    if not a.no_kernel:
        for shape in a.shapes:
            H, d = (int(s) for s in shape.split("x"))
            for B in a.batch:
                for n in a.kv_len:
                    r = kernel_row(B, H, d, n, rep=a.rep, sweep=not a.no_sweep, kv_fp8=a.kv_fp8,
                                   paged=tuple(a.page_size) if a.paged else ())
                    out["kernel"].append(r)
                    print(json.dumps(r), flush=True)
    if a.skinny:
        for size in ("xl", "2.7b"):
            for name, N, K in skinny_shapes(size):
                for M in SKINNY_M:
                    r = skinny_row(size, name, M, N, K, rep=a.rep, fp8=a.fp8, fp4=a.fp4)
                    out["skinny"].append(r)
                    print(json.dumps(r), flush=True)
    if a.sample:
        out["sample"] = []
        for B in SAMPLE_B:
            for V in SAMPLE_V:
                for k in SAMPLE_K:
                    r = sample_row(B, V, k, rep=a.rep)
                    out["sample"].append(r)
                    print(json.dumps(r), flush=True)
    if not a.no_e2e:
        points = [(512, 1, 128, 384), (512, 8, 128, 384), (4096, 1, 2048, 512)]
        if a.kv_fp8:
            points.append((4096, 8, 2048, 512))  # the cache is the larger stream of a step
        for ctx, B, prompt, new in points:
            r = e2e_row(a.model, ctx, B, prompt, new, arms=a.arms, runs=3 if a.sample else 1,
                        page_size=a.page_size[0] if a.paged and len(a.page_size) == 1 else 64)
            out["e2e"].append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
