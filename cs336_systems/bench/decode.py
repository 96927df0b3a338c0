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
HBM rate, with ``torch.mm`` on the same operands alongside.

End to end: tokens/s of ``generate`` with ``use_cache=True`` against ``use_cache=False`` (a full
forward over the window per token) and against ``use_cache=True, graph=True`` (the cached step
replayed from a HIP graph over the skinny-M kernel), model ``xl`` held in bf16. ``--arms`` picks the
arms (the uncached one takes minutes at context 4096).

    python -m cs336_systems.bench.decode --json profiles/decode_attention.json
    python -m cs336_systems.bench.decode --no-e2e --batch 8 --kv-len 4096
    python -m cs336_systems.bench.decode --no-kernel --skinny --arms cached graph --json profiles/decode_graph.json
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


def kernel_row(B: int, H: int, d: int, kv_len: int, warmup: int = 10, rep: int = 50, sweep: bool = True) -> dict:
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
    del q, k, v
    torch.cuda.empty_cache()
    return row


SKINNY_M = (1, 8, 16)
LM_HEAD_VOCAB = 50257  # the GPT-2 vocabulary: N is not a multiple of 16 (nor of 4)


def skinny_shapes(model_size: str) -> list[tuple[str, int, int]]:
    """(name, N, K) of the five projections of a decode step."""
    from ..models import get_model_config

    c = get_model_config(model_size)
    d, f = c["d_model"], c["d_ff"]
    return [("qkv", 3 * d, d), ("o", d, d), ("w1|w3", 2 * f, d), ("w2", d, f), ("lm_head", LM_HEAD_VOCAB, d)]


def skinny_row(model_size: str, name: str, M: int, N: int, K: int, warmup: int = 10, rep: int = 50) -> dict:
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
    del x, w, out
    torch.cuda.empty_cache()
    return row


ARMS = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "graph": dict(use_cache=True, graph=True)}


def e2e_row(model_size: str, ctx: int, B: int, prompt: int, new: int, arms=("cached", "uncached", "graph")) -> dict:
    from ..models import build_model

    torch.manual_seed(0)
    model = build_model(model_size, ctx, device="cuda").to(torch.bfloat16).eval()
    x = torch.randint(0, model.vocab_size, (B, prompt), device="cuda")
    row = dict(model=model_size, context_length=ctx, B=B, prompt=prompt, new_tokens=new, dtype="bf16")
    for arm in arms:
        kw = ARMS[arm]
        model.generate(x, 4, top_k=1, **kw)  # warm-up: GEMM selection, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(x, new, top_k=1, **kw)  # (the graph arm's time includes its capture)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert out.shape == (B, new)
        name = "cached_graph" if arm == "graph" else arm
        row[f"{name}_s"] = dt
        row[f"{name}_tok_s"] = B * new / dt
        row[f"{name}_ms_per_step"] = dt / new * 1e3
    if "cached_s" in row and "uncached_s" in row:
        row["speedup"] = row["uncached_s"] / row["cached_s"]
    if "cached_s" in row and "cached_graph_s" in row:
        row["graph_speedup_vs_cached"] = row["cached_s"] / row["cached_graph_s"]
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
    ap.add_argument("--arms", nargs="+", default=["cached", "uncached", "graph"], choices=sorted(ARMS))
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench.decode needs a GPU")
    if not ops.load_ext():
        raise SystemExit(ops.load_error())
    out = dict(hbm_achievable_gbs=HBM_ACHIEVABLE_GBS, kernel=[], skinny=[], e2e=[])
    if not a.no_kernel:
        for shape in a.shapes:
            H, d = (int(s) for s in shape.split("x"))
            for B in a.batch:
                for n in a.kv_len:
                    r = kernel_row(B, H, d, n, rep=a.rep, sweep=not a.no_sweep)
                    out["kernel"].append(r)
                    print(json.dumps(r), flush=True)
    if a.skinny:
        for size in ("xl", "2.7b"):
            for name, N, K in skinny_shapes(size):
                for M in SKINNY_M:
                    r = skinny_row(size, name, M, N, K, rep=a.rep)
                    out["skinny"].append(r)
                    print(json.dumps(r), flush=True)
    if not a.no_e2e:
        for ctx, B, prompt, new in ((512, 1, 128, 384), (512, 8, 128, 384), (4096, 1, 2048, 512)):
            r = e2e_row(a.model, ctx, B, prompt, new, arms=a.arms)
            out["e2e"].append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
