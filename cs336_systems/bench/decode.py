"""Decode-attention kernel sweep and end-to-end generation with / without the KV cache.

Kernel sweep: ``ops.decode_attention`` (``csrc/flash_attn/fa_decode.hip``) timed with the HIP-event
``do_bench`` (L2 + Infinity Cache flushed before every call) at (H, d) in {(25, 64), (32, 80)} --
the xl and 2.7b head layouts -- x B x kv_len, bf16: the default split count against ``splits=1`` and
a sweep of forced split counts, in us and in GB/s of K+V bytes read, beside the 6.3 TB/s achievable
HBM rate of the MI355X and ``ops.naive_attention`` on the same tensors (q as (B, H, 1, d), the
cache sliced to kv_len), the only way to compute a decode step without the kernel.

End to end: tokens/s of ``generate`` with ``use_cache=True`` against ``use_cache=False`` (a full
forward over the window per token), model ``xl`` held in bf16.

    python -m cs336_systems.bench.decode --json profiles/decode_attention.json
    python -m cs336_systems.bench.decode --no-e2e --batch 8 --kv-len 4096
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


def e2e_row(model_size: str, ctx: int, B: int, prompt: int, new: int, arms=(True, False)) -> dict:
    from ..models import build_model

    torch.manual_seed(0)
    model = build_model(model_size, ctx, device="cuda").to(torch.bfloat16).eval()
    x = torch.randint(0, model.vocab_size, (B, prompt), device="cuda")
    row = dict(model=model_size, context_length=ctx, B=B, prompt=prompt, new_tokens=new, dtype="bf16")
    for use_cache in arms:
        model.generate(x, 4, top_k=1, use_cache=use_cache)  # warm-up: GEMM selection, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(x, new, top_k=1, use_cache=use_cache)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert out.shape == (B, new)
        name = "cached" if use_cache else "uncached"
        row[f"{name}_s"] = dt
        row[f"{name}_tok_s"] = B * new / dt
        row[f"{name}_ms_per_step"] = dt / new * 1e3
    if "cached_s" in row and "uncached_s" in row:
        row["speedup"] = row["uncached_s"] / row["cached_s"]
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
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench.decode needs a GPU")
    if not ops.load_ext():
        raise SystemExit(ops.load_error())
    out = dict(hbm_achievable_gbs=HBM_ACHIEVABLE_GBS, kernel=[], e2e=[])
    if not a.no_kernel:
        for shape in a.shapes:
            H, d = (int(s) for s in shape.split("x"))
            for B in a.batch:
                for n in a.kv_len:
                    r = kernel_row(B, H, d, n, rep=a.rep, sweep=not a.no_sweep)
                    out["kernel"].append(r)
                    print(json.dumps(r), flush=True)
    if not a.no_e2e:
        for ctx, B, prompt, new in ((512, 1, 128, 384), (512, 8, 128, 384), (4096, 1, 2048, 512)):
            r = e2e_row(a.model, ctx, B, prompt, new)
            out["e2e"].append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
