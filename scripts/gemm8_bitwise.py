"""Dump (or compare) gemm8's results on the XL problems of every epilogue kind and the vocabulary
head, on fixed inputs, to check two builds bit for bit:
    CS336_LIB=.../variants/base/libcs336_hip.so python scripts/gemm8_bitwise.py dump /tmp/g8.pt
    python scripts/gemm8_bitwise.py check /tmp/g8.pt      (exit status 1 on a difference)
One seed, random operands, 52,224 tokens (a token count as a third argument for another one). The
outputs together are 5.7 GB, so the dump holds one 64-bit digest per output row instead of the
rows: the sum over the row of (bf16 bit pattern as an unsigned 16-bit integer) x (an odd 64-bit
multiplier per column), modulo 2^64. One differing bit pattern in a row always changes its digest
(an odd multiple of a non-zero 16-bit difference is non-zero modulo 2^64); the check counts
differing rows."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, F, V, SEQ, DH = 1600, 6400, 10000, 512, 64
# name, N, K, epi
PROBLEMS = [
    ("qkv fwd + rope", 3 * D, D, 3), ("o fwd", D, D, 0), ("w13 fwd + swiglu", 2 * F, D, 1), ("w2 fwd", D, F, 0),
    ("w2 dX + swiglu bwd", F, D, 2), ("w13 dX", D, 2 * F, 0), ("qkv dX", D, 3 * D, 0), ("lm fwd", V, D, 0),
    ("lm dX", D, V, 0),
]


def digest(t):
    """(rows,) int64: per-row digest of a 2-D bf16 tensor's bit patterns."""
    rows, cols = t.shape
    w = (torch.arange(cols, device=t.device, dtype=torch.int64) * 0x1E3779B97F4A7C15 + 0x2545F4914F6CDD1D) | 1
    out = torch.empty(rows, device=t.device, dtype=torch.int64)
    for r0 in range(0, rows, 4096):
        bits = t[r0: r0 + 4096].contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        out[r0: r0 + 4096] = (bits * w).sum(1)
    return out.cpu()


def run(tokens):
    from cs336_systems import ops

    assert ops.load_ext(), ops.load_error()
    cs = torch.ops.cs336
    res = {}
    g = torch.Generator(device="cuda").manual_seed(20261)
    bf = torch.bfloat16
    for name, N, K, epi in PROBLEMS:
        a = torch.randn(tokens, K, device="cuda", generator=g).to(bf)
        b = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(bf)
        if epi == 1:
            half = N // 2
            y = torch.empty(tokens, N, device="cuda", dtype=bf)
            h = torch.empty(tokens, half, device="cuda", dtype=bf)
            cs.gemm8(a, b, y, 1, 0, h, None, half)
            outs = {"y": y, "h": h}
        elif epi == 2:
            y = (torch.randn(tokens, 2 * N, device="cuda", generator=g) * 2).to(bf)
            dab = torch.empty(tokens, 2 * N, device="cuda", dtype=bf)
            cs.gemm8(a, b, dab, 2, 0, None, y, N)
            outs = {"da|db": dab}
        elif epi == 3:
            ang = torch.rand(SEQ, DH // 2, device="cuda", generator=g) * 6.2831853
            c = torch.empty(tokens, N, device="cuda", dtype=bf)
            cs.gemm8_rope(a, b, c, ang.cos().contiguous(), ang.sin().contiguous(), None, SEQ, 2 * D, DH)
            outs = {"c": c}
        else:
            c = torch.empty(tokens, N, device="cuda", dtype=bf)
            cs.gemm8(a, b, c, 0, 0, None, None, 0)
            outs = {"c": c}
        torch.cuda.synchronize()
        for k, v in outs.items():
            res[f"{name} [{k}]"] = digest(v)
        del a, b, outs
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    res = run(int(sys.argv[3]) if len(sys.argv) > 3 else 52224)
    if mode == "dump":
        torch.save(res, path)
        print(f"dumped {len(res)} outputs")
    else:
        ref = torch.load(path, weights_only=True)
        bad = 0
        for key, got in res.items():
            n = int((got != ref[key]).sum())
            bad += n > 0
            print(f"{key}: {'same' if not n else '%d of %d rows differ' % (n, got.numel())}")
        print(f"{len(res)} outputs, {bad} differing")
        print("BITWISE " + ("OK" if not bad else "DIFF"))
        sys.exit(1 if bad else 0)
