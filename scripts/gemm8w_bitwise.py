"""Dump (or compare) the four XL weight gradients as the step computes them (ops.gemm.mm_dw: gemm8w
with the committed plan, slab reduction included) on fixed inputs, to check two builds bitwise:
    CS336_LIB=.../variants/base/libcs336_hip.so python scripts/gemm8w_bitwise.py dump /tmp/dw.pt
    python scripts/gemm8w_bitwise.py check /tmp/dw.pt      (exit status 1 on a difference)
One seed, 52,224 tokens (a token count as a third argument for another one); the dump holds the fp32
results themselves (165 MB), the check compares their bit patterns with torch.equal."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, N_out (dY columns), K_in (X columns)
PROBLEMS = [("w13 dW", 12800, 1600), ("w2 dW", 1600, 6400), ("qkv dW", 4800, 1600), ("o dW", 1600, 1600)]


def run(tokens):
    from cs336_systems import ops
    from cs336_systems.ops import gemm

    assert ops.load_ext(), ops.load_error()
    out = {}
    g = torch.Generator(device="cuda").manual_seed(20260)
    for name, n, k in PROBLEMS:
        dy = torch.randn(tokens, n, device="cuda", generator=g).bfloat16()
        x = torch.randn(tokens, k, device="cuda", generator=g).bfloat16()
        out[f"{name} {gemm.dw_launch_plan(dy, x)}"] = gemm.mm_dw(dy, x).cpu()
        del dy, x
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    res = run(int(sys.argv[3]) if len(sys.argv) > 3 else 52224)
    if mode == "dump":
        torch.save(res, path)
        print(f"dumped {len(res)} problems")
    else:
        ref = torch.load(path, weights_only=True)
        bad = 0
        for key, got in res.items():
            same = torch.equal(got.view(torch.int32), ref[key].view(torch.int32))
            bad += not same
            print(f"{key}: {'same' if same else 'max |diff| %.3g' % (got - ref[key]).abs().max().item()}")
        print(f"{len(res)} problems, {bad} differing")
        print("BITWISE " + ("OK" if not bad else "DIFF"))
        sys.exit(1 if bad else 0)
