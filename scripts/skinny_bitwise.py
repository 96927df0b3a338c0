"""Dump (or compare) the outputs of ``cs336::gemm_skinny`` and ``cs336::gemm_skinny_w8`` on fixed inputs,
to check two builds bitwise (both kernels are deterministic: no atomics, sums in wave order):
    CS336_LIB=.../variants/base/libcs336_hip.so python scripts/skinny_bitwise.py dump /tmp/sk.pt
    python scripts/skinny_bitwise.py check /tmp/sk.pt      (exit status 1 on a difference)
Shapes: the ``PATHS`` of ``tests/test_skinny_gemm_gpu.py`` and ``tests/test_skinny_w8_gpu.py`` (every tile
count per wave, wave count and tail) plus (50257, 64) and (17, 48), at M 1 / 3 / 16 in bf16 and fp16,
one seed; the FP8 op takes those with K % 16 == 0. The check compares bit patterns with torch.equal."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(48, 8232), (4100, 1608), (4100, 4104), (8200, 1608), (8200, 4104),
          (48, 8240), (4100, 1616), (4100, 4112), (8200, 1616), (8200, 4112), (50257, 64), (17, 48)]
MS = (1, 3, 16)


def run():
    from cs336_systems import ops
    from cs336_systems.ops import _ext

    assert ops.load_ext(), ops.load_error()
    hip = _ext.ops()
    out = {}
    for dt in (torch.bfloat16, torch.float16):
        for n, k in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(20261 + 31 * n + k)
            w = torch.randn(n, k, device="cuda", generator=g)
            e = torch.randint(-6, 7, (n, 1), device="cuda", generator=g)
            wq, scale = ops.quantize_fp8_rows(w * torch.exp2(e.float()))
            w = w.to(dt)
            for m in MS:
                x = torch.randn(m, k, device="cuda", generator=g).to(dt)
                y = torch.empty(m, n, device="cuda", dtype=dt)
                hip.gemm_skinny(x, w, y)
                out[f"gemm_skinny {dt} M {m} N {n} K {k}"] = y.cpu()
                if k % 16 == 0:
                    y = torch.empty(m, n, device="cuda", dtype=dt)
                    hip.gemm_skinny_w8(x, wq, scale, y)
                    out[f"gemm_skinny_w8 {dt} M {m} N {n} K {k}"] = y.cpu()
    return out


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    res = run()
    if mode == "dump":
        torch.save(res, path)
        print(f"dumped {len(res)} outputs")
    else:
        ref = torch.load(path, weights_only=True)
        assert set(ref) == set(res), "the dump holds other problems"
        bad = 0
        for key, got in res.items():
            same = torch.equal(got.view(torch.int16), ref[key].view(torch.int16))
            bad += not same
            if not same:
                print(f"{key}: max |diff| {(got.float() - ref[key].float()).abs().max().item():.3g}")
        print(f"{len(res)} outputs, {bad} differing")
        print("BITWISE " + ("OK" if not bad else "DIFF"))
        sys.exit(1 if bad else 0)
