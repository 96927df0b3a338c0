"""Where a gemm8w k-tile's time goes, per phase and wave group, from in-kernel stamps (diagnostic
build, -DCS336_G8_STAMP; the companion of scripts/gemm8_stamps.py).

    CS336_BUILD_VARIANT="stamp -DCS336_G8_STAMP=1" python -m cs336_systems._native.build
    CS336_LIB=cs336_systems/_native/variants/stamp/libcs336_hip.so python scripts/gemm8w_stamps.py [--tokens 52224]

For each XL weight-gradient problem with its committed plan (ops.gemm.DW_PLANS: roles and splits;
random operands, three warm launches, then a stamped one) every workgroup stamps four k-tiles in the
middle of its range. Per phase (P0: k 0-31, P1: k 32-63 of the k-tile; the buffer has room for
four) and per wave group (0 leads, 1 runs one barrier behind) the kernel sums three segments,
reported here as cycles per k-tile, median over workgroups:

  work  phase entry -> its reads, DMA issue and counted waits done (lgkmcnt(0) reached)
  wait  from there -> through the barrier before the MFMA cluster (the partner group's cluster ends)
  mma   from there -> through the barrier after the cluster (the partner group's `work` ends)

`work` longer than the partner's cluster (8 x FN MFMAs, about 16 cycles each) shows up as that
phase's `wait` near zero and the partner's `mma` stretched: the matrix core idles for the excess.
Each stamp costs about 40 cycles (three per phase), so read the shares and the differences between
phases, not the k-tile total; the stamped build is never timed against the shipped one.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, N_out (dY columns), K_in (X columns)
PROBLEMS = [("w13 dW", 12800, 1600), ("w2 dW", 1600, 6400), ("qkv dW", 4800, 1600), ("o dW", 1600, 1600)]


def analyse(st: torch.Tensor) -> dict:
    """st: (workgroups, 4, 8) -- per wave group g rows 2g (work[4], wait[4]) and 2g + 1 (mma[4],
    stamped k-tiles, k-tiles, HW_ID, XCC_ID)."""
    s = st.cpu().tolist()
    med = statistics.median
    out: dict = {"workgroups": len(s), "stamped_ktiles": int(med(w[1][4] for w in s)), "ktiles": int(med(w[1][5] for w in s))}
    for g in (0, 1):
        live = [w for w in s if w[2 * g + 1][4] > 0]
        if not live:
            continue
        phases = max((ph + 1 for ph in range(4) if any(w[2 * g][ph] for w in live)), default=0)
        for name, row, col in (("work", 0, 0), ("wait", 0, 4), ("mma", 1, 0)):
            out[f"g{g}_{name}"] = [round(med(w[2 * g + row][col + ph] / w[2 * g + 1][4] for w in live)) for ph in range(phases)]
        out[f"g{g}_ktile"] = round(med(sum(w[2 * g][:8]) + sum(w[2 * g + 1][:4]) for w in live) / out["stamped_ktiles"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=52224)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from cs336_systems import ops
    from cs336_systems.ops import gemm

    assert ops.load_ext(), ops.load_error()
    cs = torch.ops.cs336
    T = args.tokens
    rows = []
    for name, n, k in PROBLEMS:
        g = torch.Generator(device="cuda").manual_seed(n + k)
        dy = (torch.rand(T, n, device="cuda", generator=g) * 2 - 1).bfloat16()
        x = (torch.rand(T, k, device="cuda", generator=g) * 2 - 1).bfloat16()
        trans, sk = gemm.dw_launch_plan(dy, x)
        a, b = (x, dy) if trans else (dy, x)
        M, N = a.shape[1], b.shape[1]
        out = torch.empty((sk, n, k) if sk > 1 else (n, k), device="cuda", dtype=torch.float32)
        wgs = -(-M // 256) * (N // (320 if N % 320 == 0 else 256)) * sk
        st = torch.zeros(4 * wgs, 8, dtype=torch.int64, device="cuda")
        for _ in range(3):
            cs.gemm8w(a, b, out, sk, trans, False, 0)
        torch.cuda.synchronize()
        if not cs.gemm8_stamps(st):
            raise SystemExit("this build writes no stamps: build the CS336_G8_STAMP variant and load it with CS336_LIB")
        cs.gemm8w(a, b, out, sk, trans, False, 0)
        torch.cuda.synchronize()
        cs.gemm8_stamps(None)
        row = {"problem": name, "tokens": T, "M": M, "N": N, "trans": trans, "splits": sk, **analyse(st.view(wgs, 4, 8))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dy, x, out, st
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
