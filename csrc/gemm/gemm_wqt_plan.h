// Launch plan of the weight-only FP8 / MXFP4 tile GEMM for more than 128 rows (gemm_wqt.hip), host code
// only: the kernel's dispatch and the bindings call it. A function of (format, M, N, K) alone: no tuning
// table, no device query.
//
// The kernel's units. A workgroup of 4 waves owns a BM x BN tile of out and walks K in k-tiles of 64. Per
// k-tile it stages BM x 64 of x and the CONVERTED BN x 64 of W in LDS as 16-bit rows of 128 bytes (8 chunks
// of 16 B, chunk index XOR-ed by the row: fa_common.h's swizzle for 128-byte rows), two buffers of each.
// A converted W element then feeds BM rows of x: the conversions per MFMA, which bound gemm_wq at 128
// rows, fall by BM / 16.
//
// Tile. (128, 128), (128, 64) or (64, 64), the first in that order with at least one workgroup for each of
// the 256 CUs, else the last. BN shrinks before BM: a workgroup converts its own BN x K of W, so the
// launch converts (and reads from L2) W ceil(M / BM) times, while x, the operand BN multiplies, needs no
// conversion. At M 256 x N 1600 the 128 x 128 tiles are 26 workgroups; 64 x 64 are 100.
//
// Split K. While the workgroups are still fewer than the CUs and every split keeps at least 4 k-tiles (so
// its two-buffer pipeline runs), the k-tiles are split in two again, up to 8 ways: split z of S owns
// k-tiles [T z / S, T (z + 1) / S). The splits are grid.z; each writes its fp32 partial tile to a
// workspace (S x M x N rounded up to 4 columns) with plain stores, and a second launch adds the S partials
// of an element in the order z = 0 .. S - 1, applies the FP8 row scale and rounds once. No atomic of any
// kind: one summation order per (M, N, K). M 129 x N 1600 x K 1600: 75 tiles of 64 x 64, S = 4, 300
// workgroups, 3.3 MB of partials beside W's 2.6 MB.
//
// Budget. LDS is 2 buffers x (BM + BN) x 128 B: 64 KB at 128 x 128, so two workgroups fit in a CU's
// 160 KB; 48 KB and 32 KB for the smaller tiles. Registers: the accumulator is (BM / 64) x (BN / 64) MFMA
// blocks of 16 fp32 per wave (64 at 128 x 128), the staged k-tile is BM / 32 x chunks and at most 2 W
// loads per thread (24 VGPRs), the fragments of a k-step 16: every kernel stays at or below 144 VGPRs (3
// waves per SIMD, so LDS and not registers sets the 2 workgroups per CU) with 0 B scratch;
// tests/test_gemm_wqt_resources.py holds the LDS, register and scratch figures.
#pragma once

#include <stdint.h>

#include "skinny_plan.h"

namespace cs336 {

constexpr int kWqtMinM = 129;
constexpr int kWqtKTile = 64;
constexpr int kWqtCus = 256;
constexpr int kWqtMaxSplit = 8, kWqtMinSplitKTiles = 4;

struct WqtPlan {
  int bm, bn, split;
};

constexpr int64_t wqt_tiles(int64_t M, int64_t N, int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

inline WqtPlan gemm_wqt_plan(SkinnyFormat, int64_t M, int64_t N, int64_t K) {
  WqtPlan p{64, 64, 1};
  if (wqt_tiles(M, N, 128, 128) >= kWqtCus) p = WqtPlan{128, 128, 1};
  else if (wqt_tiles(M, N, 128, 64) >= kWqtCus) p = WqtPlan{128, 64, 1};
  const int64_t tiles = wqt_tiles(M, N, p.bm, p.bn), ktiles = (K + kWqtKTile - 1) / kWqtKTile;
  while (p.split < kWqtMaxSplit && tiles * p.split < kWqtCus && ktiles / (2 * p.split) >= kWqtMinSplitKTiles) p.split *= 2;
  return p;
}

// dynamic LDS of a launch: two buffers of the x tile and of the converted W tile
constexpr int wqt_lds_bytes(int bm, int bn) { return 2 * (bm + bn) * kWqtKTile * 2; }
// row stride (floats) and size of the split launch's workspace; 0 without a split
constexpr int64_t wqt_ws_ld(int64_t N) { return (N + 3) / 4 * 4; }
inline int64_t wqt_workspace_floats(SkinnyFormat f, int64_t M, int64_t N, int64_t K) {
  const WqtPlan p = gemm_wqt_plan(f, M, N, K);
  return p.split > 1 ? p.split * M * wqt_ws_ld(N) : 0;
}

}  // namespace cs336
