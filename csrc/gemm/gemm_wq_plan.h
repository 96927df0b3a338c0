// Launch plan of the weight-only FP8 / MXFP4 GEMM for 17..128 rows (gemm_wq.hip), host code only: the
// kernel's dispatch and the bindings call it. A function of (format, M, N, K) alone: no tuning table, no
// device query.
//
// The kernel's units. A W load is 16 bytes of one W row: KL = 16 k (e4m3) or 32 k (MXFP4, one MX block). A
// k-block is the 4 loads of a wave's 4 lane groups (64 / 128 k). A slab is the U k-blocks of one W register
// set, and the x slab a workgroup's k-group stages in LDS is 16 MB rows x that k, MB = 2 / 4 / 8 for
// M <= 32 / 64 / 128.
//
// U (wq_u). The slab is held at 16 KB (MXFP4 at MB = 8: 32 KB, one k-block is that large): two buffers of
// two k-groups are then 64 KB, and two workgroups fit in a CU's 160 KB. That makes U = 4 / 2 / 1 (e4m3) and
// 2 / 1 / 1 (MXFP4): the k a set covers shrinks as the rows grow. What hides HBM latency is bytes in flight
// per CU, and at MB = 8 a W load feeds 16 (e4m3) / 32 (MXFP4) MFMAs, so the few loads in flight per wave
// are many MFMA-cycles apart; the waves of a CU (up to 16) supply the rest.
//
// Rows per workgroup (tiles of 16 W rows; wq_tiles_per_wg). Every workgroup reads all of x from L2: over
// the launch that is (N / rows-per-workgroup) x M x K x 2 bytes against W's N x K (e4m3) or N x K x 17/32
// (MXFP4) from HBM, a ratio of 2 M / rows (e4m3) and about 4 M / rows (MXFP4). L2 delivers a small
// multiple of HBM's rate, so the plan keeps the ratio at 4 or below: at least MB / 2 tiles per workgroup
// for e4m3 (16 / 32 / 64 rows) and MB tiles for MXFP4 (32 / 64 / 128 rows). Above that floor more rows per
// workgroup only pay while there are workgroups to spare: the count doubles (up to 8 tiles) while at least
// 512 workgroups, two for each of the 256 CUs, remain. On the xl / 2.7b projections only the vocabulary
// head (3142 tiles) has that many. Small N is not special-cased: waves whose tiles lie beyond N work on
// clamped rows and store nothing.
//
// Tiles per workgroup -> (TN, RW): 1 -> (1, 1), 2 -> (1, 2), 4 -> (2, 2), 8 -> (2, 4). Row-waves come first
// (more waves to overlap loads with MFMAs), then TN = 2, where one B fragment read from LDS serves two W
// tiles and halves the LDS traffic per MFMA.
//
// KG. Two k-groups when the format and MB leave LDS for them (wq_kgmax) and K has at least 4 slabs, so that
// each group's pipeline runs two or more slabs; else one. Partials are summed through LDS in group order.
#pragma once

#include "skinny_plan.h"

namespace cs336 {

constexpr int kWqMinM = 17, kWqMaxM = 128;

constexpr int wq_mb(int M) { return M <= 32 ? 2 : (M <= 64 ? 4 : 8); }
// k-blocks per W register set (= per x slab)
constexpr int wq_u(SkinnyFormat f, int mb) { return f == SkinnyFormat::MXFP4 ? (mb == 2 ? 2 : 1) : 8 / mb; }
// k and bytes of one x slab
constexpr int wq_slab_k(SkinnyFormat f, int mb) { return skinny_kblock(f) * wq_u(f, mb); }
constexpr int wq_slab_bytes(SkinnyFormat f, int mb) { return 16 * mb * wq_slab_k(f, mb) * 2; }
// most k-groups: two buffers per group within 64 KB
constexpr int wq_kgmax(SkinnyFormat f, int mb) { return 65536 / (2 * wq_slab_bytes(f, mb)) >= 2 ? 2 : 1; }
// fewest 16-row W tiles per workgroup: x re-read from L2 at most 4x W's bytes
constexpr int wq_min_tiles(SkinnyFormat f, int mb) { return f == SkinnyFormat::MXFP4 ? mb : mb / 2; }
constexpr int kWqSpareWorkgroups = 512;

inline int wq_tiles_per_wg(SkinnyFormat f, int M, int N) {
  const int tiles = (N + 15) / 16;
  int tpw = wq_min_tiles(f, wq_mb(M));
  while (tpw < 8 && tiles / (2 * tpw) >= kWqSpareWorkgroups) tpw *= 2;
  return tpw;
}
constexpr int wq_tn(int tpw) { return tpw >= 4 ? 2 : 1; }
constexpr int wq_rw(int tpw) { return tpw / wq_tn(tpw); }
constexpr int wq_workgroups(int N, int tpw) { return ((N + 15) / 16 + tpw - 1) / tpw; }

// row-waves, k-groups and W tiles per wave of the launch for (M, N, K)
inline void gemm_wq_plan(SkinnyFormat f, int M, int N, int K, int& rw, int& kg, int& tn) {
  const int mb = wq_mb(M), tpw = wq_tiles_per_wg(f, M, N);
  tn = wq_tn(tpw);
  rw = wq_rw(tpw);
  const int slabs = (K + wq_slab_k(f, mb) - 1) / wq_slab_k(f, mb);
  kg = wq_kgmax(f, mb) >= 2 && slabs >= 4 ? 2 : 1;
}

// dynamic LDS of a launch: two slab buffers per k-group; the k-groups' partial sums reuse it
constexpr int wq_lds_bytes(SkinnyFormat f, int mb, int kg) { return 2 * kg * wq_slab_bytes(f, mb); }

}  // namespace cs336
