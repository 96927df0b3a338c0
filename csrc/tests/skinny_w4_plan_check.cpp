// Plan invariants of the skinny-M decode GEMM for the MXFP4 weight format (gemm/skinny_plan.h), host code
// only, built with the ordinary host compiler by tests/test_skinny_w4_plan.py. A wrong plan is a kernel
// launched with waves that own no register set, or a grid that leaves tiles out. For every N up to 8300
// and the vocabulary head, and every K that is a multiple of 32 up to 10240:
//   * W tiles per wave: 4 / 2 / 1 at >= 512 / >= 256 / fewer tiles, as in the other formats;
//   * waves: 1 .. MAXW (4 / 8 / 8), at most one per full register set of K (a set is U = 2 / 2 / 4
//     k-blocks of 128 k, written out here as the kernel's three configurations have them);
//   * workgroups cover the tiles exactly;
// and a table pins the plans of the models' shapes.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../gemm/skinny_plan.h"

using namespace cs336;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
    }                                             \
  } while (0)

int main() {
  static_assert(skinny_k_per_load(SkinnyFormat::MXFP4) == 32 && skinny_kblock(SkinnyFormat::MXFP4) == 128, "one MX block per load");
  static_assert(skinny_u(SkinnyFormat::MXFP4, 4) == 2 && skinny_u(SkinnyFormat::MXFP4, 2) == 2 && skinny_u(SkinnyFormat::MXFP4, 1) == 4, "U");
  // the other formats keep the values csrc/tests/host_checks.cpp records
  static_assert(skinny_u(SkinnyFormat::W16, 1) == 8 && skinny_u(SkinnyFormat::E4M3, 1) == 8 && skinny_u(SkinnyFormat::W16, 4) == 4 &&
                    skinny_u(SkinnyFormat::E4M3, 2) == 4,
                "U of the 16-bit and FP8 formats");
  std::vector<int> ns;
  for (int n = 1; n <= 8300; ++n) ns.push_back(n);
  ns.push_back(50257);
  long checked = 0;
  const SkinnyFormat f = SkinnyFormat::MXFP4;
  for (int N : ns)
    for (int K = 32; K <= 10240; K += 32) {
      int tn = -1, waves = -1;
      gemm_skinny_plan(f, N, K, tn, waves);
      const int tiles = (N + 15) / 16;
      CHECK(tn == (tiles >= 512 ? 4 : tiles >= 256 ? 2 : 1), "mxfp4 plan N=%d K=%d: tn %d for %d tiles", N, K, tn, tiles);
      if (tn != 1 && tn != 2 && tn != 4) continue;
      const int u = tn == 1 ? 4 : 2;
      CHECK(waves >= 1 && waves <= (tn == 4 ? 4 : 8), "mxfp4 plan N=%d K=%d: %d waves at tn %d", N, K, waves, tn);
      CHECK(waves <= std::max(1, K / (128 * u)), "mxfp4 plan N=%d K=%d: %d waves for %d full sets", N, K, waves, K / (128 * u));
      const int wgs = skinny_workgroups(N, tn);
      CHECK(wgs * tn >= tiles && (wgs - 1) * tn < tiles, "mxfp4 plan N=%d: %d workgroups x %d for %d tiles", N, wgs, tn, tiles);
      ++checked;
    }
  // (N, K) -> (tn, waves): a set covers the k of the FP8 format's, so these are the FP8 plans of host_checks.cpp
  const int table[][4] = {{48, 8256, 1, 8},   {4100, 1632, 2, 6},  {4800, 1600, 2, 6}, {1600, 1600, 1, 3}, {12800, 1600, 4, 4},
                          {50257, 1600, 4, 3}, {50257, 128, 4, 1},  {2560, 10240, 1, 8}, {8177, 512, 4, 2}, {8176, 512, 2, 2},
                          {1, 32, 1, 1},      {6400, 1600, 2, 6},  {1600, 6400, 1, 8}, {4096, 256, 2, 1}, {4081, 1024, 2, 4},
                          {4080, 1024, 1, 2}, {17, 96, 1, 1}};
  for (const auto& r : table) {
    int tn = -1, waves = -1;
    gemm_skinny_plan(f, r[0], r[1], tn, waves);
    CHECK(tn == r[2] && waves == r[3], "mxfp4 plan (%d, %d): (%d, %d), recorded (%d, %d)", r[0], r[1], tn, waves, r[2], r[3]);
  }
  std::printf("mxfp4 skinny plan: %ld (N, K) checked\n", checked);
  if (failures) {
    std::fprintf(stderr, "%d plan checks failed\n", failures);
    return 1;
  }
  std::printf("mxfp4 plan checks passed\n");
  return 0;
}
