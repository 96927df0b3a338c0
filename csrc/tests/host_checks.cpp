// Host-side checks of the index math the kernels rely on, built with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code only (scripts/sanitize_host.sh; GPU sanitizers are not
// available on this pool). A wrong mapping here is a silent wrong result or an out-of-bounds access
// on the GPU, so each property is checked exhaustively over the shapes that matter:
//
//  * tile_order / xcd_remap (fa_common.h): every causal / non-causal FA2 grid maps block ids to
//    (batch*head, tile level) BIJECTIVELY, for every head-group size the host can pick;
//  * tile_of_block (gemm/gemm_common.h): the grouped tile order of the three MFMA GEMM kernels maps
//    the block ids of a grid of tiles_m x tiles_n workgroups onto its tiles BIJECTIVELY;
//  * swz / lds_off: the XOR-swizzled LDS images keep every 16-B chunk of a row inside the row and
//    the row-fragment (ds_read_b128) and transposed (ds_read_b64_tr_b16) reads bank-conflict free
//    for every row width the kernels instantiate (64, 128, 192, 256 B; 128 is also the dSᵀ image),
//    at the addresses the kernels compute: row_offsets (fa_bwd_common.h), tr_offsets and
//    lds_tr_addr (fa_common.h), which must agree with lds_off and with each other;
//  * stream_k_mode / macro_tile_area (tensile_names.h): the Tensile name parsing behind the
//    concurrency-safe GEMM selection;
//  * gemm_skinny_plan (gemm/skinny_plan.h): for both weight formats the decode GEMM's plan picks the
//    tile count per wave at its thresholds, a wave count within the kernel's MAXW and the full register
//    sets of K, and a grid that covers every tile; a table pins the plans of the model's shapes.
#include <cstdio>
#include <set>
#include <vector>

#include "../gemm/gemm_common.h"
#include "../gemm/skinny_plan.h"
#include "cs336/tensile_names.h"
#include "fa_bwd_common.h"

using namespace cs336;
using namespace cs336::fa;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");             \
    }                                         \
  } while (0)

static void check_tile_order() {
  const int nbhs[] = {1, 3, 6, 8, 16, 24, 64, 600, 384};
  const int nts[] = {1, 2, 4, 5, 8, 32, 128};
  const int grps[] = {1, 2, 3, 8, 1 << 20};
  long checked = 0;
  for (int nbh : nbhs)
    for (int nt : nts)
      for (int order = 0; order <= 2; ++order)
        for (int grp : grps) {
          std::vector<char> seen((size_t)nbh * nt, 0);
          for (int bid = 0; bid < nbh * nt; ++bid) {
            int bh = -1, lvl = -1;
            tile_order(bid, nbh, nt, order, grp, bh, lvl);
            CHECK(bh >= 0 && bh < nbh && lvl >= 0 && lvl < nt, "tile_order out of range nbh=%d nt=%d order=%d grp=%d bid=%d -> (%d,%d)",
                  nbh, nt, order, grp, bid, bh, lvl);
            if (bh < 0 || bh >= nbh || lvl < 0 || lvl >= nt) continue;
            char& s = seen[(size_t)bh * nt + lvl];
            CHECK(!s, "tile_order not injective nbh=%d nt=%d order=%d grp=%d (%d,%d)", nbh, nt, order, grp, bh, lvl);
            s = 1;
            ++checked;
          }
        }
  for (int total : {1, 7, 8, 9, 255, 256, 257, 2400, 4801}) {
    std::set<int> ids;
    for (int b = 0; b < total; ++b) ids.insert(xcd_remap(b, total));
    CHECK((int)ids.size() == total && *ids.begin() == 0 && *ids.rbegin() == total - 1, "xcd_remap not a permutation of %d", total);
  }
  std::printf("tile_order: %ld block ids checked\n", checked);
}

// tiles_m 204 is the XL token count in 256-row tiles (52,224 / 256); tiles_n 1..40 covers every
// column-tile count of the model's projections and the odd ones that leave a partial last group
static void check_gemm_tile_order() {
  std::vector<int> tms;
  for (int m = 1; m <= 20; ++m) tms.push_back(m);
  for (int m : {33, 192, 204}) tms.push_back(m);
  long checked = 0;
  for (int tiles_m : tms)
    for (int tiles_n : {1, 2, 3, 5, 8, 15, 32, 40}) {
      const int blocks = tiles_m * tiles_n;
      std::vector<char> seen((size_t)blocks, 0);
      for (int b = 0; b < blocks; ++b) {
        const gemm_common::Tile t = gemm_common::tile_of_block(b, blocks, tiles_m, tiles_n);
        const bool in = t.tm >= 0 && t.tm < tiles_m && t.tn >= 0 && t.tn < tiles_n;
        CHECK(in, "tile_of_block out of range tiles_m=%d tiles_n=%d block=%d -> (%d,%d)", tiles_m, tiles_n, b, t.tm, t.tn);
        if (!in) continue;
        char& s = seen[(size_t)t.tm * tiles_n + t.tn];
        CHECK(!s, "tile_of_block not injective tiles_m=%d tiles_n=%d (%d,%d)", tiles_m, tiles_n, t.tm, t.tn);
        s = 1;
        ++checked;
      }
    }
  std::printf("gemm tile order: %ld block ids checked\n", checked);
}

template <int RB>
static void check_swizzle() {
  constexpr int CPR = RB / 16;
  // chunks stay in their row and the map is a permutation of the row's chunks
  for (int r = 0; r < 256; ++r) {
    std::set<int> phys;
    for (int c = 0; c < CPR; ++c) {
      const int off = lds_off<RB>(r, c);
      CHECK(off >= r * RB && off < (r + 1) * RB && off % 16 == 0, "RB=%d row %d chunk %d leaves its row", RB, r, c);
      phys.insert(off);
    }
    CHECK((int)phys.size() == CPR, "RB=%d row %d: swizzle is not a permutation", RB, r);
  }
  // ds_read_b128 row fragments: 4 groups of 16 lanes, lane -> row r0 + (lane & 31), chunk 2ks + (lane >> 5),
  // addressed as the one-kernel backwards do: a 32-row base + row_offsets (which must equal lds_off)
  const int g128[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                           {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
  constexpr int NKS = CPR / 2;
  int worst = 0;
  for (int r0 = 0; r0 < 128; r0 += 32)
    for (int ks = 0; ks < NKS; ++ks)
      for (int hi = 0; hi < 2; ++hi)
        for (const auto& g : g128) {
          int banks[64] = {0};
          for (int l : g) {
            const int lane = l + 32 * hi;
            uint32_t roff[NKS];
            row_offsets<RB>(lane & 31, lane >> 5, roff);
            const int a = r0 * RB + (int)roff[ks];
            CHECK(a == lds_off<RB>(r0 + (lane & 31), 2 * ks + (lane >> 5)), "RB=%d row_offsets lane %d ks %d base %d", RB, lane, ks, r0);
            for (int w = 0; w < 4; ++w) ++banks[(a / 4 + w) % 64];
          }
          for (int b : banks) worst = b > worst ? b : worst;
        }
  CHECK(worst <= 1, "RB=%d ds_read_b128 row fragments: %d-way bank conflict", RB, worst);
  // ds_read_b64_tr_b16: one instruction = one 32-lane half; the addresses are a 16-row base +
  // tr_offsets (the one-kernel backwards), which must equal lds_tr_frag's own (lds_tr_addr) for
  // every lane, column tile and base
  int worst_tr = 0;
  const int ndt = RB / 64;  // 32-wide column tiles
  for (int base = 0; base < 256; base += 16)
    for (int dt = 0; dt < ndt; ++dt)
      for (int h = 0; h < 2; ++h)
        for (int second = 0; second < 2; ++second) {
          int banks[64] = {0};
          for (int lane = 32 * h; lane < 32 * h + 32; ++lane) {
            uint32_t oa, ob;
            tr_offsets<RB>(lane, dt, oa, ob);
            int fa, fb;
            lds_tr_addr<RB>(0, base & ~31, (base >> 4) & 1, dt, lane, fa, fb);
            CHECK(base * RB + (int)oa == fa && base * RB + (int)ob == fb, "RB=%d tr_offsets lane %d tile %d base %d", RB, lane, dt, base);
            const int a = base * RB + (int)(second ? ob : oa);
            for (int w = 0; w < 2; ++w) ++banks[(a / 4 + w) % 64];
          }
          for (int b : banks) worst_tr = b > worst_tr ? b : worst_tr;
        }
  CHECK(worst_tr <= 1, "RB=%d ds_read_b64_tr_b16: %d-way bank conflict", RB, worst_tr);
  std::printf("swizzle RB=%d: row-fragment reads %d-way, transposed reads %d-way\n", RB, worst, worst_tr);
}

static void check_names() {
  CHECK(stream_k_mode("Cijk_Alik_Bljk_BBS_MT160x256x64_SS1_SK3_SKFTR0_SKXCCM8_TLDS1_WG32_8_1") == 3, "SK3");
  CHECK(stream_k_mode("Cijk_Ailk_Bjlk_BSS_MT256x256x64_SK0_SKXCCM0_WG32_8_1") == 0, "SK0");
  CHECK(stream_k_mode("Cijk_Ailk_Bjlk_MT128x128x64_SKXCCM8_WG32") == 0, "no SK token");
  CHECK(stream_k_mode("x_SK12") == 12, "trailing SK12");
  CHECK(stream_k_mode("") == 0 && stream_k_mode("_SK") == 0 && stream_k_mode("_SK_") == 0, "degenerate names");
  CHECK(macro_tile_area("Cijk_MT160x256x64_MI16") == 160 * 256, "MT160x256");
  CHECK(macro_tile_area("Cijk_noMT") == 0 && macro_tile_area("_MTx") == 0, "no MT");
}

// the row-constant staging of the backward kernels: row_perm is a bijection on each 64-row tile that puts
// accumulator register reg of lane-half h (32-row group t) at 32t + 16h + reg, and the LDS-DMA
// source chunks land the same rows in the same places
static void check_row_perm() {
  std::set<int> seen;
  for (int r = 0; r < 64; ++r) {
    CHECK(row_perm(r) >= 0 && row_perm(r) < 64, "row_perm(%d) out of range", r);
    seen.insert(row_perm(r));
  }
  CHECK(seen.size() == 64, "row_perm is not a bijection on 0..63");
  for (int t = 0; t < 2; ++t)
    for (int h = 0; h < 2; ++h)
      for (int reg = 0; reg < 16; ++reg)
        CHECK(row_perm(32 * t + acc_row(reg, h)) == 32 * t + 16 * h + reg, "row_perm t %d h %d reg %d", t, h, reg);
  for (int c = 0; c < 16; ++c)
    for (int u = 0; u < 4; ++u)
      CHECK(row_perm(4 * row_perm_src_chunk(c) + u) == 4 * c + u, "DMA chunk %d element %d", c, u);
}

// U (k-blocks per register set) and MAXW are written out here as the kernel's three configurations
// have them (TN 4: 4, 4; TN 2: 4, 8; TN 1: 8, 8), the k-block as 4 W loads of 8 / 16 k
static void check_skinny_plan() {
  std::vector<int> ns;
  for (int n = 1; n <= 8300; ++n) ns.push_back(n);  // every N: 4095 / 4096 and 8176 / 8177 are the tile thresholds
  ns.push_back(50257);
  long checked = 0;
  for (SkinnyFormat f : {SkinnyFormat::W16, SkinnyFormat::E4M3}) {
    const int unit = f == SkinnyFormat::W16 ? 8 : 16, kblock = 4 * unit;
    const char* fn = f == SkinnyFormat::W16 ? "16-bit" : "fp8";
    for (int N : ns)
      for (int K = unit; K <= 10240; K += unit) {
        int tn = -1, waves = -1;
        gemm_skinny_plan(f, N, K, tn, waves);
        const int tiles = (N + 15) / 16;
        CHECK(tn == (tiles >= 512 ? 4 : tiles >= 256 ? 2 : 1), "skinny plan %s N=%d K=%d: tn %d for %d tiles", fn, N, K, tn, tiles);
        if (tn != 1 && tn != 2 && tn != 4) continue;
        const int u = tn == 1 ? 8 : 4;
        CHECK(waves >= 1 && waves <= (tn == 4 ? 4 : 8), "skinny plan %s N=%d K=%d: %d waves at tn %d", fn, N, K, waves, tn);
        CHECK(waves <= std::max(1, K / (kblock * u)), "skinny plan %s N=%d K=%d: %d waves for %d full sets", fn, N, K, waves, K / (kblock * u));
        const int wgs = skinny_workgroups(N, tn);
        CHECK(wgs * tn >= tiles && (wgs - 1) * tn < tiles, "skinny plan %s N=%d: %d workgroups x %d for %d tiles", fn, N, wgs, tn, tiles);
        ++checked;
      }
  }
  // (N, K) -> (tn, waves), 16-bit then fp8, as the two plan functions gave them before they became one
  // (0, 0: K is no multiple of 16)
  const int table[][6] = {{48, 8240, 1, 8, 1, 8},   {4100, 1616, 2, 8, 2, 6},  {4800, 1600, 2, 8, 2, 6},  {1600, 1600, 1, 6, 1, 3},
                          {12800, 1600, 4, 4, 4, 4}, {50257, 1600, 4, 3, 4, 3}, {50257, 64, 4, 1, 4, 1},   {2560, 10240, 1, 8, 1, 8},
                          {8177, 512, 4, 4, 4, 2},  {8176, 512, 2, 4, 2, 2},   {1, 8, 1, 1, 0, 0},        {1, 16, 1, 1, 1, 1},
                          {6400, 1600, 2, 8, 2, 6}, {1600, 6400, 1, 8, 1, 8},  {4096, 256, 2, 2, 2, 1},   {4081, 1024, 2, 8, 2, 4},
                          {4080, 1024, 1, 4, 1, 2}, {17, 48, 1, 1, 1, 1}};
  for (const auto& r : table)
    for (int w8 = 0; w8 < 2; ++w8) {
      if (!r[2 + 2 * w8]) continue;
      int tn = -1, waves = -1;
      gemm_skinny_plan(w8 ? SkinnyFormat::E4M3 : SkinnyFormat::W16, r[0], r[1], tn, waves);
      CHECK(tn == r[2 + 2 * w8] && waves == r[3 + 2 * w8], "skinny plan %s (%d, %d): (%d, %d), recorded (%d, %d)", w8 ? "fp8" : "16-bit", r[0],
            r[1], tn, waves, r[2 + 2 * w8], r[3 + 2 * w8]);
    }
  std::printf("skinny plan: %ld (format, N, K) checked\n", checked);
}

int main() {
  check_skinny_plan();
  check_row_perm();
  check_tile_order();
  check_gemm_tile_order();
  check_swizzle<64>();
  check_swizzle<128>();
  check_swizzle<192>();
  check_swizzle<256>();
  check_names();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("host checks passed\n");
  return 0;
}
