// Launch plan of the skinny-M decode GEMM (gemm_skinny.h), host code only: the kernel's dispatch,
// csrc/tests/host_checks.cpp and csrc/tests/skinny_w4_plan_check.cpp call it. The reasoning behind the
// numbers is in the kernel files.
#pragma once

#include <algorithm>

#include "cs336/skinny_format.h"

namespace cs336 {

// k per 16-byte W load: 8 values of a 16-bit format, 16 e4m3 bytes, 32 e2m1 codes (one MX block). A
// lane group of 4 such loads is the kernel's k-block (32 / 64 / 128 k), and K must be a multiple of
// one load.
constexpr int skinny_k_per_load(SkinnyFormat f) { return f == SkinnyFormat::MXFP4 ? 32 : (f == SkinnyFormat::E4M3 ? 16 : 8); }
constexpr int skinny_kblock(SkinnyFormat f) { return 4 * skinny_k_per_load(f); }

constexpr int kSkinnyTargetWaves = 2048;  // about 8 waves on each of the 256 CUs

// k-blocks per register set and most waves per workgroup of the configuration with tn W tiles per
// wave. MXFP4 halves U: its x fragments per k-block are twice FP8's, and a set then covers FP8's k.
constexpr int skinny_u(int tn) { return tn == 1 ? 8 : 4; }
constexpr int skinny_u(SkinnyFormat f, int tn) { return f == SkinnyFormat::MXFP4 ? skinny_u(tn) / 2 : skinny_u(tn); }
constexpr int skinny_maxw(int tn) { return tn == 4 ? 4 : 8; }

// workgroups of a launch with tn W tiles (16 rows each) per wave: every wave of one covers the same tn tiles
constexpr int skinny_workgroups(int N, int tn) { return ((N + 15) / 16 + tn - 1) / tn; }

// W tiles per wave (1 / 2 / 4) and waves (K ranges) per workgroup the launch uses for (N, K)
inline void gemm_skinny_plan(SkinnyFormat f, int N, int K, int& tn, int& waves) {
  const int tiles = (N + 15) / 16;
  tn = tiles >= 512 ? 4 : (tiles >= 256 ? 2 : 1);
  const int wgs = skinny_workgroups(N, tn);
  const int nfull = K / (skinny_kblock(f) * skinny_u(f, tn));
  const int want = (kSkinnyTargetWaves + wgs - 1) / wgs;
  waves = std::max(1, std::min(skinny_maxw(tn), std::min(want, nfull)));
}

}  // namespace cs336
