// Pieces the MFMA GEMM kernels share (gemm.hip, gemm8.hip, gemm8w.hip): operand typedefs, the grouped
// tile order, the raw wait / barrier primitives and the per-phase stamp recorder of the diagnostic
// builds. Everything here is inlined; the kernels keep their own names and namespaces.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cs336 {
namespace gemm_common {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// gemm8 / gemm8w tile: 256 rows, 64-deep k-tiles, 512 threads (gemm.hip has its own tile shapes)
constexpr int BM = 256, BK = 64, NT = 512;

// ---- tile order ---------------------------------------------------------------------------------
// Block ids go round-robin over the 8 XCDs; xcd_remap gives the blocks of one XCD a contiguous range
// of ids (a bijection on [0, total) for any total). The remapped id then walks groups of kGroupM
// tile rows column by column, so the tiles co-resident on one XCD share A row panels and B column
// panels in that XCD's L2. tile_of_block is a bijection from [0, tiles_m·tiles_n) onto the tiles
// (csrc/tests/host_checks.cpp, check_gemm_tile_order).
constexpr int kGroupM = 8;

__host__ __device__ __forceinline__ int xcd_remap(int bid, int total) {
  const int xcd = bid & 7, q = total >> 3, r = total & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

struct Tile { int tm, tn; };
// the kernels pass blockIdx.x and gridDim.x
__host__ __device__ __forceinline__ Tile tile_of_block(int block, int blocks, int tiles_m, int tiles_n) {
  const int bid = xcd_remap(block, blocks);
  const int per_group = kGroupM * tiles_n;
  const int first_m = (bid / per_group) * kGroupM;
  const int gsz = tiles_m - first_m < kGroupM ? tiles_m - first_m : kGroupM;
  return {first_m + (bid % per_group) % gsz, (bid % per_group) / gsz};
}

// ---- waits and barriers ---------------------------------------------------------------------------
// raw s_barrier (never __syncthreads(), which would drain the DMA in flight), fenced so that the
// compiler moves nothing across it
__device__ __forceinline__ void sbarrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int N>
__device__ __forceinline__ void vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// where this wave runs (rows of the stamp buffer end with these two)
__device__ __forceinline__ void hw_ids(uint32_t& hw, uint32_t& xcc) {
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
}

// ---- per-phase stamps (diagnostic builds: -DCS336_G8_STAMP=1 or 2) --------------------------------
#ifdef CS336_G8_STAMP
constexpr int kStampLevel = CS336_G8_STAMP;
#else
constexpr int kStampLevel = 0;
#endif

// Recorder of a two-phase main loop. kTiles k-tiles in the middle of the workgroup's range are
// stamped at every phase's entry (mark 3p; begin() is mark 0), after its reads / DMA issue / counted
// waits (3p + 1) and after the barrier before its MFMA cluster (3p + 2); mark 3·kPhases comes after
// the last barrier. The sums of the three segments per phase leave through store(): two rows of 8
// per wave group -- work[4], wait[4] | mma[4], stamped k-tiles, k-tiles, HW_ID, XCC_ID -- which
// `analyse` in scripts/gemm8w_stamps.py reads (the rows have room for four phases).
// PhaseStamps<false> is the same interface with nothing in it: the shipped loops call it too. The
// one lane per wave group that calls store() is picked behind `ps.kOn &&`: without that constant
// the dead lane test alone moved the shipped gemm8's assembly (profiles/gemm_shared_helpers.md).
template <bool ON>
struct PhaseStamps {
  static constexpr bool kOn = false;
  __device__ __forceinline__ PhaseStamps(bool, int) {}
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void end_tile() {}
  __device__ __forceinline__ void store(uint64_t*, int) const {}
};

template <>
struct PhaseStamps<true> {
  static constexpr bool kOn = true;
  static constexpr int kTiles = 4, kPhases = 2;
  uint32_t work[4] = {0, 0, 0, 0}, wait[4] = {0, 0, 0, 0}, mma[4] = {0, 0, 0, 0}, cnt = 0;
  uint32_t ts[3 * kPhases + 1];
  int lo;           // first stamped k-tile
  bool on, samp = false;  // this launch records; this k-tile is one of the stamped ones

  // on: the launch has a buffer with room for this workgroup's rows; nkt: k-tiles of this workgroup
  __device__ __forceinline__ PhaseStamps(bool on_, int nkt) : lo(nkt > kTiles ? (nkt - kTiles) / 2 : 0), on(on_) {}

  __device__ __forceinline__ static uint32_t now() {
    uint64_t v;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return (uint32_t)v;
  }
  __device__ __forceinline__ void begin(int t) {
    samp = on && t >= lo && t < lo + kTiles;
#pragma unroll
    for (int i = 0; i <= 3 * kPhases; ++i) ts[i] = 0;
    mark(0);
  }
  __device__ __forceinline__ void mark(int i) {
    if (samp) ts[i] = now();
  }
  __device__ __forceinline__ void end_tile() {
    if (!samp) return;
#pragma unroll
    for (int ph = 0; ph < kPhases; ++ph) {
      work[ph] += ts[3 * ph + 1] - ts[3 * ph];
      wait[ph] += ts[3 * ph + 2] - ts[3 * ph + 1];
      mma[ph] += ts[3 * ph + 3] - ts[3 * ph + 2];
    }
    ++cnt;
  }
  // rows: this wave group's two rows; called by one lane of the group
  __device__ __forceinline__ void store(uint64_t* rows, int nkt) const {
    if (!on) return;
    uint32_t hw, xcc;
    hw_ids(hw, xcc);
#pragma unroll
    for (int ph = 0; ph < kPhases; ++ph) {
      rows[ph] = work[ph];
      rows[4 + ph] = wait[ph];
      rows[8 + ph] = mma[ph];
    }
    rows[12] = cnt; rows[13] = (uint64_t)nkt; rows[14] = hw; rows[15] = xcc;
  }
};

}  // namespace gemm_common
}  // namespace cs336
