// Host interface of the NT projection GEMM with fused SwiGLU epilogues (csrc/gemm/gemm8.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cs336 {
namespace gemm8 {

// C = A · Bᵀ, A [M][K] and B [N][K] bf16 K-major (row strides lda, ldb), bf16 out.
// epi 0: C [M][N].
// epi 1 (W1|W3 forward): B = [W1; W3] (2·half rows), N = 2·half; writes y = C = [a|b] (ldc) and
//        h = silu(a)·b [M][half] (ldh).
// epi 2 (W2 input gradient): N = half; dh = A·Bᵀ is not stored; reads y = [a|b] (ldy) and writes
//        C = [da|db] [M][2·half] (ldc).
// epi 3 (QKV forward + RoPE): C [M][N] with columns < rope_cols rotated in interleaved pairs by
//        the fp32 (ctx, rdh/2) cos/sin tables at position rpos[row] (or row % rseq when rpos is null).
// Requires M % 256 == 0, K % 64 == 0, N % (64·fn) == 0 (epi 1: half % (32·fn) == 0), 16-B aligned
// rows; fn = 5 (BN 320) or 4 (BN 256), 0 = pick.
struct Args {
  const uint16_t* a;
  const uint16_t* b;
  uint16_t* c;
  uint16_t* h;
  const uint16_t* y;
  int64_t lda, ldb, ldc, ldh, ldy;
  int M, N, K;
  int half;
  // epi 3
  const float* rcos;
  const float* rsin;
  const int64_t* rpos;
  int rseq, rope_cols, rdh;
  // diagnostic builds only (-DCS336_G8_STAMP, scripts/gemm8_stamps.py): per workgroup 8 uint64 --
  // s_memtime at start / after the prologue / after the main loop / after the epilogue's stores
  // retired, s_memrealtime at start and end, HW_ID, XCC_ID. Built with -DCS336_G8_STAMP=2 and with
  // room for 5 rows per workgroup (stamp_rows), 4 more rows per workgroup follow those, laid out as
  // gemm8w's below: per wave group and phase of the k-tile the cycles of reads + DMA issue + counted
  // waits, of the wait at the barrier before the MFMA cluster and from there to the next barrier,
  // summed over a few k-tiles in the middle of the range (scripts/gemm8_stamps.py --phases). Level
  // 2 slows the loop; level 1 leaves it untouched. Ignored by the shipped build, and by a launch
  // with more than stamp_rows workgroups.
  uint64_t* stamps = nullptr;
  int64_t stamp_rows = 0;
};
int pick_fn(int N, int epi, int half);
// whether this build writes stamps at all (built with -DCS336_G8_STAMP)
bool stamps_built();
// gemm8 and gemm8w address each operand (gemm8: and each tile's output rows) through one buffer
// descriptor with 32-bit byte offsets: every such extent in bytes must be < kDmaLimit. The extents
// are even (2-byte elements), so this is the same set that the two former spellings accepted:
// `< 2^31 - 2^20` here and `not >= 0x7fffffff - 2^20`, which differ at the odd 2^31 - 2^20 - 1 only.
constexpr int64_t kDmaLimit = (int64_t(1) << 31) - (int64_t(1) << 20);
bool launch(const Args& p, int epi, int fn, hipStream_t s);

// Weight gradient with both operands MN-major (csrc/gemm/gemm8w.hip): C[m][n] = Σ_t A[t][m]·B[t][n],
// A [K][lda] (m < M), B [K][ldb] (n < N), fp32 out. trans_out: C[m][n] stored at c[n·ldc + m].
// splits > 1: split s writes its partial to c + s·slab_stride (dense slabs, reduced by the caller).
// accumulate: c += (splits == 1 only). Requires K % 64 == 0, N % (64·fn) == 0 (fn 5 or 4), M % 4 == 0;
// M is padded to the 256-row tile (rows >= M are computed and dropped).
struct WArgs {
  const uint16_t* a;
  const uint16_t* b;
  float* c;
  int64_t lda, ldb, ldc, slab_stride;
  int64_t a_elems, b_elems;  // storage extent of a / b from their base pointers (bounds for the DMA)
  int M, N, K;
  int splits;
  int trans_out, accumulate;
  // diagnostic builds only (-DCS336_G8_STAMP, scripts/gemm8w_stamps.py): the same buffer as
  // Args::stamps, 4 rows of 8 uint64 per workgroup (split-major) -- per wave group the cycles of
  // each of the four phases, summed over a few k-tiles in the middle of the range: reads + DMA issue
  // + counted waits, the wait at the barrier before the MFMA cluster, from there to the next barrier;
  // then the number of stamped k-tiles, the k-tiles, HW_ID, XCC_ID. Ignored by the shipped build,
  // and by a launch whose workgroups need more than stamp_rows rows.
  uint64_t* stamps = nullptr;
  int64_t stamp_rows = 0;
};
bool launch_w(const WArgs& p, int fn, hipStream_t s);

}  // namespace gemm8
}  // namespace cs336
