// cs336-build: agpr-accumulators
//
// "gemm8w": the weight-gradient GEMMs of the Transformer step, dW = dYᵀ·X, straight from the
// token-major activations (no dYᵀ / Xᵀ transposes):
//
//   C[m][n] = Σ_t A[t][m] · B[t][n]     A = dY [tokens][N_out], B = X [tokens][K_in], fp32 out
//
// (or the transposed roles, C stored transposed, when that tiles the shape better). Both operands are
// "MN-major": the contraction index t is the row of the stored matrix. Structure follows gemm8
// (csrc/gemm/gemm8.hip: 256 × 64·FN tile, BK 64, 8 waves 2 × 4, second wave group one barrier
// behind, two LDS-DMA stages, counted vmcnt waits), with what MN-major operands change:
//
// * LDS images are [64 t][R] (R = 256 or 320 columns, rows of 512 / 640 B) and every 16x16x32
//   fragment is two ds_read_b64_tr_b16 (the transposed LDS read: lane i of a 16-lane group gets
//   column i of 4 rows). The 32-B slots of each row are XOR-swizzled by the row so the 8 rows a
//   32-lane half reads land on 8 different bank slots (conflict-free for both row lengths); as
//   always with LDS-DMA, the swizzle is applied to the per-lane global source address;
// * a K-tile runs as 2 phases split along K -- k 0-31 and k 32-63, each over all 128 rows of the
//   wave (8 A fragments in two sets of four, FN B fragments: 52 operand VGPRs at FN 5) with a
//   cluster of 8 x FN MFMAs -- because a DMA granule holds whole t-rows. The wave group that does
//   not compute reads its fragments, issues DMA and waits, and in this kernel that reader is the
//   critical path (in-kernel stamps, profiles/gemm8w_phase_balance.md: its segment is longer than
//   the partner's cluster in every phase, so the K-tile costs the sum of the reader segments, not
//   the largest): each segment pays the LDS latency and the lgkmcnt(0) drain once whatever it
//   reads, so two segments of 26 reads cost less than four of 18 / 8 / 18 / 8; and the reader's
//   VALU is kept to nothing -- every lane carries the LDS address of each fragment's first read in
//   a register (8 + FN), the second read and the second K-half are immediate offsets, and the
//   addresses change stage once per K-tile behind the last MFMAs;
// * DMA order and counted waits. Per K-tile t (stage t & 1), in issue order: P0(t) restages the
//   other stage's t-rows 32-63 (last read in P1(t-1)) with the second half of K-tile t+1; P1(t)
//   restages this stage's t-rows 0-31 (last read in P0(t)) with the first half of K-tile t+2. A
//   half is waited for one phase before its first read (the wave's vmcnt, then the barrier before
//   the cluster, which the second wave group -- one barrier behind -- passes before the first
//   group reads). vmcnt retires in issue order, so with n0 / n1 granules per wave in a first /
//   second half (N01 = n0 + n1 is the same for every wave):
//     P0(t) retires second half(t):  younger are first half(t+1) [P1(t-1) or the prologue] and
//           second half(t+1) [just issued] -> vmcnt(N01); on the last K-tile nothing -> vmcnt(0);
//     P1(t) retires first half(t+1): younger are second half(t+1) [P0(t)] and first half(t+2)
//           [just issued] -> vmcnt(N01); with no K-tile t+2 only the former -> vmcnt(n1); on the
//           last K-tile no wait;
//     prologue: issues K-tile 0 whole and first half(1), retires first half(0) -> vmcnt(N01), or
//           vmcnt(n1) with a single K-tile.
//   Each half has two phases (about 1400 cycles) in flight;
// * fp32 accumulators leave straight from registers, 16 B per lane (4 consecutive output columns, or
//   4 consecutive output rows when the result is stored transposed), into the DDP bucket or a
//   split-K slab; rows beyond M (the last, padded row tile) are computed and dropped.
#include "cs336/kernels.h"
#include "gemm8.h"
#include "gemm_common.h"

namespace cs336 {
namespace gemm8 {
namespace {

using namespace gemm_common;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// 32-B slot swizzle of an MN-major image row t (S = row bytes): the 8 rows {0..3, 8..11} (+4) a
// 32-lane half of a transposed fragment read touches map to 8 distinct slots of a 256-B bank row
template <int S>
__device__ __forceinline__ int swz(int t) {
  static_assert(S % 256 == 0 || S % 256 == 128, "row bytes");
  if constexpr (S % 256 == 0) return (t & 3) | (((t >> 3) & 1) << 2);
  else return ((t >> 1) & 1) | (((t >> 3) & 1) << 1);  // rows alternate 128-B bank halves already
}

// one lane's 16 B of the result: stored, or added to what is there
__device__ __forceinline__ void store4(float4* d, f32x4 v, int accumulate) {
  float4 w = make_float4(v[0], v[1], v[2], v[3]);
  if (accumulate) {
    const float4 o = *d;
    w.x += o.x; w.y += o.y; w.z += o.z; w.w += o.w;
  }
  *d = w;
}

template <int FN>
struct WGeo {
  static constexpr int BN = 64 * FN, WTN = 16 * FN;
  static constexpr int SA = 2 * BM, SB = 2 * BN;          // image row bytes
  static constexpr int A_BYTES = BK * SA, B_BYTES = BK * SB, STAGE = A_BYTES + B_BYTES;
  static constexpr int GA = (32 * SA / 1024) / 8;         // A granules per wave per K-half (2)
  static constexpr int GB_T = 32 * SB / 1024;             // B granules per K-half (16 or 20)
  static constexpr int GB_HI = (GB_T + 7) / 8, GB_LO = GB_T / 8;  // 3/2 (FN 5) or 2/2 (FN 4)
};

template <int FN, int TRANS>
__global__ __launch_bounds__(NT, 2) void gemm8w_kernel(const WArgs p) {
  using G = WGeo<FN>;
  constexpr int BN = G::BN, WTN = G::WTN, SA = G::SA, SB = G::SB, STAGE = G::STAGE;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int tiles_n = p.N / BN, tiles_m = (p.M + BM - 1) / BM;
  const Tile tile = tile_of_block(blockIdx.x, gridDim.x, tiles_m, tiles_n);
  const int m0 = tile.tm * BM, n0 = tile.tn * BN;

  const int nkt_all = p.K / BK, split = blockIdx.y, nsplit = gridDim.y;
  const int kt0 = (int)((int64_t)nkt_all * split / nsplit), kt1 = (int)((int64_t)nkt_all * (split + 1) / nsplit);
  const int nkt = kt1 - kt0;

  // buffer descriptors based at (first row of this split, first column of this tile); the record
  // count ends at the tensor's last element, so the padded columns of the last row tile read zeros
  // instead of faulting at the very end
  const int64_t a_off = (int64_t)kt0 * BK * p.lda + m0, b_off = (int64_t)kt0 * BK * p.ldb + n0;
  auto rec = [](int64_t elems) -> uint32_t {
    const int64_t bytes = elems > 0 ? 2 * elems : 0;
    return (uint32_t)(bytes < 0x7fffffff ? bytes : 0x7fffffff);
  };
  const uint32_t a_rec = rec(p.a_elems - a_off), b_rec = rec(p.b_elems - b_off);
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(p.a + a_off), (short)0, a_rec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(p.b + b_off), (short)0, b_rec, 0x00020000);

  // ---- DMA granules: per K-half h (t-rows 32h..32h+31) A: 2 per wave; B: FN 5 -> 3 for the wave
  // group with wr == h, 2 for the other (20 in all), FN 4 -> 2 ---------------------------------
  uint32_t va[2][G::GA], la[2][G::GA];
  uint32_t vb[2][G::GB_HI], lb[2][G::GB_HI];
  auto src_off = [&](int S, int64_t ld, int byte) -> uint32_t {  // image byte -> global byte offset
    const int t = byte / S, cb = byte % S, ps = cb >> 5, hb = (cb >> 4) & 1;
    const int ls = ps ^ (S == SA ? swz<SA>(t) : swz<SB>(t));
    return 2u * (uint32_t)(t * ld + ls * 16 + hb * 8);
  };
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < G::GA; ++i) {
      const int g = wave + 8 * i;
      const int byte = h * 32 * SA + g * 1024;
      la[h][i] = (uint32_t)byte;
      va[h][i] = src_off(SA, p.lda, byte + lane * 16);
    }
#pragma unroll
    for (int i = 0; i < G::GB_HI; ++i) {
      int g;
      if constexpr (G::GB_HI == G::GB_LO) g = wave + 8 * i;
      else g = (wr == h) ? (wc + 4 * i) : (12 + wc + 4 * i);  // 3-group: 0..11, 2-group: 12..19
      const int byte = h * 32 * SB + g * 1024;
      lb[h][i] = (uint32_t)(G::A_BYTES + byte);
      vb[h][i] = src_off(SB, p.ldb, byte + lane * 16);
    }
  }
  const int nb_h0 = (G::GB_HI == G::GB_LO || wr == 0) ? G::GB_HI : G::GB_LO;  // B granules in half 0
  const int nb_h1 = (G::GB_HI == G::GB_LO || wr == 1) ? G::GB_HI : G::GB_LO;
  // LDS-DMA in inline asm (M0 = the wave-uniform LDS address; nothing else in this kernel writes
  // M0): issued through the builtin, the DMA is a pending LDS write the compiler cannot tell from the
  // transposed fragment reads, so it would need asm reads (below) whose results it must then copy
  // into the MFMA operand registers -- 4 v_mov per MFMA, measured 1.4x the VALU and 1.37x the wave
  // cycles of gemm8 on the same FLOPs (profiles/r3_gemm8w_pmc.md)
  const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
  auto glds = [&](const __amdgpu_buffer_rsrc_t& rs, uint32_t vo, uint32_t so, uint32_t lds_off) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, %3 offen lds"
                 :
                 : "v"(vo), "s"(lds_base + lds_off), "s"(rs), "s"(so)
                 : "memory");
  };
#define CS336_G8W_ISSUE(H, KT, ST)                                                                          \
  do {                                                                                                     \
    const uint32_t base_ = (uint32_t)((ST) * STAGE);                                                       \
    const uint32_t soa_ = (uint32_t)(KT) * BK * 2u * (uint32_t)p.lda, sob_ = (uint32_t)(KT) * BK * 2u * (uint32_t)p.ldb; \
    _Pragma("unroll") for (int i_ = 0; i_ < G::GA; ++i_)                                                   \
      glds(ra, va[H][i_], soa_, base_ + la[H][i_]); \
    const int nb_ = (H) == 0 ? nb_h0 : nb_h1;                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < G::GB_HI; ++i_) if (i_ < nb_)                                  \
      glds(rb, vb[H][i_], sob_, base_ + lb[H][i_]); \
  } while (0)
  // outstanding DMA of one K-half issue (this wave): n0 = GA + nb_h0, n1 = GA + nb_h1 (n0 + n1 does
  // not depend on the wave)
  const bool big0 = G::GB_HI != G::GB_LO && wr == 0;  // this wave issues 3 B granules in half 0
  constexpr int N01 = 2 * G::GA + G::GB_HI + G::GB_LO;  // both halves of one K-tile

  // ---- transposed fragment reads ------------------------------------------------------------
  const int g4 = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  // Each fragment = two ds_read_b64_tr_b16 (builtin) joined into one 128-bit MFMA operand; the
  // phase's explicit lgkmcnt(0) before its barrier retires them (WAR against the DMA restaging)
  // Each lane keeps the LDS byte address of the first read of every fragment (this K-tile's stage,
  // k 0-31); the second read (+4 t-rows) and the second K-half (+32 t-rows) are immediate offsets
  // (neither changes the swizzle of a row: it uses bits 0, 1 and 3 of t only), and the addresses
  // move to the other stage once per K-tile: 8 + FN adds per K-tile where recomputing them cost
  // one to two VALU per read in the reader's segment, which is the critical path
  uint32_t ada[8], adb[FN];
  {
    const int t0 = 8 * g4 + q;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      ada[i] = (uint32_t)(t0 * SA + ((((wr * 128 + 16 * i) >> 4) ^ swz<SA>(t0)) << 5) + 8 * pp);
#pragma unroll
    for (int j = 0; j < FN; ++j)
      adb[j] = (uint32_t)(G::A_BYTES + t0 * SB + ((((wc * WTN + 16 * j) >> 4) ^ swz<SB>(t0)) << 5) + 8 * pp);
  }
  auto frag = [&](uint32_t addr, int S, int ks) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + addr + 32 * ks * S));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + addr + 32 * ks * S + 4 * S));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  f32x4 acc[8][FN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fx[4], fy[4], fb[FN];  // A rows 0-63 / rows 64-127 of the wave's 128, B
  const int arow = wr * 128, bcol = wc * WTN;

  // one phase's MFMA cluster: all 8 row blocks x FN column blocks of one 32-wide K-half
  auto mma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const bf16x8& a = i < 4 ? fx[i & 3] : fy[i & 3];
        if constexpr (TRANS)  // lane: C[m = 4(l>>4)+r][n = l&15] -> 4 consecutive m (stored along a row of Cᵀ)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, fb[j], acc[i][j], 0, 0, 0);
        else  // lane: C[m = l&15][n = 4(l>>4)+r] -> 4 consecutive n
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], a, acc[i][j], 0, 0, 0);
      }
    __builtin_amdgcn_s_setprio(0);
  };
  auto read_x = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fx[i] = frag(ada[i], SA, ks);
  };
  auto read_y = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fy[i] = frag(ada[4 + i], SA, ks);
  };
  auto read_b = [&](int ks) {
#pragma unroll
    for (int j = 0; j < FN; ++j) fb[j] = frag(adb[j], SB, ks);
  };
  // the fragment addresses move to the other stage behind the K-tile's last MFMAs (the wave only
  // waits for the barrier there); opaque to the compiler so that the adds stay there
  auto next_stage = [&](int t) {
    const uint32_t d = (t & 1) ? (uint32_t)(-STAGE) : (uint32_t)STAGE;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ada[i] += d;
      asm volatile("" : "+v"(ada[i]));
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      adb[j] += d;
      asm volatile("" : "+v"(adb[j]));
    }
  };

  // diagnostic builds (-DCS336_G8_STAMP, any level): per-phase stamps of a few k-tiles in the middle
  // of this workgroup's range (PhaseStamps, gemm_common.h; scripts/gemm8w_stamps.py)
  PhaseStamps<(kStampLevel >= 1)> ps(true, nkt);

  // the two counted waits of a K-tile (constants: header comment)
  auto wait_h1 = [&](bool more1) {  // retires this K-tile's second half
    if (more1) vmcnt<N01>();
    else vmcnt<0>();
  };
  auto wait_h0 = [&](bool more1, bool more2) {  // retires the next K-tile's first half
    if (!more1) return;
    if (more2) vmcnt<N01>();
    else if (big0) vmcnt<G::GA + G::GB_LO>();  // younger: K-tile t+1's second half (n1)
    else vmcnt<G::GA + G::GB_HI>();
  };

  // ---- prologue: K-tile 0 whole, K-tile 1's first half; only K-tile 0's first half is waited for
  // here (its second half at phase 0) ------------------------------------------------------------
  if (nkt > 0) {
    CS336_G8W_ISSUE(0, 0, 0);
    CS336_G8W_ISSUE(1, 0, 0);
    if (nkt > 1) {
      CS336_G8W_ISSUE(0, 1, 1);
      vmcnt<N01>();  // younger: K-tile 0's second half, K-tile 1's first half
    } else {
      if (big0) vmcnt<G::GA + G::GB_LO>();  // younger: K-tile 0's second half (n1)
      else vmcnt<G::GA + G::GB_HI>();
    }
  }
  sbarrier();
  if (wr == 1) sbarrier();

  for (int t = 0; t < nkt; ++t) {
    const bool more1 = t + 1 < nkt, more2 = t + 2 < nkt;
    // P0: k 0-31, all 128 rows; restage the other stage's second half with K-tile t+1; retire this
    // K-tile's second half (read in P1)
    ps.begin(t);  // mark 0
    if (more1) CS336_G8W_ISSUE(1, t + 1, (t + 1) & 1);
    read_x(0);
    read_y(0);
    read_b(0);
    wait_h1(more1);
    lgkm0();
    ps.mark(1);
    sbarrier();
    ps.mark(2);
    mma();
    sbarrier();
    // P1: k 32-63; restage this stage's first half with K-tile t+2; retire K-tile t+1's first half
    ps.mark(3);
    if (more2) CS336_G8W_ISSUE(0, t + 2, t & 1);
    read_x(1);
    read_y(1);
    read_b(1);
    wait_h0(more1, more2);
    lgkm0();
    ps.mark(4);
    sbarrier();
    ps.mark(5);
    mma();
    next_stage(t);
    sbarrier();
    ps.mark(6);
    ps.end_tile();
  }
#undef CS336_G8W_ISSUE
  if (wr == 0) sbarrier();
  // 4 rows of 8 per workgroup (split-major), two per wave group
  if (ps.kOn && p.stamps && lane == 0 && wc == 0)
    ps.store(p.stamps + 32 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + 16 * wr, nkt);

  // ---- epilogue: fp32 straight from the accumulators, 16 B per lane ----------------------------
  float* c = p.c + (int64_t)split * p.slab_stride;
  const int lr = lane & 15, lq = 4 * (lane >> 4);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x4 v = acc[i][j];
      if constexpr (TRANS) {
        // C[m .. m+3][n] -> Cᵀ row n, columns m .. m+3
        const int m = m0 + arow + 16 * i + lq, n = n0 + bcol + 16 * j + lr;
        if (m < p.M) store4(reinterpret_cast<float4*>(c + (int64_t)n * p.ldc + m), v, p.accumulate);
      } else {
        const int m = m0 + arow + 16 * i + lr, n = n0 + bcol + 16 * j + lq;
        if (m < p.M) store4(reinterpret_cast<float4*>(c + (int64_t)m * p.ldc + n), v, p.accumulate);
      }
    }
}

template <int FN, int TRANS>
void launch_wt(const WArgs& p_in, hipStream_t s) {
  WArgs p = p_in;
  const dim3 grid((unsigned)(((p.M + BM - 1) / BM) * (p.N / (64 * FN))), (unsigned)p.splits), block(NT);
  if (4 * (int64_t)grid.x * grid.y > p.stamp_rows) p.stamps = nullptr;
  hipLaunchKernelGGL((gemm8w_kernel<FN, TRANS>), grid, block, 0, s, p);
}

}  // namespace

bool launch_w(const WArgs& p, int fn, hipStream_t s) {
  if (p.K % BK || p.K < BK || p.M <= 0 || p.M % 4 || p.splits < 1 || p.splits > 64) return false;
  if (fn == 0) fn = p.N % 320 == 0 ? 5 : (p.N % 256 == 0 ? 4 : 0);
  if ((fn != 4 && fn != 5) || p.N % (64 * fn)) return false;
  if (p.splits > 1 && p.accumulate) return false;
  if (fn == 5) {
    if (p.trans_out) launch_wt<5, 1>(p, s);
    else launch_wt<5, 0>(p, s);
  } else {
    if (p.trans_out) launch_wt<4, 1>(p, s);
    else launch_wt<4, 0>(p, s);
  }
  return true;
}

}  // namespace gemm8
}  // namespace cs336
