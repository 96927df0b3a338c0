// Weight-only FP8 / MXFP4 GEMM for 17 <= M <= 128 rows (gfx950, wave64): the batched decode and verify
// steps whose projections no longer fit the skinny kernel's one batch tile.
//
//   out[M,N] = round_T( fp32( x[M,K] · q[N,K]ᵀ ) * scale[N] ),  q OCP e4m3, scale fp32 per row   (W8)
//   out[M,N] = round_T( fp32( x[M,K] · dq[N,K]ᵀ ) ),  dq = e2m1 code * 2^(e8m0 block scale - 127)  (W4)
//
// x / out bf16 or fp16. Formats, operand rules and the conversions (exact) are those of gemm_skinny.h /
// gemm_skinny_w4.hip; this file reuses that header's Act<T>, vector types and format constants. 30 kernels:
// 2 formats x 2 activation types x the (MB, tiles per workgroup) pairs of the plan (gemm_wq_plan.h;
// tests/test_gemm_wq_resources.py pins the list and the registers).
//
// How the work is laid out:
//
//   * MFMA orientation is the skinny kernel's: v_mfma_f32_16x16x32_{bf16,f16}, a 16-row W tile as the A
//     operand, a 16-row block of x as the B operand; lane (r, g) = (l & 15, l >> 4) holds W row r and ONE
//     16-byte W load of it: k = KL g .. KL g + KL - 1 of a k-block of 4 KL (KL = 16 e4m3 / 32 MXFP4). The
//     load is converted ONCE into XC = KL / 8 A operands (convert(): v_cvt_scalef32_pk_*_fp8 / _fp4
//     through Act<T>), operand h holding k = KL g + 8 h .. + 7, and each feeds the MFMAs of all MB batch
//     blocks (MB = 2 / 4 / 8 for M <= 32 / 64 / 128): TN x MB fp32 4-vectors of accumulator per wave.
//   * W goes from HBM straight to VGPRs with 16-B non-temporal loads, two register sets (TN x U loads and,
//     for MXFP4, as many scale bytes) in ping-pong: the next set's loads are issued before this set's
//     MFMAs.
//   * x goes through LDS, shared by the RW row-waves of a k-group. A slab is 16 MB rows x the k of one W
//     register set (KS = 4 KL U). The group's 64 RW threads fetch the next slab with 16-B global loads into
//     registers while the current one is consumed, and write it to the other LDS buffer after the current
//     slab's MFMAs; one workgroup barrier per slab. In LDS a slab is row-major in 16-B chunks (CPR per row)
//     with the chunk index XOR-ed by the row (swz()): the B-fragment ds_read_b128 of a lane group is 16 rows
//     at one logical chunk, which the swizzle spreads over the 16 chunk slots of the 256-byte bank line.
//   * Work split, inside the workgroup only: RW row-waves each own TN W tiles; KG k-groups each own a
//     contiguous range of slabs and their own pair of slab buffers. After the loop the groups 1.. write
//     their accumulators to LDS (over the slab buffers), group 0 adds them in group order, applies the FP8
//     row scale to the fp32 sum and rounds once. No atomics, no workspace: bitwise reproducible.
//   * Edges by clamped addresses and selects, never branches around loads: W rows >= N read row N - 1 (and
//     its scales), x rows >= M are staged from row M - 1; both only reach accumulator rows / columns that
//     are never stored. A W load or x chunk at k >= K reads the row's first 16 bytes and is replaced by
//     zeros (MXFP4: with the unit block scale).
//
// Departures from the plan of record, and why:
//   * One masked path. Every W load and staged chunk carries the k < K select, full slabs included,
//     instead of an unmasked main loop plus a k-block-at-a-time tail: the select is 5 VALU per W load
//     beside its 2 MB .. 4 MB MFMAs, and one loop body keeps the barrier count of the k-groups equal by
//     construction. The last slab of an odd K runs all its U k-blocks, the ones past K on zeros.
//   * RW is a template parameter, not a launch dimension: the staging registers per thread are
//     slab chunks / (64 RW) and must be a compile-time array to stay in VGPRs.
#include "gemm_skinny.h"
#include "gemm_wq_plan.h"

namespace cs336 {
namespace {

// One W load -> its XC A operands. W8: dwords 0,1 are k 0..7, dwords 2,3 k 8..15 of the lane's 16.
template <typename T>
__device__ __forceinline__ void convert(W8<T>, u32x4 w, uint32_t, u32x4 (&a)[2]) {
  a[0] = u32x4{Act<T>::lo(w[0]), Act<T>::hi(w[0]), Act<T>::lo(w[1]), Act<T>::hi(w[1])};
  a[1] = u32x4{Act<T>::lo(w[2]), Act<T>::hi(w[2]), Act<T>::lo(w[3]), Act<T>::hi(w[3])};
}
// W4: dword d is k 8d .. 8d+7 of the lane's 32; the block scale 2^(sb - 127) is the conversion's operand
template <typename T>
__device__ __forceinline__ void convert(W4<T>, u32x4 w, uint32_t sb, u32x4 (&a)[4]) {
  const float s = __builtin_bit_cast(float, sb << 23);
#pragma unroll
  for (int d = 0; d < 4; ++d)
    a[d] = u32x4{Act<T>::template fp4<0>(w[d], s), Act<T>::template fp4<1>(w[d], s), Act<T>::template fp4<2>(w[d], s),
                 Act<T>::template fp4<3>(w[d], s)};
}

// F: weight format (W8<T> / W4<T> of gemm_skinny.h); MB: 16-row batch blocks; TN: W tiles per wave; RW:
// row-waves per k-group. blockDim.x = 64 RW KG, dynamic LDS = wq_lds_bytes.
template <typename F, int MB, int TN, int RW>
__global__ __launch_bounds__(64 * RW * wq_kgmax(F::kFormat, MB)) void gemm_wq_kernel(const SkinnyParams p) {
  typedef typename F::act T;
  constexpr int KL = F::kPerLoad, XC = KL / 8, KB = 4 * KL;
  constexpr int U = wq_u(F::kFormat, MB), KS = KB * U;
  constexpr int KPW = F::kBlockScale ? 2 : 1;  // k per byte of W
  constexpr int ROWS = 16 * MB, CPR = KS / 8;  // slab rows, 16-B chunks per slab row
  constexpr int NT = 64 * RW, SPT = ROWS * CPR / NT;
  constexpr int SLAB = ROWS * CPR;  // chunks per slab buffer
  static_assert(ROWS * CPR % NT == 0 && (CPR & (CPR - 1)) == 0 && CPR >= 8, "slab shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char wq_lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int KG = (int)(blockDim.x >> 6) / RW;
  const int kg = wave / RW, rw = wave - kg * RW;
  const int tg = (int)threadIdx.x - kg * NT;  // thread of the k-group
  const int r = lane & 15, g = lane >> 4;
  const int n0 = ((int)blockIdx.x * RW + rw) * (16 * TN);
  u32x4* const slab = reinterpret_cast<u32x4*>(wq_lds) + kg * (2 * SLAB);

  // the swizzle: rows of one 256-byte bank line (16 / CPR of them when CPR < 16) share a value
  constexpr int RPL = CPR >= 16 ? 1 : 16 / CPR, SWZ = (CPR >= 16 ? 16 : CPR) - 1;
  auto swz = [](int row) { return (row / RPL) & SWZ; };

  const uint8_t* wrow[TN];
  const uint8_t* srow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int64_t n = min(n0 + 16 * t + r, p.N - 1);
    wrow[t] = static_cast<const uint8_t*>(p.w) + n * p.ldw;
    srow[t] = F::kBlockScale ? p.bscale + n * p.ldbs : nullptr;
  }

  f32x4 acc[TN][MB];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[t][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct WSet {
    u32x4 w[TN][U];
    uint32_t s[TN][U];
  };
  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
  auto load_w = [&](WSet& f, int k0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + KB * u + KL * g;
      const bool ok = k < p.K;  // K % KL == 0: a load is all inside or all outside
      const int kk = ok ? k : 0;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const u32x4 v = ld16_nt(wrow[t] + kk / KPW);
        f.w[t][u] = ok ? v : zero;
        if constexpr (F::kBlockScale) {
          const uint32_t sv = srow[t][kk / KL];
          f.s[t][u] = ok ? sv : 127u;
        } else {
          f.s[t][u] = 0u;
        }
      }
    }
  };

  // staging: chunk i = tg + NT j of the slab, row i / CPR (clamped to M - 1), logical chunk i % CPR
  u32x4 st[SPT];
  auto stage_load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int i = tg + NT * j, row = i / CPR, c = i % CPR;
      const int k = k0 + 8 * c;
      const bool ok = k < p.K;
      const u32x4 v = ld16(static_cast<const uint16_t*>(p.x) + (int64_t)min(row, p.M - 1) * p.ldx + (ok ? k : 0));
      st[j] = ok ? v : zero;
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int i = tg + NT * j, row = i / CPR, c = i % CPR;
      slab[buf * SLAB + row * CPR + (c ^ swz(row))] = st[j];
    }
  };
  auto mma = [&](const WSet& f, int buf) {
    const u32x4* xs = slab + buf * SLAB;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 a[TN][XC];
#pragma unroll
      for (int t = 0; t < TN; ++t) convert(F{}, f.w[t][u], f.s[t][u], a[t]);
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const int row = 16 * b + r;
        u32x4 xv[XC];
#pragma unroll
        for (int h = 0; h < XC; ++h) xv[h] = xs[row * CPR + ((XC * (4 * u + g) + h) ^ swz(row))];
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int h = 0; h < XC; ++h) acc[t][b] = Act<T>::mma(a[t][h], xv[h], acc[t][b]);
      }
    }
  };

  // slabs [s0, s0 + cnt) of this k-group; every group runs niter iterations (the barriers), the ones past
  // its range at k0 = K: all loads masked, zeros times zeros
  const int ns = (p.K + KS - 1) / KS;  // K < 2^30
  const int s0 = (int)((int64_t)ns * kg / KG), cnt = (int)((int64_t)ns * (kg + 1) / KG) - s0;
  const int niter = (ns + KG - 1) / KG;
  auto k_of = [&](int i) { return i < cnt ? (s0 + i) * KS : p.K; };

  WSet wa, wb;
  stage_load(k_of(0));
  load_w(wa, k_of(0));
  stage_store(0);
  stage_load(k_of(1));
  __syncthreads();
  for (int i = 0; i < niter; i += 2) {
    load_w(wb, k_of(i + 1));
    mma(wa, 0);
    stage_store(1);
    stage_load(k_of(i + 2));
    __syncthreads();
    if (i + 1 < niter) {  // uniform over the workgroup
      load_w(wa, k_of(i + 2));
      mma(wb, 1);
      stage_store(0);
      stage_load(k_of(i + 3));
      __syncthreads();
    }
  }

  // k-groups 1.. leave their partial tiles in LDS (all slab reads are behind the last barrier); group 0
  // adds them in group order. Lane l holds W rows n = 4 (l >> 4) + j of batch row 16 b + (l & 15).
  f32x4* const red = reinterpret_cast<f32x4*>(wq_lds);
  constexpr int PER = TN * MB * 64;
  if (kg > 0) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int b = 0; b < MB; ++b) red[((kg - 1) * RW + rw) * PER + (t * MB + b) * 64 + lane] = acc[t][b];
  }
  if (KG > 1) __syncthreads();
  if (kg > 0) return;
  typedef typename Elem<T>::storage S;
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int n = n0 + 16 * t + 4 * g;
    float sc[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (F::kRowScale) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[j] = p.scale[min(n + j, p.N - 1)];
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      f32x4 s = acc[t][b];
      for (int q = 1; q < KG; ++q) s += red[((q - 1) * RW + rw) * PER + (t * MB + b) * 64 + lane];
      if constexpr (F::kRowScale) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] *= sc[j];
      }
      const int m = 16 * b + r;
      if (m < p.M && n < p.N) {
        S* o = static_cast<S*>(p.out) + (int64_t)m * p.ldo + n;
        if (p.vec_out && n + 3 < p.N) {
          const uint32_t lo = (uint32_t)Elem<T>::from_f(s[0]) | ((uint32_t)Elem<T>::from_f(s[1]) << 16);
          const uint32_t hi = (uint32_t)Elem<T>::from_f(s[2]) | ((uint32_t)Elem<T>::from_f(s[3]) << 16);
          *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (n + j < p.N) o[j] = Elem<T>::from_f(s[j]);
        }
      }
    }
  }
}

template <typename F, int MB, int TPW>
void launch_wq(const SkinnyParams& p, int kg, hipStream_t s) {
  // only the (MB, tiles per workgroup) pairs the plan can return exist as kernels
  if constexpr (TPW >= wq_min_tiles(F::kFormat, MB)) {
    constexpr int TN = wq_tn(TPW), RW = wq_rw(TPW);
    hipLaunchKernelGGL((gemm_wq_kernel<F, MB, TN, RW>), dim3(wq_workgroups(p.N, TPW)), dim3(64 * RW * kg),
                       wq_lds_bytes(F::kFormat, MB, kg), s, p);
  } else {
    fprintf(stderr, "cs336: gemm_wq plan outside the kernel list\n");
    abort();
  }
}

template <typename F, int MB>
void dispatch_tpw(const SkinnyParams& p, int tpw, int kg, hipStream_t s) {
  if (tpw == 1) launch_wq<F, MB, 1>(p, kg, s);
  else if (tpw == 2) launch_wq<F, MB, 2>(p, kg, s);
  else if (tpw == 4) launch_wq<F, MB, 4>(p, kg, s);
  else launch_wq<F, MB, 8>(p, kg, s);
}

template <typename F>
void dispatch_wq(const SkinnyParams& p, hipStream_t s) {
  int rw, kg, tn;
  gemm_wq_plan(F::kFormat, p.M, p.N, p.K, rw, kg, tn);
  const int mb = wq_mb(p.M), tpw = rw * tn;
  if (mb == 2) dispatch_tpw<F, 2>(p, tpw, kg, s);
  else if (mb == 4) dispatch_tpw<F, 4>(p, tpw, kg, s);
  else dispatch_tpw<F, 8>(p, tpw, kg, s);
}

}  // namespace

bool gemm_wq_ok(SkinnyFormat f, int64_t M, int64_t N, int64_t K, int64_t elem_size) {
  // 32-bit row / k indices in the kernel (row offsets are 64-bit): N + 128 and K + one slab must fit
  if (f != SkinnyFormat::E4M3 && f != SkinnyFormat::MXFP4) return false;
  const int kl = skinny_k_per_load(f);
  return elem_size == 2 && M >= kWqMinM && M <= kWqMaxM && N >= 1 && N < (int64_t)1 << 30 && K >= kl && K % kl == 0 &&
         K < (int64_t)1 << 30;
}

void gemm_wq(const SkinnyParams& p, SkinnyFormat f, DType t, hipStream_t s) {
  const bool w4 = f == SkinnyFormat::MXFP4;
  if (f == SkinnyFormat::W16 || (t != DType::BF16 && t != DType::F16)) {
    fprintf(stderr, "cs336: gemm_wq takes e4m3 / MXFP4 weights and bf16 / fp16 activations only\n");
    abort();
  }
  if (t == DType::BF16) w4 ? dispatch_wq<W4<BF16>>(p, s) : dispatch_wq<W8<BF16>>(p, s);
  else w4 ? dispatch_wq<W4<F16>>(p, s) : dispatch_wq<W8<F16>>(p, s);
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
