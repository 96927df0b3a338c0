// The skinny-M decode GEMM's one kernel template, its weight-format policies and its dispatch. Included
// by gemm_skinny.hip (the 16-bit and FP8 formats, 12 kernels) and gemm_skinny_w4.hip (MXFP4, 6 kernels;
// what that format changes is described there).
//
// Skinny-M GEMM for decode: y[M,N] = x[M,K] · W[N,K]ᵀ with 1 <= M <= 16 (gfx950, wave64), W in x's
// 16-bit type or as FP8 bytes with a scale per row (W8A16):
//   out[M,N] = round_T( fp32( x[M,K] · q[N,K]ᵀ ) * scale[N] ),  q OCP e4m3.
//
// One token per sequence makes every projection of a decode step a GEMM with M = batch rows: the
// whole cost is reading W once from HBM. The kernel streams W and does nothing else per byte:
//
//   * v_mfma_f32_16x16x32_{bf16,f16} with a 16-row W tile as the A operand and x as the B operand:
//     lane l holds k = 8(l>>4) .. +7 of W row (l & 15), which is ONE 16-byte load, and the same k of
//     batch row (l & 15). The dot products cost no VALU and every M up to 16 costs the same. Per load
//     instruction each W row is read in a 64-byte run (4 lanes x 16 B); consecutive instructions
//     continue the row.
//   * W goes from global memory straight to VGPRs with non-temporal 16-B loads (streamed once, no
//     reuse): no LDS staging. Two register sets of TN x U loads ping-pong: set B's loads are issued
//     before set A's MFMAs run, so 8-32 W loads per lane are in flight and the compiler's counted
//     s_waitcnt vmcnt sits at each MFMA, the first consumer.
//   * A wave reuses each x fragment for TN W tiles (TN = 4 / 2 for tall W: x then moves at 1/4 / 1/2
//     of W's instruction rate; it is L2-resident). W with fewer than 256 tiles (N < 4096) runs
//     TN = 1 so that there are enough workgroups to pull from every HBM channel; its x re-read is
//     M/16 of the W bytes, from L2.
//   * K is split INSIDE the workgroup: its waves own contiguous K ranges and the partial 16x16 fp32
//     tiles are summed through LDS in wave order. No atomics: a call is bitwise reproducible for
//     given shapes. The wave count (1..MAXW) is chosen on the host so that about 8 waves per CU exist.
//   * Edges by clamped addresses, never by branches around loads: W rows >= N read row N-1 and batch
//     rows >= M read row M-1 (the same cache lines again); their products land in accumulator
//     rows / columns that are never stored (an MFMA output element depends on its own A row and B
//     column only). K not a multiple of the k-block: the last k-blocks run one at a time with the
//     16-B W chunks at k >= K, and their x, replaced by zeros.
//
// What the FP8 format changes (the policy W8 below; everything else is the one kernel) and why:
//
//   * A 16-byte W load carries 16 k-values of one row, two MFMAs' worth. Lane (r, g) = (l & 15,
//     l >> 4) owns k = 16g .. 16g+15 of a 64-k block of W row r (still ONE 16-B load, and a 64-byte
//     run of the row per instruction) and the same k of batch row r (TWO 16-B loads of x, 32
//     contiguous bytes). The first MFMA takes the low 8 k of both, the second the high 8: the MFMA
//     sums over its 32 k-slots and does not care which k sits in which slot as long as A and B agree.
//   * W is converted in registers to x's type by v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: two
//     values per VALU instruction, 8 per W load, beside 2 MFMAs. Every e4m3 value is exact in bf16
//     and in fp16, so the conversion adds no error. The per-row scale multiplies the fp32 sum once in
//     the epilogue, after the in-workgroup reduction and before the one rounding to T; scale rows
//     >= N read scale[N-1], like the W rows.
//
// Plan (gemm_skinny_plan, skinny_plan.h). TN keeps the same thresholds in both formats, 4 / 2 / 1 at
// >= 512 / >= 256 / fewer tiles: they come from how many workgroups it takes to pull from every HBM
// channel, which counts tiles, not bytes. U (k-blocks per register set) is 4 / 4 / 8 in both, so a
// set holds the same TN x U 16-B W loads per lane -- the same bytes in flight per wave, which is what
// hides HBM latency -- and in FP8 covers twice the k. x per set is then 2U loads, twice the 16-bit
// format's registers; the TN = 1 configuration (2 x 96 fragment VGPRs) still fits the 256 that 8 waves
// of a workgroup leave each wave. Waves: up to 4 / 8 / 8, at most one per full register set of K,
// aiming at 2048 waves on the chip. With half the bytes per row a given K has half the register sets
// in FP8, so short-K weights run fewer, equally loaded waves than in bf16.
// MXFP4 (gemm_skinny_w4.hip) halves U to 2 / 2 / 4: its x fragments per k-block are twice FP8's, and a
// set then covers FP8's k with FP8's x registers, half its W bytes and one scale byte per W load.
#pragma once

#include "cs336/common.h"
#include "cs336/kernels.h"
#include "skinny_plan.h"

namespace cs336 {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// Act<T>::mma: one MFMA; Act<T>::lo / hi: the low / high two e4m3 bytes of a dword as a packed pair
// of T (exact); Act<T>::fp4<B>: the two e2m1 codes of byte B of a dword (low nibble first) times the
// power of two `scale`, as a packed pair of T
template <typename T> struct Act;
template <> struct Act<BF16> {
  static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t lo(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, false));
  }
  static __device__ __forceinline__ uint32_t hi(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, true));
  }
  template <int B> static __device__ __forceinline__ uint32_t fp4(uint32_t d, float scale) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, B));
  }
};
template <> struct Act<F16> {
  static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t lo(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d, 1.0f, false));
  }
  static __device__ __forceinline__ uint32_t hi(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d, 1.0f, true));
  }
  template <int B> static __device__ __forceinline__ uint32_t fp4(uint32_t d, float scale) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, scale, B));
  }
};

// Weight formats, on activations of type T. storage: W's element, the unit of ldw and of offsets into
// a W row; kPerLoad: k per 16-byte W load (8 / 16 / 32); kXChunks: 16-B x loads that cover the same k;
// mma: one W load times its x chunks into the accumulator; kRowScale: the epilogue multiplies by
// scale[n]. bscale: what a lane keeps per W load of a block-scaled format (MXFP4: the e8m0 byte of the
// load's 32-k block, read by ld_bscale at block index `b` of the lane's scale row); the other formats
// keep the empty NoScale, their ld_bscale touches no memory, and all of it compiles to nothing.
struct NoScale {};
template <typename T> struct W16 {
  typedef T act;
  typedef uint16_t storage;
  static constexpr SkinnyFormat kFormat = SkinnyFormat::W16;
  static constexpr int kPerLoad = skinny_k_per_load(kFormat), kXChunks = 1;
  static constexpr bool kRowScale = false, kBlockScale = false;
  typedef NoScale bscale;
  static __device__ __forceinline__ NoScale ld_bscale(const uint8_t*, int) { return NoScale{}; }
  static __device__ __forceinline__ NoScale unit_bscale() { return NoScale{}; }
  static __device__ __forceinline__ f32x4 mma(u32x4 w, const u32x4 (&x)[1], NoScale, f32x4 acc) { return Act<T>::mma(w, x[0], acc); }
};
template <typename T> struct W8 {
  typedef T act;
  typedef uint8_t storage;
  static constexpr SkinnyFormat kFormat = SkinnyFormat::E4M3;
  static constexpr int kPerLoad = skinny_k_per_load(kFormat), kXChunks = 2;
  static constexpr bool kRowScale = true, kBlockScale = false;
  typedef NoScale bscale;
  static __device__ __forceinline__ NoScale ld_bscale(const uint8_t*, int) { return NoScale{}; }
  static __device__ __forceinline__ NoScale unit_bscale() { return NoScale{}; }
  static __device__ __forceinline__ f32x4 mma(u32x4 w, const u32x4 (&x)[2], NoScale, f32x4 acc) {
    const u32x4 w0 = u32x4{Act<T>::lo(w[0]), Act<T>::hi(w[0]), Act<T>::lo(w[1]), Act<T>::hi(w[1])};
    const u32x4 w1 = u32x4{Act<T>::lo(w[2]), Act<T>::hi(w[2]), Act<T>::lo(w[3]), Act<T>::hi(w[3])};
    acc = Act<T>::mma(w0, x[0], acc);
    return Act<T>::mma(w1, x[1], acc);
  }
};
// OCP MXFP4: 32 e2m1 codes per 16-byte load, which is one MX block of one row, with one e8m0 byte.
// Dword d of the load is k = 8d .. 8d+7 of the lane's 32: four conversions (byte selects 0..3, the
// block's scale 2^(byte - 127) as the fp32 operand `byte << 23`) make the A operand of one MFMA, whose
// B operand is x chunk d. The scale is in the converted values: no epilogue multiply.
template <typename T> struct W4 {
  typedef T act;
  typedef uint8_t storage;
  static constexpr SkinnyFormat kFormat = SkinnyFormat::MXFP4;
  static constexpr int kPerLoad = skinny_k_per_load(kFormat), kXChunks = 4;
  static constexpr bool kRowScale = false, kBlockScale = true;
  typedef uint32_t bscale;
  static __device__ __forceinline__ uint32_t ld_bscale(const uint8_t* row, int b) { return row[b]; }
  static __device__ __forceinline__ uint32_t unit_bscale() { return 127u; }
  static __device__ __forceinline__ f32x4 mma(u32x4 w, const u32x4 (&x)[4], uint32_t sb, f32x4 acc) {
    const float s = __builtin_bit_cast(float, sb << 23);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const u32x4 wd = u32x4{Act<T>::template fp4<0>(w[d], s), Act<T>::template fp4<1>(w[d], s),
                             Act<T>::template fp4<2>(w[d], s), Act<T>::template fp4<3>(w[d], s)};
      acc = Act<T>::mma(wd, x[d], acc);
    }
    return acc;
  }
};

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
template <typename S>
__device__ __forceinline__ u32x4 ld16_nt(const S* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// F: weight format; TN: W tiles (16 rows each) per wave, sharing one x fragment; U: k-blocks (4 W
// loads of k: 32 / 64 / 128) per register set; MAXW: most waves (K ranges) per workgroup.
template <typename F, int TN, int U, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void gemm_skinny_kernel(const SkinnyParams p) {
  typedef typename F::act T;
  typedef typename F::storage WS;
  constexpr int KL = F::kPerLoad, KB = 4 * KL, XC = F::kXChunks;
  constexpr int WL = 16 / (int)sizeof(WS);  // W elements per load; a row offset of k is k / (KL / WL) of them
  static_assert(KL % WL == 0, "a W element holds a whole number of k");
  constexpr int KPW = KL / WL;
  __shared__ f32x4 red[MAXW * TN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = (int)(blockDim.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = (int)blockIdx.x * (16 * TN);

  const WS* wrow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
    wrow[t] = static_cast<const WS*>(p.w) + (int64_t)min(n0 + 16 * t + r, p.N - 1) * p.ldw + WL * g;
  const uint16_t* xrow = static_cast<const uint16_t*>(p.x) + (int64_t)min(r, p.M - 1) * p.ldx + KL * g;

  // block-scaled formats: the lane's scale row, at its lane group's block (clamped like the W row)
  const uint8_t* srow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
    srow[t] = F::kBlockScale ? p.bscale + (int64_t)min(n0 + 16 * t + r, p.N - 1) * p.ldbs + g : nullptr;

  f32x4 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frag {
    u32x4 w[TN][U];
    u32x4 x[U][XC];
    typename F::bscale s[TN][U];
  };
  auto load = [&](Frag& f, int it) {
    const int k = it * (KB * U);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int h = 0; h < XC; ++h) f.x[u][h] = ld16(xrow + k + KB * u + 8 * h);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        f.w[t][u] = ld16_nt(wrow[t] + k / KPW + (KB / KPW) * u);
        f.s[t][u] = F::ld_bscale(srow[t] + k / KL, (KB / KL) * u);
      }
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) acc[t] = F::mma(f.w[t][u], f.x[u], f.s[t][u], acc[t]);
  };

  // full register sets [it0, it1) of this wave's K range
  const int nfull = p.K / (KB * U);
  const int it0 = nfull * wave / nw, it1 = nfull * (wave + 1) / nw;  // nfull < 2^25, waves <= 8
  Frag fa, fb;
  int it = it0;
  if (it < it1) load(fa, it);
  for (; it + 2 <= it1; it += 2) {
    load(fb, it + 1);
    mma(fa);
    if (it + 2 < it1) load(fa, it + 2);
    mma(fb);
  }
  if (it < it1) mma(fa);

  // the k-blocks after the last full set (fewer than U, plus a partial one), dealt round-robin
  const int kt0 = nfull * (KB * U);
  const int ntail = (p.K - kt0 + KB - 1) / KB;
  for (int j = wave; j < ntail; j += nw) {
    const int k = kt0 + KB * j;
    const bool ok = k + KL * g < p.K;  // K % KL == 0: a lane's W load is all inside or all outside
    const int kk = ok ? k : -KL * g;   // outside: the row's first chunk (valid memory), then zeroed
    const int kb = ok ? k / KL : -g;   // ... and the row's first block scale, then the unit
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    u32x4 xv[XC];
#pragma unroll
    for (int h = 0; h < XC; ++h) {  // load and select in one body: apart, the selects become branches
      const u32x4 v = ld16(xrow + kk + 8 * h);
      xv[h] = ok ? v : zero;
    }
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      u32x4 wv = ld16_nt(wrow[t] + kk / KPW);
      wv = ok ? wv : zero;
      typename F::bscale sv = F::ld_bscale(srow[t], kb);
      if constexpr (F::kBlockScale) sv = ok ? sv : F::unit_bscale();
      acc[t] = F::mma(wv, xv, sv, acc[t]);
    }
  }

  // sum the waves' partial tiles in wave order; lane l holds rows n = 4(l>>4) + j of batch row l & 15
#pragma unroll
  for (int t = 0; t < TN; ++t) red[(wave * TN + t) * 64 + lane] = acc[t];
  __syncthreads();
  typedef typename Elem<T>::storage S;
  for (int t = wave; t < TN; t += nw) {
    f32x4 s = red[t * 64 + lane];
    for (int w = 1; w < nw; ++w) s += red[(w * TN + t) * 64 + lane];
    const int n = n0 + 16 * t + 4 * g;
    if constexpr (F::kRowScale) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] *= p.scale[min(n + j, p.N - 1)];
    }
    if (r < p.M && n < p.N) {
      S* o = static_cast<S*>(p.out) + (int64_t)r * p.ldo + n;
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

template <typename F, int TN>
void launch(const SkinnyParams& p, int waves, hipStream_t s) {
  hipLaunchKernelGGL((gemm_skinny_kernel<F, TN, skinny_u(F::kFormat, TN), skinny_maxw(TN)>), dim3(skinny_workgroups(p.N, TN)),
                     dim3(64 * waves), 0, s, p);
}

template <typename F>
void dispatch(const SkinnyParams& p, hipStream_t s) {
  int tn, waves;
  gemm_skinny_plan(F::kFormat, p.N, p.K, tn, waves);
  // 3 configurations per format and dtype (tests/test_skinny_resources.py and
  // tests/test_skinny_w4_resources.py count them per file)
  if (tn == 4) launch<F, 4>(p, waves, s);
  else if (tn == 2) launch<F, 2>(p, waves, s);
  else launch<F, 1>(p, waves, s);
}

}  // namespace
}  // namespace cs336
