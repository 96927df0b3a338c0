// FP8 weight-only skinny-M GEMM for decode (W8A16, gfx950, wave64):
//   out[M,N] = round_T( fp32( x[M,K] · q[N,K]ᵀ ) * scale[N] ),  1 <= M <= 16, x / out bf16 or fp16,
//   q OCP e4m3 bytes with one fp32 scale per row.
//
// The same kernel as gemm_skinny.hip with W at half the bytes; what differs and why:
//
//   * A 16-byte W load now carries 16 k-values of one row, two MFMAs' worth. Lane (r, g) = (l & 15,
//     l >> 4) owns k = 16g .. 16g+15 of a 64-k block of W row r (ONE non-temporal 16-B load) and the
//     same k of batch row r (TWO 16-B loads of x, 32 contiguous bytes). The first MFMA takes the low
//     8 k of both, the second the high 8: v_mfma_f32_16x16x32_{bf16,f16} sums over its 32 k-slots and
//     does not care which k sits in which slot as long as A and B agree. Per load instruction a W row
//     is read in a 64-byte run (4 lanes x 16 B), as in the 16-bit kernel.
//   * W is converted in registers to x's type by v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: two
//     values per VALU instruction, 8 per W load, beside 2 MFMAs. Every e4m3 value is exact in bf16
//     and in fp16, so the conversion adds no error. The per-row scale multiplies the fp32 sum once in
//     the epilogue, after the in-workgroup reduction and before the one rounding to T.
//   * Kept: W straight to VGPRs with no LDS staging; two register sets in flight (set B's loads are
//     issued before set A's conversions and MFMAs); K split across the workgroup's waves and summed
//     through LDS in wave order (no atomics: bitwise reproducible); edges by clamped addresses (W rows
//     >= N read row N-1, batch rows >= M read row M-1, scale rows >= N read scale[N-1]; their products
//     land in accumulator rows / columns that are never stored); K % 64 != 0: the last k-blocks run one
//     at a time with the 16-k chunks at k >= K replaced by zeros in both operands.
//
// Plan (gemm_skinny_w8_plan). TN (W tiles per wave sharing one x fragment) keeps the 16-bit kernel's
// thresholds, 4 / 2 / 1 at >= 512 / >= 256 / fewer tiles: they come from how many workgroups it takes
// to pull from every HBM channel, which counts tiles, not bytes. U (64-k blocks per register set) is
// 4 / 4 / 8, so a set holds the same TN x U 16-B W loads per lane as there -- the same bytes in flight
// per wave, which is what hides HBM latency -- and covers twice the k. x per set is 2U loads, twice
// the 16-bit kernel's registers; the TN = 1 configuration (2 x 96 fragment VGPRs) still fits the 256
// that 8 waves of a workgroup leave each wave. Waves: up to 4 / 8 / 8 as there, at most one per full
// register set of K, aiming at the same 2048 waves on the chip. With half the bytes per row a given K
// has half the register sets, so short-K weights run fewer, equally loaded waves than in bf16.
#include <algorithm>

#include "cs336/common.h"
#include "cs336/kernels.h"

namespace cs336 {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// W8<T>::lo / hi: the low / high two e4m3 bytes of a dword as a packed pair of T (exact)
template <typename T> struct W8;
template <> struct W8<BF16> {
  static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t lo(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, false));
  }
  static __device__ __forceinline__ uint32_t hi(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, true));
  }
};
template <> struct W8<F16> {
  static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t lo(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d, 1.0f, false));
  }
  static __device__ __forceinline__ uint32_t hi(uint32_t d) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d, 1.0f, true));
  }
};

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x4 ld16_nt(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// 16 e4m3 bytes (k .. k+15 of one W row) times the same 16 k of x, as two MFMAs
template <typename T>
__device__ __forceinline__ f32x4 mma16(u32x4 w, u32x4 x0, u32x4 x1, f32x4 acc) {
  const u32x4 w0 = u32x4{W8<T>::lo(w[0]), W8<T>::hi(w[0]), W8<T>::lo(w[1]), W8<T>::hi(w[1])};
  const u32x4 w1 = u32x4{W8<T>::lo(w[2]), W8<T>::hi(w[2]), W8<T>::lo(w[3]), W8<T>::hi(w[3])};
  acc = W8<T>::mma(w0, x0, acc);
  return W8<T>::mma(w1, x1, acc);
}

// TN: W tiles (16 rows each) per wave, sharing one x fragment; U: k-blocks (64 k) per register set;
// MAXW: most waves (K ranges) per workgroup.
template <typename T, int TN, int U, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void gemm_skinny_w8_kernel(const SkinnyW8Params p) {
  __shared__ f32x4 red[MAXW * TN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = (int)(blockDim.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = (int)blockIdx.x * (16 * TN);

  const uint8_t* wrow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
    wrow[t] = static_cast<const uint8_t*>(p.wq) + (int64_t)min(n0 + 16 * t + r, p.N - 1) * p.ldw + 16 * g;
  const uint16_t* xrow = static_cast<const uint16_t*>(p.x) + (int64_t)min(r, p.M - 1) * p.ldx + 16 * g;

  f32x4 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frag {
    u32x4 w[TN][U];
    u32x4 x[U][2];
  };
  auto load = [&](Frag& f, int it) {
    const int k = it * (64 * U);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f.x[u][0] = ld16(xrow + k + 64 * u);
      f.x[u][1] = ld16(xrow + k + 64 * u + 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) f.w[t][u] = ld16_nt(wrow[t] + k + 64 * u);
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) acc[t] = mma16<T>(f.w[t][u], f.x[u][0], f.x[u][1], acc[t]);
  };

  // full register sets [it0, it1) of this wave's K range
  const int nfull = p.K / (64 * U);
  const int it0 = nfull * wave / nw, it1 = nfull * (wave + 1) / nw;  // nfull < 2^24, waves <= 8
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
  const int kt0 = nfull * (64 * U);
  const int ntail = (p.K - kt0 + 63) / 64;
  for (int j = wave; j < ntail; j += nw) {
    const int k = kt0 + 64 * j;
    const bool ok = k + 16 * g < p.K;  // K % 16 == 0: a lane's 16 k are all inside or all outside
    const int kk = ok ? k : -16 * g;   // outside: the row's first chunk (valid memory), then zeroed
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    u32x4 x0 = ld16(xrow + kk), x1 = ld16(xrow + kk + 8);
    x0 = ok ? x0 : zero;
    x1 = ok ? x1 : zero;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      u32x4 wv = ld16_nt(wrow[t] + kk);
      wv = ok ? wv : zero;
      acc[t] = mma16<T>(wv, x0, x1, acc[t]);
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
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] *= p.scale[min(n + j, p.N - 1)];
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

constexpr int kTargetWaves = 2048;  // about 8 waves on each of the 256 CUs

template <typename T, int TN, int U, int MAXW>
void launch(const SkinnyW8Params& p, int waves, hipStream_t s) {
  const int tiles = (p.N + 15) / 16, wgs = (tiles + TN - 1) / TN;
  hipLaunchKernelGGL((gemm_skinny_w8_kernel<T, TN, U, MAXW>), dim3(wgs), dim3(64 * waves), 0, s, p);
}

template <typename T>
void dispatch(const SkinnyW8Params& p, hipStream_t s) {
  int tn, waves;
  gemm_skinny_w8_plan(p.N, p.K, tn, waves);
  // the file's 3 configurations per dtype (tests/test_skinny_w8_resources.py counts them)
  if (tn == 4) launch<T, 4, 4, 4>(p, waves, s);
  else if (tn == 2) launch<T, 2, 4, 8>(p, waves, s);
  else launch<T, 1, 8, 8>(p, waves, s);
}

}  // namespace

void gemm_skinny_w8_plan(int N, int K, int& tn, int& waves) {
  const int tiles = (N + 15) / 16;
  tn = tiles >= 512 ? 4 : (tiles >= 256 ? 2 : 1);
  const int u = tn == 1 ? 8 : 4, maxw = tn == 4 ? 4 : 8;
  const int wgs = (tiles + tn - 1) / tn;
  const int nfull = K / (64 * u);
  const int want = (kTargetWaves + wgs - 1) / wgs;
  waves = std::max(1, std::min(maxw, std::min(want, nfull)));
}

bool gemm_skinny_w8_ok(int64_t M, int64_t N, int64_t K, int64_t elem_size) {
  // the 32-bit rules of gemm_skinny_ok (N + 64 and K + 512 fit); a W load is 16 k
  return elem_size == 2 && M >= 1 && M <= 16 && N >= 1 && N < (int64_t)1 << 30 && K >= 16 && K % 16 == 0 &&
         K < (int64_t)1 << 30;
}

void gemm_skinny_w8(const SkinnyW8Params& p, DType t, hipStream_t s) {
  if (t == DType::BF16) dispatch<BF16>(p, s);
  else if (t == DType::F16) dispatch<F16>(p, s);
  else {
    fprintf(stderr, "cs336: gemm_skinny_w8 takes bf16 / fp16 activations only\n");
    abort();
  }
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
