// Skinny-M GEMM for decode: y[M,N] = x[M,K] · W[N,K]ᵀ with 1 <= M <= 16 (gfx950, wave64).
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
//     column only). K % 32 != 0: the last k-blocks run one at a time with the 16-B chunks at
//     k >= K replaced by zeros in both operands.
#include <algorithm>

#include "cs336/common.h"
#include "cs336/kernels.h"

namespace cs336 {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

template <typename T> struct Mma;
template <> struct Mma<BF16> {
  static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma<F16> {
  static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x4 ld16_nt(const uint16_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// TN: W tiles (16 rows each) per wave, sharing one x fragment; U: k-blocks (32 k) per register set;
// MAXW: most waves (K ranges) per workgroup.
template <typename T, int TN, int U, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void gemm_skinny_kernel(const SkinnyParams p) {
  __shared__ f32x4 red[MAXW * TN * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = (int)(blockDim.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = (int)blockIdx.x * (16 * TN);

  const uint16_t* wrow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
    wrow[t] = static_cast<const uint16_t*>(p.w) + (int64_t)min(n0 + 16 * t + r, p.N - 1) * p.ldw + 8 * g;
  const uint16_t* xrow = static_cast<const uint16_t*>(p.x) + (int64_t)min(r, p.M - 1) * p.ldx + 8 * g;

  f32x4 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frag {
    u32x4 w[TN][U];
    u32x4 x[U];
  };
  auto load = [&](Frag& f, int it) {
    const int k = it * (32 * U);
#pragma unroll
    for (int u = 0; u < U; ++u) f.x[u] = ld16(xrow + k + 32 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) f.w[t][u] = ld16_nt(wrow[t] + k + 32 * u);
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TN; ++t) acc[t] = Mma<T>::run(f.w[t][u], f.x[u], acc[t]);
  };

  // full register sets [it0, it1) of this wave's K range
  const int nfull = p.K / (32 * U);
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
  const int kt0 = nfull * (32 * U);
  const int ntail = (p.K - kt0 + 31) / 32;
  for (int j = wave; j < ntail; j += nw) {
    const int k = kt0 + 32 * j;
    const bool ok = k + 8 * g < p.K;  // K % 8 == 0: a 16-B chunk is all inside or all outside
    const int kk = ok ? k : -8 * g;   // outside: the row's first chunk (valid memory), then zeroed
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    u32x4 xv = ld16(xrow + kk);
    xv = ok ? xv : zero;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      u32x4 wv = ld16_nt(wrow[t] + kk);
      wv = ok ? wv : zero;
      acc[t] = Mma<T>::run(wv, xv, acc[t]);
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
void launch(const SkinnyParams& p, int waves, hipStream_t s) {
  const int tiles = (p.N + 15) / 16, wgs = (tiles + TN - 1) / TN;
  hipLaunchKernelGGL((gemm_skinny_kernel<T, TN, U, MAXW>), dim3(wgs), dim3(64 * waves), 0, s, p);
}

template <typename T>
void dispatch(const SkinnyParams& p, hipStream_t s) {
  int tn, waves;
  gemm_skinny_plan(p.N, p.K, tn, waves);
  // the file's 3 configurations per dtype (tests/test_skinny_resources.py counts them)
  if (tn == 4) launch<T, 4, 4, 4>(p, waves, s);
  else if (tn == 2) launch<T, 2, 4, 8>(p, waves, s);
  else launch<T, 1, 8, 8>(p, waves, s);
}

}  // namespace

void gemm_skinny_plan(int N, int K, int& tn, int& waves) {
  const int tiles = (N + 15) / 16;
  tn = tiles >= 512 ? 4 : (tiles >= 256 ? 2 : 1);
  const int u = tn == 1 ? 8 : 4, maxw = tn == 4 ? 4 : 8;
  const int wgs = (tiles + tn - 1) / tn;
  const int nfull = K / (32 * u);
  const int want = (kTargetWaves + wgs - 1) / wgs;
  waves = std::max(1, std::min(maxw, std::min(want, nfull)));
}

bool gemm_skinny_ok(int64_t M, int64_t N, int64_t K, int64_t elem_size) {
  // 32-bit row / k indices in the kernel (row offsets are 64-bit): N + 64 and K + 256 must fit
  return elem_size == 2 && M >= 1 && M <= 16 && N >= 1 && N < (int64_t)1 << 30 && K >= 8 && K % 8 == 0 &&
         K < (int64_t)1 << 30;
}

void gemm_skinny(const SkinnyParams& p, DType t, hipStream_t s) {
  if (t == DType::BF16) dispatch<BF16>(p, s);
  else if (t == DType::F16) dispatch<F16>(p, s);
  else {
    fprintf(stderr, "cs336: gemm_skinny takes bf16 / fp16 only\n");
    abort();
  }
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
