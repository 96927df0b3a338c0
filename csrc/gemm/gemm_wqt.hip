// Weight-only FP8 / MXFP4 tile GEMM for M > 128 rows (gfx950, wave64): prefill, chunk, extend and large
// verify / decode steps on the quantized weight copy.
//
//   out[M,N] = round_T( fp32( x[M,K] · q[N,K]ᵀ ) * scale[N] ),  q OCP e4m3, scale fp32 per row   (W8)
//   out[M,N] = round_T( fp32( x[M,K] · dq[N,K]ᵀ ) ),  dq = e2m1 code * 2^(e8m0 block scale - 127)  (W4)
//
// x / out bf16 or fp16. Formats, operand rules and the conversions (exact) are those of gemm_skinny.h /
// gemm_wq.hip; this file reuses that header's Act<T>, vector types and format constants. 12 tile kernels
// (2 formats x 2 activation types x the 3 tiles of the plan, gemm_wqt_plan.h) and 2 reduce kernels.
//
// A tile GEMM that dequantizes on the way into LDS:
//
//   * A workgroup of 4 waves (2 x 2) owns a BM x BN tile of out; a wave owns a (BM / 2) x (BN / 2) quadrant as
//     32 x 32 blocks of v_mfma_f32_32x32x16_{bf16,f16}. The W block is the A operand and the x block the B
//     operand, so a lane's 4 consecutive accumulator registers are 4 consecutive columns n of one row m:
//     one 8-byte store.
//   * Per k-tile of 64 a thread loads its share of the W tile straight into VGPRs, 16 bytes of one W row
//     per load (16 e4m3 values, or one 32-value MX block plus its e8m0 byte), converts it ONCE
//     (v_cvt_scalef32_pk_*_fp8 / _fp4 through Act<T>, the MX block scale as the conversion's operand) and
//     writes the 2 / 4 chunks of 16-bit values into the W image in LDS. x goes the same way without the
//     conversion (BM / 32 chunks per thread). Both images are rows of 128 bytes with the 16-byte chunk
//     index XOR-ed by the row (swz()): an operand read (32 rows at one logical chunk per half wave) and
//     the staging writes are spread over the banks.
//   * Two LDS buffers, one barrier per k-tile: the global loads of k-tile t + 1 are issued before the MFMAs
//     of k-tile t, their conversion and LDS writes come after those MFMAs and go to the buffer every wave
//     left at the previous barrier.
//   * Edges by clamped addresses and selects: W rows >= N read row N - 1 (and its scales), x rows >= M row
//     M - 1; both only reach accumulator rows / columns that are never stored. A W load or x chunk at k >= K
//     reads the row's first 16 bytes and is replaced by zeros (MXFP4: with the unit block scale), so LDS
//     holds zeros there: 0 x NaN through an MFMA would be NaN.
//   * Split K (plan): grid.z splits each own a range of k-tiles and store fp32 partial tiles to the
//     workspace; wqt_reduce_kernel adds them in split order, scales and rounds once. Without a split the
//     tile kernel's epilogue does the same from its registers. No atomics: bitwise reproducible.
#include "gemm_skinny.h"
#include "gemm_wqt_plan.h"

namespace cs336 {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

template <typename T> struct Mma32;
template <> struct Mma32<BF16> {
  static __device__ __forceinline__ f32x16 mma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma32<F16> {
  static __device__ __forceinline__ f32x16 mma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// One W load -> its chunks of 8 16-bit values, in k order. W8: dwords 0,1 are k 0..7, dwords 2,3 k 8..15.
template <typename T>
__device__ __forceinline__ void convert(W8<T>, u32x4 w, uint32_t, u32x4 (&a)[2]) {
  a[0] = u32x4{Act<T>::lo(w[0]), Act<T>::hi(w[0]), Act<T>::lo(w[1]), Act<T>::hi(w[1])};
  a[1] = u32x4{Act<T>::lo(w[2]), Act<T>::hi(w[2]), Act<T>::lo(w[3]), Act<T>::hi(w[3])};
}
// W4: dword d is k 8d .. 8d+7 of the load's 32; the block scale 2^(sb - 127) is the conversion's operand
template <typename T>
__device__ __forceinline__ void convert(W4<T>, u32x4 w, uint32_t sb, u32x4 (&a)[4]) {
  const float s = __builtin_bit_cast(float, sb << 23);
#pragma unroll
  for (int d = 0; d < 4; ++d)
    a[d] = u32x4{Act<T>::template fp4<0>(w[d], s), Act<T>::template fp4<1>(w[d], s), Act<T>::template fp4<2>(w[d], s),
                 Act<T>::template fp4<3>(w[d], s)};
}

struct WqtParams {
  SkinnyParams g;
  float* ws;     // split launches: S x M x ldws fp32 partials; else nullptr
  int64_t ldws;  // multiple of 4, >= N
  int tiles_m;   // tiles along M; blockIdx.x = tile_n * tiles_m + tile_m (the tiles of one W panel are neighbours)
  int ktiles;
};

// chunk swizzle of a 128-byte row (fa_common.h's swz<128>): rows 2g, 2g+1 share a 256-byte bank line
__device__ __forceinline__ int swz(int row) {
  const int g = (row >> 1) & 7;
  return g ^ ((g & 1) << 2);
}

// F: weight format (W8<T> / W4<T> of gemm_skinny.h); BM x BN: the workgroup's tile. blockDim.x = 256,
// grid = (tiles, 1, splits), dynamic LDS = wqt_lds_bytes(BM, BN).
template <typename F, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_wqt_kernel(const WqtParams q) {
  typedef typename F::act T;
  const SkinnyParams& p = q.g;
  constexpr int KT = kWqtKTile, KL = F::kPerLoad, XC = KL / 8;
  constexpr int KPW = F::kBlockScale ? 2 : 1;  // k per byte of W
  constexpr int LPR = KT / KL;                 // W loads per row of a k-tile
  constexpr int WLOADS = BN * LPR, WPT = (WLOADS + 255) / 256, XPT = BM * 8 / 256;
  constexpr int TMB = BM / 64, TNB = BN / 64;  // 32 x 32 blocks per wave
  constexpr int XIMG = BM * 8, BUF = XIMG + BN * 8;  // 16-byte chunks: x image, one buffer
  static_assert(KT == 64 && BM % 64 == 0 && BN % 64 == 0 && (WLOADS % 256 == 0 || WLOADS == 128), "tile shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char wqt_lds[];
  u32x4* const lds = reinterpret_cast<u32x4*>(wqt_lds);

  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile_m = (int)blockIdx.x % q.tiles_m, tile_n = (int)blockIdx.x / q.tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int z = (int)blockIdx.z, S = (int)gridDim.z;
  const int kt0 = (int)((int64_t)q.ktiles * z / S), kt1 = (int)((int64_t)q.ktiles * (z + 1) / S);

  // staging: x chunk (row xr + 32 j, logical chunk xc); W load (row wr + (256 / LPR) j, part wp of LPR)
  const int xr = tid >> 3, xc = tid & 7;
  const int wr = tid / LPR, wp = tid % LPR;
  const bool wact = WLOADS % 256 == 0 || wave < WLOADS / 64;  // wave-uniform
  const uint16_t* xrow[XPT];
#pragma unroll
  for (int j = 0; j < XPT; ++j) xrow[j] = static_cast<const uint16_t*>(p.x) + (int64_t)min(m0 + xr + 32 * j, p.M - 1) * p.ldx;
  const uint8_t* wrow[WPT];
  const uint8_t* srow[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const int64_t n = min(n0 + wr + (256 / LPR) * j, p.N - 1);
    wrow[j] = static_cast<const uint8_t*>(p.w) + n * p.ldw;
    srow[j] = F::kBlockScale ? p.bscale + n * p.ldbs : nullptr;
  }

  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
  u32x4 xs[XPT], wst[WPT];
  uint32_t sst[WPT];
  auto load = [&](int kt) {
    const int kx = kt * KT + 8 * xc, kw = kt * KT + KL * wp;
    const bool okx = kx < p.K, okw = kw < p.K;  // K % KL == 0: a load is all inside or all outside
    const int kkx = okx ? kx : 0, kkw = okw ? kw : 0;
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      const u32x4 v = ld16(xrow[j] + kkx);
      xs[j] = okx ? v : zero;
    }
    if (wact) {
#pragma unroll
      for (int j = 0; j < WPT; ++j) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(wrow[j] + kkw / KPW);
        wst[j] = okw ? v : zero;
        if constexpr (F::kBlockScale) {
          const uint32_t sv = srow[j][kkw / KL];
          sst[j] = okw ? sv : 127u;
        } else {
          sst[j] = 0u;
        }
      }
    }
  };
  auto store = [&](int buf) {
    u32x4* const img = lds + buf * BUF;
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      const int row = xr + 32 * j;
      img[row * 8 + (xc ^ swz(row))] = xs[j];
    }
    if (wact) {
#pragma unroll
      for (int j = 0; j < WPT; ++j) {
        const int row = wr + (256 / LPR) * j;
        u32x4 a[XC];
        convert(F{}, wst[j], sst[j], a);
#pragma unroll
        for (int h = 0; h < XC; ++h) img[XIMG + row * 8 + ((XC * wp + h) ^ swz(row))] = a[h];
      }
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fh = lane >> 5;
  f32x16 acc[TNB][TMB];
#pragma unroll
  for (int i = 0; i < TNB; ++i)
#pragma unroll
    for (int j = 0; j < TMB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  auto mma = [&](int buf) {
    const u32x4* const img = lds + buf * BUF;
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
      const int c = 2 * ks + fh;
      u32x4 a[TNB], b[TMB];
#pragma unroll
      for (int i = 0; i < TNB; ++i) {
        const int row = wn * (BN / 2) + 32 * i + fr;
        a[i] = img[XIMG + row * 8 + (c ^ swz(row))];
      }
#pragma unroll
      for (int j = 0; j < TMB; ++j) {
        const int row = wm * (BM / 2) + 32 * j + fr;
        b[j] = img[row * 8 + (c ^ swz(row))];
      }
#pragma unroll
      for (int i = 0; i < TNB; ++i)
#pragma unroll
        for (int j = 0; j < TMB; ++j) acc[i][j] = Mma32<T>::mma(a[i], b[j], acc[i][j]);
    }
  };

  // k-tiles [kt0, kt1) of this split (never empty); one barrier per k-tile
  const int nt = kt1 - kt0;
  load(kt0);
  store(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;  // uniform over the workgroup
    if (more) load(kt0 + t + 1);
    mma(t & 1);
    if (more) store((t + 1) & 1);
    __syncthreads();
  }

  // lane (fr, fh) holds, in registers 4 rq .. 4 rq + 3 of block (i, j), columns n .. n + 3 of row m
  typedef typename Elem<T>::storage O;
#pragma unroll
  for (int i = 0; i < TNB; ++i)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int n = n0 + wn * (BN / 2) + 32 * i + 8 * rq + 4 * fh;
      float sc[4] = {1.f, 1.f, 1.f, 1.f};
      if constexpr (F::kRowScale) {
        if (q.ws == nullptr) {
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[e] = p.scale[min(n + e, p.N - 1)];
        }
      }
#pragma unroll
      for (int j = 0; j < TMB; ++j) {
        const int m = m0 + wm * (BM / 2) + 32 * j + fr;
        float s[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = acc[i][j][4 * rq + e];
        if (q.ws != nullptr) {  // n % 4 == 0 and ldws % 4 == 0: n < ldws leaves room for all four
          if (m < p.M && n < q.ldws)
            *reinterpret_cast<float4*>(q.ws + ((int64_t)z * p.M + m) * q.ldws + n) = make_float4(s[0], s[1], s[2], s[3]);
          continue;
        }
        if (m >= p.M || n >= p.N) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] *= sc[e];
        O* o = static_cast<O*>(p.out) + (int64_t)m * p.ldo + n;
        if (p.vec_out && n + 3 < p.N) {
          const uint32_t lo = (uint32_t)Elem<T>::from_f(s[0]) | ((uint32_t)Elem<T>::from_f(s[1]) << 16);
          const uint32_t hi = (uint32_t)Elem<T>::from_f(s[2]) | ((uint32_t)Elem<T>::from_f(s[3]) << 16);
          *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < p.N) o[e] = Elem<T>::from_f(s[e]);
        }
      }
    }
}

// out[m, n .. n + 3] = round(scale[n] * (ws[0] + ws[1] + ... + ws[S - 1])), one thread per 4 columns
template <typename T>
__global__ __launch_bounds__(256) void wqt_reduce_kernel(const WqtParams q, int S) {
  const SkinnyParams& p = q.g;
  const int64_t gpr = q.ldws / 4, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = idx / gpr;
  const int n = (int)(idx - m * gpr) * 4;
  if (m >= p.M) return;
  const float4 v0 = *reinterpret_cast<const float4*>(q.ws + m * q.ldws + n);
  float s[4] = {v0.x, v0.y, v0.z, v0.w};
  for (int z = 1; z < S; ++z) {
    const float4 v = *reinterpret_cast<const float4*>(q.ws + ((int64_t)z * p.M + m) * q.ldws + n);
    s[0] += v.x;
    s[1] += v.y;
    s[2] += v.z;
    s[3] += v.w;
  }
  if (p.scale != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] *= p.scale[min(n + e, p.N - 1)];
  }
  typedef typename Elem<T>::storage O;
  O* o = static_cast<O*>(p.out) + m * p.ldo + n;
  if (p.vec_out && n + 3 < p.N) {
    const uint32_t lo = (uint32_t)Elem<T>::from_f(s[0]) | ((uint32_t)Elem<T>::from_f(s[1]) << 16);
    const uint32_t hi = (uint32_t)Elem<T>::from_f(s[2]) | ((uint32_t)Elem<T>::from_f(s[3]) << 16);
    *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.N) o[e] = Elem<T>::from_f(s[e]);
  }
}

template <typename F, int BM, int BN>
void launch_wqt(const WqtParams& q, int split, hipStream_t s) {
  const int64_t tiles = wqt_tiles(q.g.M, q.g.N, BM, BN);
  hipLaunchKernelGGL((gemm_wqt_kernel<F, BM, BN>), dim3((unsigned)tiles, 1, split), dim3(256), wqt_lds_bytes(BM, BN), s, q);
}

template <typename F>
void dispatch_wqt(const SkinnyParams& p, float* ws, hipStream_t s) {
  typedef typename F::act T;
  const WqtPlan plan = gemm_wqt_plan(F::kFormat, p.M, p.N, p.K);
  if (plan.split > 1 && ws == nullptr) {
    fprintf(stderr, "cs336: gemm_wqt split launch without a workspace\n");
    abort();
  }
  WqtParams q;
  q.g = p;
  if (!F::kRowScale) q.g.scale = nullptr;
  q.ws = plan.split > 1 ? ws : nullptr;
  q.ldws = wqt_ws_ld(p.N);
  q.tiles_m = (p.M + plan.bm - 1) / plan.bm;
  q.ktiles = (p.K + kWqtKTile - 1) / kWqtKTile;
  if (plan.bm == 128 && plan.bn == 128) launch_wqt<F, 128, 128>(q, plan.split, s);
  else if (plan.bm == 128) launch_wqt<F, 128, 64>(q, plan.split, s);
  else launch_wqt<F, 64, 64>(q, plan.split, s);
  if (plan.split > 1) {
    const int64_t threads = (int64_t)p.M * (q.ldws / 4);
    hipLaunchKernelGGL((wqt_reduce_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, q, plan.split);
  }
}

}  // namespace

bool gemm_wqt_ok(SkinnyFormat f, int64_t M, int64_t N, int64_t K, int64_t elem_size) {
  // 32-bit row / k indices in the kernel (row offsets are 64-bit): M + 128, N + 128, K + one k-tile and
  // the tile count must fit
  if (f != SkinnyFormat::E4M3 && f != SkinnyFormat::MXFP4) return false;
  const int kl = skinny_k_per_load(f);
  return elem_size == 2 && M >= kWqtMinM && M < (int64_t)1 << 24 && N >= 1 && N < (int64_t)1 << 30 && K >= kl && K % kl == 0 &&
         K < (int64_t)1 << 30 && wqt_tiles(M, N, 128, 128) < (int64_t)1 << 30;
}

void gemm_wqt(const SkinnyParams& p, float* ws, SkinnyFormat f, DType t, hipStream_t s) {
  const bool w4 = f == SkinnyFormat::MXFP4;
  if (f == SkinnyFormat::W16 || (t != DType::BF16 && t != DType::F16)) {
    fprintf(stderr, "cs336: gemm_wqt takes e4m3 / MXFP4 weights and bf16 / fp16 activations only\n");
    abort();
  }
  if (t == DType::BF16) w4 ? dispatch_wqt<W4<BF16>>(p, ws, s) : dispatch_wqt<W8<BF16>>(p, ws, s);
  else w4 ? dispatch_wqt<W4<F16>>(p, ws, s) : dispatch_wqt<W8<F16>>(p, ws, s);
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
