// Fused temperature / top-k sampler over one row of logits for MI355X: the whole of generate()'s
// topk -> masked_fill -> softmax -> multinomial chain in one launch, with the random number an input.
//
// Rule (cs336_systems/ops/sample.py states it in full): kept_i = x_i >= (k-th largest logit of the row),
// w_i = exp((x_i - max) / temperature) for kept i, S = sum w_i, and the token is the smallest kept i
// whose inclusive prefix sum of w exceeds u * S (the last kept i with w_i > 0 if rounding leaves none).
// The kernel holds no random-number generator: u comes from the caller, so the token is a pure
// function of the inputs, bit for bit (no float atomics; every sum below has one fixed order).
//
// One workgroup of 1024 threads per row. The batch is small (1-64 rows) and a row is 20-260 KB, so
// a row's latency is what counts, not the chip's throughput: 16 waves are the most loads one CU can
// keep in flight, and with one row per workgroup every reduction stays inside LDS. The row is read
// from L2 once per pass, in tiles of 1024 x 8 elements, thread t owning elements [8 t, 8 t + 8) of
// the tile (16-B loads for 16-bit logits, 2 x 16 B for fp32). Rows need not be 16-B aligned (a bf16
// row at V 50257 is not): the tiles are laid over the row from the 16-B boundary at or below its first
// element, so every group of 8 is aligned; the groups that straddle the row's ends (at most two) are
// read element by element with bounds checks, and positions outside the row count as -inf.
//
// Passes: (1) row max; (2) top_k > 1: the k-th largest value by radix select, 8 bits per pass from the
// top, over order-preserving keys of the RAW storage bits (16-bit keys for bf16 / fp16: 2 passes; 32-bit
// for fp32: 4), -0.0 canonicalised to +0.0; integer count histograms in LDS (8 interleaved copies, so
// that the few hot exponent bins of pass one spread over the banks); (3) the weights and S; (4) the
// tiles again, up to the one that holds the token. Sum order: a thread adds its 8 weights left to
// right, a wave adds its 64 thread sums by the xor butterfly, and ONE running sum R goes sequentially
// over (tile, wave). Pass 4 rebuilds the same R, so the first (tile, wave) step with R > u * S is
// found exactly (that wave's total is then > 0); inside that wave the 64 thread sums and then the 8
// weights of one thread are added sequentially onto R, first excess wins. Only the wave's butterfly
// total and its sequential chain may disagree in the last bit: then the wave's last positive weight
// is taken.
//
// sample_advance (p.step != nullptr) is the same body inside a captured decode step: u = u_table[s, b]
// with s = step[0], a finished row emits eos_id, tok[b] / out[b, s] / done[b] are written with plain
// stores by one thread, and s outside [0, S) stores nothing (the append kernels' rule for a slot
// outside the cache).
#include <cfloat>

#include "cs336/kernels.h"

namespace cs336 {
namespace {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / kWave;
constexpr int kE = 8;  // elements per thread per tile
constexpr int kSampleTile = kSampleThreads * kE;
constexpr int kBins = 256, kCopies = 8;

// Order-preserving unsigned key of an element's raw bits (sign-magnitude -> biased), and back.
template <typename T>
struct Key {
  typedef typename Elem<T>::storage S;
  static constexpr int bits = 8 * (int)sizeof(S);
  static constexpr uint32_t top = 1u << (bits - 1);
  static constexpr uint32_t all = bits == 32 ? 0xffffffffu : 0xffffu;
  static __device__ __forceinline__ uint32_t raw(S x) {
    if constexpr (sizeof(S) == 4) return __float_as_uint(x);
    else return (uint32_t)x;
  }
  static __device__ __forceinline__ uint32_t of(S x) {
    uint32_t b = raw(x);
    if (b == top) b = 0;  // -0.0 == +0.0
    return (b & top) ? (~b & all) : (b | top);
  }
  static __device__ __forceinline__ float value(uint32_t k) {
    const uint32_t b = (k & top) ? (k & ~top) : (~k & all);
    if constexpr (sizeof(S) == 4) return __uint_as_float(b);
    else return Elem<T>::to_f((S)b);
  }
};

// Elements [j0, j0 + 8) of the aligned virtual row vrow, whose positions [lo, hi) are the real row.
template <typename T>
__device__ __forceinline__ void load_group(const typename Elem<T>::storage* vrow, int j0, int lo, int hi,
                                           typename Elem<T>::storage (&r)[kE]) {
  typedef typename Elem<T>::storage S;
  if (j0 >= lo && j0 + kE <= hi) {
    if constexpr (sizeof(S) == 4) {
      const float4 a = *reinterpret_cast<const float4*>(vrow + j0);
      const float4 b = *reinterpret_cast<const float4*>(vrow + j0 + 4);
      r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
      r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    } else {
      const uint4 v = *reinterpret_cast<const uint4*>(vrow + j0);
      r[0] = (S)(v.x & 0xffff); r[1] = (S)(v.x >> 16);
      r[2] = (S)(v.y & 0xffff); r[3] = (S)(v.y >> 16);
      r[4] = (S)(v.z & 0xffff); r[5] = (S)(v.z >> 16);
      r[6] = (S)(v.w & 0xffff); r[7] = (S)(v.w >> 16);
    }
  } else {
    const S ninf = Elem<T>::from_f(-INFINITY);
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      const int j = j0 + e;
      r[e] = ninf;
      if (j >= lo && j < hi) r[e] = vrow[j];
    }
  }
}

// The thread's 8 weights of one tile and their left-to-right sum.
template <typename T>
__device__ __forceinline__ float tile_weights(const typename Elem<T>::storage* vrow, int j0, int lo, int hi, float m,
                                              float thr, float inv_t, float (&w)[kE]) {
  typename Elem<T>::storage r[kE];
  load_group<T>(vrow, j0, lo, hi, r);
  float ls = 0.f;
#pragma unroll
  for (int e = 0; e < kE; ++e) {
    const float x = Elem<T>::to_f(r[e]);
    w[e] = x >= thr ? __expf((x - m) * inv_t) : 0.f;
    ls += w[e];
  }
  return ls;
}

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
  const int lane = threadIdx.x % kWave;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(const SampleParams p) {
  typedef typename Elem<T>::storage S;
  typedef Key<T> K;
  __shared__ float red[kSampleWaves];
  __shared__ float wtot[2][kSampleWaves];
  __shared__ unsigned hist[kBins * kCopies];
  __shared__ unsigned wsum[4];
  __shared__ int sel[2];
  __shared__ int ired[kSampleWaves];
  __shared__ int res;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  int s = 0;
  float u;
  if (p.step) {
    s = p.step[0];
    if (s < 0 || s >= p.S) return;  // (the whole workgroup: nothing is stored)
    if (p.done[b]) {                // every thread reads done[b] before the first barrier; one writes it after the last
      if (tid == 0) {
        p.tok[b] = p.eos_id;
        p.out[(int64_t)b * p.S + s] = p.eos_id;
      }
      return;
    }
    u = p.u[(int64_t)s * p.B + b];
  } else {
    u = p.u[b];
  }
  if (tid == 0) res = 0;

  const S* row = static_cast<const S*>(p.logits) + (int64_t)b * p.row_stride;
  const int pad = (int)((reinterpret_cast<uintptr_t>(row) % 16) / sizeof(S));
  const S* vrow = row - pad;
  const int lo = pad, hi = pad + p.V;
  const int jt = tid * kE;

  // (1) the row max (NaNs are ignored by fmaxf)
  float m = -INFINITY;
  for (int t0 = 0; t0 < hi; t0 += kSampleTile) {
    S r[kE];
    load_group<T>(vrow, t0 + jt, lo, hi, r);
#pragma unroll
    for (int e = 0; e < kE; ++e) m = fmaxf(m, Elem<T>::to_f(r[e]));
  }
  m = block_max<kSampleThreads>(m, red);

  // (2) the threshold: -inf keeps everything, top_k 1 keeps the max, else the k-th largest value
  float thr = -INFINITY;
  if (p.top_k == 1) {
    thr = m;
  } else if (p.top_k > 1) {
    uint32_t prefix = 0, mask = 0;
    int k = p.top_k;  // < V: positions outside the row add -inf keys, below every k-th largest
    for (int shift = K::bits - 8; shift >= 0; shift -= 8) {
      for (int i = tid; i < kBins * kCopies; i += kSampleThreads) hist[i] = 0;
      __syncthreads();
      for (int t0 = 0; t0 < hi; t0 += kSampleTile) {
        S r[kE];
        load_group<T>(vrow, t0 + jt, lo, hi, r);
#pragma unroll
        for (int e = 0; e < kE; ++e) {
          const uint32_t key = K::of(r[e]);
          if ((key & mask) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * kCopies + (lane & (kCopies - 1))], 1u);
        }
      }
      __syncthreads();
      // thread t < 256 owns digit 255 - t: its inclusive scan counts the candidates with a digit >= its own
      unsigned c = 0, incl = 0;
      if (tid < kBins) {
#pragma unroll
        for (int i = 0; i < kCopies; ++i) c += hist[(kBins - 1 - tid) * kCopies + i];
        incl = wave_incl_scan(c);
        if (lane == kWave - 1) wsum[wave] = incl;
      }
      __syncthreads();
      if (tid < kBins) {
        for (int i = 0; i < wave; ++i) incl += wsum[i];
        const unsigned excl = incl - c;
        if (excl < (unsigned)k && (unsigned)k <= incl) {  // exactly one thread: 1 <= k <= candidates
          sel[0] = kBins - 1 - tid;
          sel[1] = k - (int)excl;
        }
      }
      __syncthreads();
      prefix |= (uint32_t)sel[0] << shift;
      mask |= 255u << shift;
      k = sel[1];
    }
    thr = K::value(prefix);
  }

  // (3) S: one running sum over (tile, wave), and the last position with a positive weight
  const float inv_t = p.inv_temperature;
  float R = 0.f;
  int last = -1, par = 0;
  for (int t0 = 0; t0 < hi; t0 += kSampleTile) {
    float w[kE];
    const float ls = tile_weights<T>(vrow, t0 + jt, lo, hi, m, thr, inv_t, w);
#pragma unroll
    for (int e = 0; e < kE; ++e)
      if (w[e] > 0.f) last = t0 + jt + e;
    const float wt = wave_sum(ls);
    if (lane == 0) wtot[par][wave] = wt;
    __syncthreads();  // (two buffers: the next tile's writes cannot pass this tile's reads)
#pragma unroll
    for (int i = 0; i < kSampleWaves; ++i) R += wtot[par][i];
    par ^= 1;
  }
  const float target = u * R;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, kWave));
  if (lane == 0) ired[wave] = last;

  // (4) the same chain again, up to the first (tile, wave) step that exceeds the target
  R = 0.f;
  int fwave = -1, ft0 = 0;
  float Rb = 0.f, ls = 0.f;
  float w[kE];
  for (int t0 = 0; t0 < hi && fwave < 0; t0 += kSampleTile) {  // (fwave is the same in every thread)
    ls = tile_weights<T>(vrow, t0 + jt, lo, hi, m, thr, inv_t, w);
    const float wt = wave_sum(ls);
    if (lane == 0) wtot[par][wave] = wt;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSampleWaves; ++i) {
      const float nR = R + wtot[par][i];
      if (fwave < 0 && nR > target) {
        fwave = i;
        Rb = R;
        ft0 = t0;
      }
      R = nR;
    }
    par ^= 1;
  }
  if (fwave >= 0) {
    if (wave == fwave) {
      // R_before + the thread sums, one after the other; the wave's total is > 0, so some sum is
      float A = Rb, base = Rb;
      int sl = -1, lastl = -1;
      for (int l = 0; l < kWave; ++l) {
        const float sv = __shfl(ls, l, kWave);
        const float nA = A + sv;
        if (sl < 0 && nA > target) {
          sl = l;
          base = A;
        }
        if (sv > 0.f) lastl = l;
        A = nA;
      }
      const bool fallback = sl < 0;
      if (fallback) sl = lastl;
      if (lane == sl) {
        int pick = -1, lastp = 0;
        float c = 0.f;
#pragma unroll
        for (int e = 0; e < kE; ++e) {
          c += w[e];
          if (pick < 0 && base + c > target) pick = e;
          if (w[e] > 0.f) lastp = e;
        }
        if (fallback || pick < 0) pick = lastp;
        res = ft0 + jt + pick - pad;
      }
    }
    __syncthreads();
  } else {
    __syncthreads();
    if (tid == 0) {
      int l2 = -1;
      for (int i = 0; i < kSampleWaves; ++i) l2 = max(l2, ired[i]);
      res = l2 >= 0 ? l2 - pad : 0;
    }
  }
  if (tid == 0) {
    const int64_t token = min(max(res, 0), p.V - 1);  // (a NaN row can leave anything: stay inside [0, V))
    if (p.step) {
      p.tok[b] = token;
      p.out[(int64_t)b * p.S + s] = token;
      if (p.eos_id >= 0 && token == p.eos_id) p.done[b] = 1;
    } else {
      p.out[b] = token;
    }
  }
}

}  // namespace

void sample(const SampleParams& p, DType t, hipStream_t s) {
  if (p.B == 0) return;
  switch (t) {
    case DType::F32: hipLaunchKernelGGL(sample_kernel<float>, dim3(p.B), dim3(kSampleThreads), 0, s, p); break;
    case DType::BF16: hipLaunchKernelGGL(sample_kernel<BF16>, dim3(p.B), dim3(kSampleThreads), 0, s, p); break;
    case DType::F16: hipLaunchKernelGGL(sample_kernel<F16>, dim3(p.B), dim3(kSampleThreads), 0, s, p); break;
  }
}

}  // namespace cs336
