// Pieces shared by the one-kernel FlashAttention-2 backwards (fa_bwd_fused.hip, fa_bwd_hs.hip,
// fa_bwd_kp.hip). All three keep a wave's 32 keys on the MFMA lane, sweep 64-row query slices and form
// the same five products per tile pair; what they share here are the layout facts -- the per-lane
// fragment offsets, the accumulator pack order behind the dSᵀ write and the dK / dV stores, and
// the row_perm order of the row constants. The tile loops (read / MFMA order, DMA rings, vmcnt
// accounting) stay with each kernel. Transposed reads: tr_offsets / lds_tr_read in fa_common.h.
#pragma once

#include "fa_common.h"

namespace cs336 {
namespace fa {

constexpr int kBwdBQ = 64;  // query slice of all three kernels (and of the row-constant layout)

// Row-fragment offsets (ds_read_b128, A/B operand with the image row on the lane): row l32 = lane&31,
// chunk 2ks + hh (hh = lane>>5) of an image with RB-byte rows, from a row base that is a multiple of
// 16 rows (the swizzle is then the lane's and the base an immediate offset).
template <int RB, int NKS>
__host__ __device__ __forceinline__ void row_offsets(int l32, int hh, uint32_t (&roff)[NKS]) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) roff[ks] = (uint32_t)(l32 * RB + (((2 * ks + hh) ^ swz<RB>(l32)) << 4));
}

// acc += a·b over the 8 16-bit elements of one 16-byte chunk, in memory order (word 0 low, word 0
// high, word 1 low, ...): the order every delta = rowsum(dO·O) of these kernels is summed in
template <typename T>
__device__ __forceinline__ float dot8(uint4 a, uint4 b, float acc) {
  typedef typename Elem<T>::storage S;
  const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    acc = fmaf(Elem<T>::to_f((S)(wa[w] & 0xffff)), Elem<T>::to_f((S)(wb[w] & 0xffff)), acc);
    acc = fmaf(Elem<T>::to_f((S)(wa[w] >> 16)), Elem<T>::to_f((S)(wb[w] >> 16)), acc);
  }
  return acc;
}

// Row constants of every 64-row slice for the main kernels' LDS-DMA: 128 floats per slice, -lse·log2e
// then -delta (delta = rowsum(dO·O)), each in row_perm order. block = (head, slice); 4 threads per row.
// CONTIG: thread k sums the 16-B chunks 2k, 2k+1 of d (d 64; the order of fa_bwd_hs.hip's in-kernel
// delta, which must give the same bits), else chunks k, k+4, ... (any d). ZERO_ACC: also zero the
// slice's rows of the fp32 dQ accumulator (fa_bwd_kp.hip's atomic form).
template <typename T, int D, bool CONTIG, bool ZERO_ACC>
__global__ __launch_bounds__(256) void fa_bwd_rowc_prep(const AttnBwdParams bp, float* __restrict__ rowc,
                                                        float* __restrict__ acc) {
  static_assert(!CONTIG || D == 64, "two contiguous chunks per thread cover d 64");
  typedef typename Elem<T>::storage S;
  const int N = bp.f.Nq, nqs = N / kBwdBQ;
  const int bh = blockIdx.x / nqs, s = blockIdx.x % nqs;
  const int b = bh / bp.f.H, h = bh % bp.f.H;
  const int tid = threadIdx.x, r = tid >> 2, k = tid & 3, row = s * kBwdBQ + r;
  const S* o = (const S*)bp.f.o + b * bp.f.o_sb + h * bp.f.o_sh + (int64_t)row * bp.f.o_sn;
  const S* g = (const S*)bp.dout + b * bp.do_sb + h * bp.do_sh + (int64_t)row * bp.do_sn;
  float dsum = 0.f;
#pragma unroll
  for (int c = CONTIG ? 2 * k : k; c < (CONTIG ? 2 * k + 2 : D / 8); c += CONTIG ? 1 : 4)
    dsum = dot8<T>(*reinterpret_cast<const uint4*>(o + 8 * c), *reinterpret_cast<const uint4*>(g + 8 * c), dsum);
  dsum += __shfl_xor(dsum, 1, 64);
  dsum += __shfl_xor(dsum, 2, 64);
  if (k == 0) {
    float* rc = rowc + ((int64_t)bh * nqs + s) * 128;
    rc[row_perm(r)] = -bp.f.lse[(int64_t)bh * N + row] * kLog2e;
    rc[64 + row_perm(r)] = -dsum;
  }
  if constexpr (ZERO_ACC) {
    float4* z = reinterpret_cast<float4*>(acc + ((int64_t)bh * N + s * kBwdBQ) * D);
    for (int i = tid; i < kBwdBQ * D / 4; i += 256) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// dSᵀ row of one key (drow: the key's 128-B image row + 8 hh, swl its swizzle): the fragment sf[s2]
// holds the 32-query tile t's two 4-query halves q = 32t + 16s2 + 4hh + 0..3 and the same + 8
// (pack_acc order), one 8-B write each
template <typename F>
__device__ __forceinline__ void store_dst(char* drow, int swl, int t, const F (&sf)[2]) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const uint4 w = __builtin_bit_cast(uint4, sf[s2]);
    const int ch = 4 * t + 2 * s2;
    *reinterpret_cast<uint2*>(drow + ((ch ^ swl) << 4)) = make_uint2(w.x, w.y);
    *reinterpret_cast<uint2*>(drow + (((ch + 1) ^ swl) << 4)) = make_uint2(w.z, w.w);
  }
}

// dK (x scale, inverse RoPE at position pos when ROPE) and dV of one key into its rows rk / rv:
// lane = key, registers 4g4..4g4+3 of d tile dt = d 32dt + 8g4 + 4hh + 0..3, d = 32 NDT (no pad
// columns: fa_bwd_kp.hip, which has them at d 80, keeps its own store).
template <typename T, int NDT, bool ROPE>
__device__ __forceinline__ void store_dkdv(const f32x16 (&dk)[NDT], const f32x16 (&dv)[NDT],
                                           typename Elem<T>::storage* rk, typename Elem<T>::storage* rv, float sc,
                                           const Rope& rope, int64_t pos, int hh) {
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = 32 * dt + 8 * g4 + 4 * hh;
      float k0 = dk[dt][4 * g4] * sc, k1 = dk[dt][4 * g4 + 1] * sc, k2 = dk[dt][4 * g4 + 2] * sc,
            k3 = dk[dt][4 * g4 + 3] * sc;
      if constexpr (ROPE) rope_inv4(k0, k1, k2, k3, rope, pos, d);
      store4<T>(rk + d, make_float4(k0, k1, k2, k3));
      store4<T>(rv + d, make_float4(dv[dt][4 * g4], dv[dt][4 * g4 + 1], dv[dt][4 * g4 + 2], dv[dt][4 * g4 + 3]));
    }
}

}  // namespace fa
}  // namespace cs336
