// Device helpers shared by the decode-attention kernels (fa_decode.hip: one query row per
// (batch, head); fa_decode_chunk.hip: a tile of query rows): the row-per-lane-group geometry, 16-B
// row loads kept packed in registers, the DPP sum over a lane group and the online-softmax state of
// one lane. gfx950, wave64.
#pragma once

#include "cs336/kernels.h"

namespace cs336 {
namespace {

constexpr int kDecodeThreads = 256;
constexpr int kDecodeWaves = kDecodeThreads / kWave;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// lanes per row
__host__ __device__ constexpr int decode_group(int D) { return D <= 32 ? 4 : (D <= 64 ? 8 : 16); }
// rows per lane group and tile; two tiles (4U loads of 16 B) are in flight per lane
__host__ __device__ constexpr int decode_unroll(int es) { return es == 2 ? 4 : 2; }
__host__ __device__ constexpr int decode_tile(int D, int es) {
  return (kDecodeThreads / decode_group(D)) * decode_unroll(es);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// sum over the G lanes of a row group; every lane of the group gets the total
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_f32<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E>(v);  // quad_perm [2,3,0,1]
  if constexpr (G >= 8) v += dpp_f32<0x141>(v);   // row_half_mirror: the other quad of the 8 lanes
  if constexpr (G >= 16) v += dpp_f32<0x140>(v);  // row_mirror: the other half of the 16 lanes
  return v;
}

struct Chunk8 {
  float f[8];
};

// 8 consecutive elements as loaded: 16 B of a 16-bit type, 32 B of fp32
template <typename T, int BYTES = sizeof(typename Elem<T>::storage)>
struct Raw8 {
  uint4 a;
};
template <typename T>
struct Raw8<T, 4> {
  uint4 a, b;
};

// p is 16-B aligned
template <typename T>
__device__ __forceinline__ Raw8<T> load_raw(const typename Elem<T>::storage* p) {
  Raw8<T> r;
  r.a = *reinterpret_cast<const uint4*>(p);
  if constexpr (sizeof(typename Elem<T>::storage) == 4) r.b = *reinterpret_cast<const uint4*>(p + 4);
  return r;
}

template <typename T>
__device__ __forceinline__ Chunk8 unpack(const Raw8<T>& r) {
  Chunk8 c;
  if constexpr (sizeof(typename Elem<T>::storage) == 4) {
    c.f[0] = __uint_as_float(r.a.x); c.f[1] = __uint_as_float(r.a.y);
    c.f[2] = __uint_as_float(r.a.z); c.f[3] = __uint_as_float(r.a.w);
    c.f[4] = __uint_as_float(r.b.x); c.f[5] = __uint_as_float(r.b.y);
    c.f[6] = __uint_as_float(r.b.z); c.f[7] = __uint_as_float(r.b.w);
  } else {
    typedef typename Elem<T>::storage S;
    const uint32_t w[4] = {r.a.x, r.a.y, r.a.z, r.a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c.f[2 * i] = Elem<T>::to_f((S)(w[i] & 0xffff));
      c.f[2 * i + 1] = Elem<T>::to_f((S)(w[i] >> 16));
    }
  }
  return c;
}

template <typename T>
__device__ __forceinline__ Chunk8 load8(const typename Elem<T>::storage* p) {
  return unpack<T>(load_raw<T>(p));
}

template <typename T>
__device__ __forceinline__ void store8(typename Elem<T>::storage* p, const Chunk8& c) {
  if constexpr (sizeof(typename Elem<T>::storage) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(c.f[0], c.f[1], c.f[2], c.f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(c.f[4], c.f[5], c.f[6], c.f[7]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = (uint32_t)Elem<T>::from_f(c.f[2 * i]) | ((uint32_t)Elem<T>::from_f(c.f[2 * i + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// running softmax state of one lane: max and sum of its group's rows (exp2 domain), 8 output columns
struct Online {
  float m, l;
  float acc[8];
};

// (m, l, acc) <- merge with (m2, l2, acc2); a side with m = -inf has weight exp2(-inf) = 0
__device__ __forceinline__ void online_merge(Online& s, float m2, float l2, const float* acc2) {
  const float M = fmaxf(s.m, m2);
  const float msub = M == -INFINITY ? 0.f : M;  // both empty: nothing is inf - inf
  const float a = __builtin_amdgcn_exp2f(s.m - msub), b = __builtin_amdgcn_exp2f(m2 - msub);
  s.l = s.l * a + l2 * b;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.acc[i] = s.acc[i] * a + acc2[i] * b;
  s.m = M;
}

}  // namespace
}  // namespace cs336
