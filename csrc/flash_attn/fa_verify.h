// What the verify-attention kernels share (fa_verify.hip on 16-bit caches, fa_verify_kv8.hip on the FP8
// format): the 16x16x32 MFMA, the combine over the four lane groups of a query, and the row address
// policies. gfx950, wave64.
#pragma once

#include "fa_common.h"

namespace cs336 {
namespace fa {

typedef __attribute__((ext_vector_type(4))) float f32x4;

template <typename T> struct Mma32;
template <> struct Mma32<BF16> {
  static __device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mma32<F16> {
  static __device__ __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// lane l's value combined with those of lanes l ^ 16, l ^ 32, l ^ 48 (the four lane groups of a query)
__device__ __forceinline__ float xrow_max(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xrow_sum(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- row address policies: element offset of cached row `key` (K and V planes) -------------------
template <typename P>
struct VerifyRows;

template <>
struct VerifyRows<VerifyParams> {
  static constexpr bool kPaged = false;
  int64_t k0, v0, k_sn, v_sn;
  __device__ __forceinline__ VerifyRows(const VerifyParams& p, int b, int h)
      : k0((int64_t)b * p.k_sb + (int64_t)h * p.k_sh), v0((int64_t)b * p.v_sb + (int64_t)h * p.v_sh), k_sn(p.k_sn),
        v_sn(p.v_sn) {}
  __device__ __forceinline__ int page(int) const { return 0; }
  __device__ __forceinline__ int64_t k(int key, int) const { return k0 + (int64_t)key * k_sn; }
  __device__ __forceinline__ int64_t v(int key, int) const { return v0 + (int64_t)key * v_sn; }
};

template <>
struct VerifyRows<VerifyPagedParams> {
  static constexpr bool kPaged = true;
  const int* tbl;
  int64_t k0, v0, k_sp, v_sp, k_sn, v_sn;
  int lg, pmask, last_page;
  __device__ __forceinline__ VerifyRows(const VerifyPagedParams& p, int b, int h)
      : tbl(p.table + (int64_t)b * p.table_sb), k0((int64_t)h * p.k_sh), v0((int64_t)h * p.v_sh), k_sp(p.k_sp),
        v_sp(p.v_sp), k_sn(p.k_sn), v_sn(p.v_sn), lg(p.lg_page), pmask((1 << p.lg_page) - 1),
        last_page(p.num_pages - 1) {}
  // the raw table entry of `key`'s page (clamped at its use: nothing here waits for the load)
  __device__ __forceinline__ int page(int key) const { return tbl[key >> lg]; }
  __device__ __forceinline__ int64_t k(int key, int pg) const {
    const int id = pg < 0 ? 0 : (pg > last_page ? last_page : pg);
    return k0 + (int64_t)id * k_sp + (int64_t)(key & pmask) * k_sn;
  }
  __device__ __forceinline__ int64_t v(int key, int pg) const {
    const int id = pg < 0 ? 0 : (pg > last_page ? last_page : pg);
    return v0 + (int64_t)id * v_sp + (int64_t)(key & pmask) * v_sn;
  }
};

}  // namespace fa
}  // namespace cs336
