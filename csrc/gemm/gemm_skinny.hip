// Skinny-M GEMM for decode, 16-bit and FP8 weights: y[M,N] = x[M,K] · W[N,K]ᵀ with 1 <= M <= 16. The
// kernel template, what it does per byte of W and why, the format policies and the plan are in
// gemm_skinny.h; this file holds the 12 instantiations of W16 and W8 (bf16 / fp16 activations x 1 / 2 /
// 4 W tiles per wave; tests/test_skinny_resources.py pins their count and registers) and the entry
// points. The MXFP4 format's 6 are in gemm_skinny_w4.hip.
#include "gemm_skinny.h"

namespace cs336 {

bool gemm_skinny_ok(SkinnyFormat f, int64_t M, int64_t N, int64_t K, int64_t elem_size) {
  // 32-bit row / k indices in the kernel (row offsets are 64-bit): N + 64 and K + 8 k-blocks must fit
  const int kl = skinny_k_per_load(f);
  return elem_size == 2 && M >= 1 && M <= 16 && N >= 1 && N < (int64_t)1 << 30 && K >= kl && K % kl == 0 &&
         K < (int64_t)1 << 30;
}

void gemm_skinny(const SkinnyParams& p, SkinnyFormat f, DType t, hipStream_t s) {
  if (f == SkinnyFormat::MXFP4) return gemm_skinny_w4(p, t, s);  // gemm_skinny_w4.hip
  const bool w8 = f == SkinnyFormat::E4M3;
  if (t == DType::BF16) w8 ? dispatch<W8<BF16>>(p, s) : dispatch<W16<BF16>>(p, s);
  else if (t == DType::F16) w8 ? dispatch<W8<F16>>(p, s) : dispatch<W16<F16>>(p, s);
  else {
    fprintf(stderr, "cs336: gemm_skinny takes bf16 / fp16 activations only\n");
    abort();
  }
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
