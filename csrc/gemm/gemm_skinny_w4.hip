// Skinny-M GEMM for decode with OCP MXFP4 weights (W4A16): the policy W4 of the one kernel template in
// gemm_skinny.h, 6 kernels (bf16 / fp16 activations x 1 / 2 / 4 W tiles per wave;
// tests/test_skinny_w4_resources.py pins their count and registers).
//
//   out[M,N] = round_T( fp32( x[M,K] · dq[N,K]ᵀ ) ),  dq[n,k] = e2m1(code[n,k]) * 2^(scale[n, k/32] - 127)
//
// W is (N, K/2) bytes, the code of k = 2j in bits 3:0 of byte j and of k = 2j+1 in bits 7:4; scale is
// (N, K/32) e8m0 bytes with a row stride >= K/32. K % 32 == 0. What the format changes in the kernel:
//
//   * k ownership. A 16-byte W load is 32 k of one row: exactly one MX block. Lane (r, g) = (l & 15,
//     l >> 4) owns block g of a 128-k k-block of W row r (ONE 16-B load; a 64-byte run of the row per
//     instruction, as in the other formats) and the same 32 k of batch row r: FOUR 16-B loads of x, 64
//     contiguous bytes.
//   * Conversion. Dword d of the load (k = 8d .. 8d+7 of the lane's 32) becomes the A operand of one
//     MFMA by four v_cvt_scalef32_pk_{bf16,f16}_fp4, byte selects 0..3, each giving the low and then
//     the high nibble of its byte; x chunk d is the B operand. A and B put the same k into the same
//     slot, which is all the MFMA's sum needs. The block's scale is the instruction's fp32 operand
//     (`byte << 23` is 2^(byte - 127) for bytes 1..254), so dequantization costs one shift per load and
//     there is no epilogue scale. 16 conversions and 4 MFMAs per load. For the bytes the quantizer
//     emits (scale exponents -23 .. 13) every code x 2^X is exact in bf16 and in fp16, subnormals
//     included, so the conversion adds no error.
//   * Scale bytes: one byte load per W load, at block index 4 * (k-block) + g of the lane's scale row
//     (rows >= N clamped to N - 1 like the W rows). Per load instruction the 4 lane groups of a row read
//     4 consecutive bytes; the rows of a scale matrix are K/32 bytes (50 on xl: not a multiple of 4, so
//     a dword per lane would be misaligned and could pass the tensor's end), and a tile's scales are
//     1/16 of its W bytes, re-read from L2 lines the first access brought. Byte loads need no layout of
//     their own, take any row stride (padded rows stay possible), and follow the file's edge rule
//     unchanged. The permuted ownership (a lane owning U consecutive blocks so that one dword carries a
//     register set's scales, at 16-B instead of 64-B runs per row and instruction) and padded scale
//     rows were not measured.
//   * K tail: K % 32 == 0, so a lane's load is wholly inside or outside K; an outside load reads the
//     row's first 16 bytes and first scale byte (valid memory) and is replaced by zeros and the unit
//     scale by select.
//   * Registers. x per k is four times W's bytes, so x fragments set the budget: U (k-blocks per
//     register set) is 2 / 2 / 4 for 4 / 2 / 1 W tiles per wave (skinny_u), which covers the same k per
//     set as the FP8 format (256 / 256 / 512) with the same x registers and half the W registers plus
//     TN x U scale bytes. 0 B scratch.
//
// Everything else -- clamped W / batch rows, in-workgroup split-K through LDS in wave order (no
// atomics, bitwise reproducible), one rounding to the output type, the plan's tile thresholds -- is the
// template's.
#include "gemm_skinny.h"

namespace cs336 {

void gemm_skinny_w4(const SkinnyParams& p, DType t, hipStream_t s) {
  if (t == DType::BF16) dispatch<W4<BF16>>(p, s);
  else if (t == DType::F16) dispatch<W4<F16>>(p, s);
  else {
    fprintf(stderr, "cs336: gemm_skinny_w4 takes bf16 / fp16 activations only\n");
    abort();
  }
  CS336_HIP_CHECK(hipGetLastError());
}

}  // namespace cs336
