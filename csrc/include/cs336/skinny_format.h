// Weight formats of the skinny-M decode GEMM (csrc/gemm/gemm_skinny.h). A header of its own, free of HIP
// types, so that the launch plan (csrc/gemm/skinny_plan.h) compiles with a plain host compiler.
#pragma once

namespace cs336 {

enum class SkinnyFormat { W16, E4M3, MXFP4 };

}  // namespace cs336
