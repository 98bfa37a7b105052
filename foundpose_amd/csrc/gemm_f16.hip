// The GEMM kernel template (gemm_kernel.hpp) on IEEE fp16 operands: the "f16" mode.
#include "gemm_kernel.hpp"

template int gemm_launch_fmt<GemmFmt::F16>(int epi, const GemmBf16Args& a, hipStream_t st);
