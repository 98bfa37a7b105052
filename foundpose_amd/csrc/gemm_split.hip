// The GEMM kernel template (gemm_kernel.hpp) on split-fp16 operands: the f16x3 mode.
#include "gemm_kernel.hpp"

template int gemm_launch_fmt<GemmFmt::F16X3>(int epi, const GemmBf16Args& a, hipStream_t st);
