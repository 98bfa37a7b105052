// The GEMM kernel template (gemm_kernel.hpp) on fp8 (e4m3) operands.
#include "gemm_kernel.hpp"

template int gemm_launch_fmt<GemmFmt::FP8>(int epi, const GemmBf16Args& a, hipStream_t st);
