// The GEMM kernel template (gemm_kernel.hpp) on bf16 operands.
#include "gemm_kernel.hpp"

template int gemm_launch_fmt<GemmFmt::BF16>(int epi, const GemmBf16Args& a, hipStream_t st);
