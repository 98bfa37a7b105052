// The GEMM kernel template (gemm_kernel.hpp) on f16f8 rows (fp16 high halves + fp8 cross terms): the f16f8 mode.
#include "gemm_kernel.hpp"

template int gemm_launch_fmt<GemmFmt::F16F8>(int epi, const GemmBf16Args& a, hipStream_t st);
