// The GEMM kernel template (gemm_kernel.hpp) on bf16 operands.
#include "gemm_kernel.hpp"

int gemm_resid_tile_rows(int m_valid, int n, int cus) { return resid_tile_rows(m_valid, n, cus); }
int gemm_wide_tile_rows(int m, int m_valid, int n, int cus) { return wide_tile_rows(m, m_valid, n, cus); }

template int gemm_launch_fmt<GemmFmt::BF16>(int epi, const GemmBf16Args& a, hipStream_t st);
