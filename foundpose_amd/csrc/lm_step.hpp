// The Levenberg-Marquardt step shared by the pose refinements (refine.hip, depth_refine.hip; DESIGN.md sections 11 and 14):
// the damped 6x6 solve and the proposal of the next trial pose on a RefineState.  One lane of the solve kernel runs it.
// The functions are defined here, at global scope, without `static` or a template: that is safe only because FP_DEVICE is
// __device__ __forceinline__ (every use is inlined, no symbol is emitted twice).  Keep them FP_DEVICE.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "rot.hpp"

// (H + lam diag(H)) d = -g by Cholesky; false if a pivot is not > 0 (or not finite)
FP_DEVICE bool lm_solve(const double* H, const double* g, double lam, double* d) {
  double L[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) { L[j][i] = H[k]; L[i][j] = H[k]; }
  for (int i = 0; i < 6; ++i) L[i][i] = L[i][i] + lam * L[i][i];
  for (int j = 0; j < 6; ++j) {
    double dj = L[j][j];
    for (int m = 0; m < j; ++m) dj -= L[j][m] * L[j][m];
    if (!(dj > 0.0) || !(dj < INFINITY)) return false;
    const double ljj = sqrt(dj);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
      for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
      L[i][j] = v / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = -g[i];
    for (int m = 0; m < i; ++m) v -= L[i][m] * y[m];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int m = i + 1; m < 6; ++m) v -= L[m][i] * d[m];
    d[i] = v / L[i][i];
  }
  return true;
}

FP_DEVICE void lm_stop(RefineState& s) { s.active = 0; s.pending = 0; }

// next trial pose from the current system; a failed factorisation is a rejected step (one iteration, lam x 10)
FP_DEVICE void lm_propose(RefineState& s, int iters) {
  for (int k = 0; k <= iters && s.active; ++k) {
    if (s.it >= iters) { lm_stop(s); return; }
    double d[6];
    const bool ok = lm_solve(s.H, s.g, s.lam, d);
    s.it += 1;
    if (ok) {
      double E[9];
      rot_exp(d, E);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.Rt[i * 3 + j] = E[i * 3 + 0] * s.R[0 * 3 + j] + E[i * 3 + 1] * s.R[1 * 3 + j] + E[i * 3 + 2] * s.R[2 * 3 + j];
      for (int i = 0; i < 3; ++i) s.tt[i] = E[i * 3 + 0] * s.t[0] + E[i * 3 + 1] * s.t[1] + E[i * 3 + 2] * s.t[2] + d[3 + i];
      s.pending = 1;
      return;
    }
    s.lam *= 10.0;
    if (s.lam > 1e12) { lm_stop(s); return; }
  }
}
