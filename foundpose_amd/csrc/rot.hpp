// fp64 3-vector and rotation helpers shared by the pose kernels (pnp.hip, refine.hip).
#pragma once
#include "common.hpp"

FP_DEVICE void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
FP_DEVICE double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// E = exp([w]x) = I + a [w]x + b [w]x^2 (Rodrigues, series near 0), row-major
FP_DEVICE void rot_exp(const double* w, double* E) {
  const double th2 = dot3(w, w), th = sqrt(th2);
  double a, b;
  if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
  else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double K2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K2[i * 3 + j] = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
  for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

// exp of a rotation vector times R (left perturbation)
FP_DEVICE void rot_update(const double* w, const double* R, double* Rn) {
  double E[9];
  rot_exp(w, E);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = E[i * 3 + 0] * R[0 * 3 + j] + E[i * 3 + 1] * R[1 * 3 + j] + E[i * 3 + 2] * R[2 * 3 + j];
}
