// What the two hypothesis verifiers share (verify.hip; mask_verify.hip, section 18 step 1): the pose in the
// frame camera, the square of the model's projected bounding sphere divided into G x G cells, and a point's cell in it.  fp64, every step
// one rounded operation in the order section 17 states: each function turns FMA contraction off for itself.  verify.hip uses the types,
// to_camera and project; its set-up stays written out in its kernel (calling frame_pose / sphere_grid there changed the kernel's register
// allocation, and section 17's resource table is kept as measured), so frame_pose and sphere_grid restate those lines for mask_verify.hip.
#pragma once
#include "common.hpp"

namespace {

constexpr int PV_THREADS = 256;
constexpr int PV_MIN_GRID = 8;
constexpr int PV_MAX_GRID = 128;

struct FramePose {
  double R[9];
  double t[3];
};

struct CellGrid {
  double fx, fy, cx, cy;
  double u0, v0, h;  // the square's corner (u_c - r_px, v_c - r_px) and the cell side
  int G;
};

// X -> the frame camera: products summed k ascending, then + t
FP_DEVICE void to_camera(const FramePose& P, const double* X, double* Xc) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i) Xc[i] = ((P.R[i * 3 + 0] * X[0] + P.R[i * 3 + 1] * X[1]) + P.R[i * 3 + 2] * X[2]) + P.t[i];
}

// a point with z > 1 -> its pixel coordinates and its cell (a NaN coordinate lands in cell 0: fmax / fmin drop it)
FP_DEVICE int project(const CellGrid& g, const double* Xc, double* u, double* v) {
#pragma clang fp contract(off)
  *u = g.fx * Xc[0] / Xc[2] + g.cx;
  *v = g.fy * Xc[1] / Xc[2] + g.cy;
  const double top = (double)(g.G - 1);
  const int ix = (int)fmin(fmax(floor((*u - g.u0) / g.h), 0.0), top);
  const int iy = (int)fmin(fmax(floor((*v - g.v0) / g.h), 0.0), top);
  return iy * g.G + ix;
}

// R_f = A R, t_f = A t (A [9], R [9], t [3] row-major)
FP_DEVICE void frame_pose(const double* A, const double* R, const double* t, FramePose& P) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P.R[i * 3 + j] = (A[i * 3 + 0] * R[0 * 3 + j] + A[i * 3 + 1] * R[1 * 3 + j]) + A[i * 3 + 2] * R[2 * 3 + j];
    P.t[i] = (A[i * 3 + 0] * t[0] + A[i * 3 + 1] * t[1]) + A[i * 3 + 2] * t[2];
  }
}

// the grid of the sphere (c, rho) seen at P by the camera cam = (fx, fy, cx, cy); false when C.z <= rho + 1 (a NaN pose too): g.u0, g.v0
// and g.h are then not set.  *rpx: the square's half side in pixels.
FP_DEVICE bool sphere_grid(const FramePose& P, const double* cam, const double* c, double rho, int G, CellGrid& g, double* rpx) {
#pragma clang fp contract(off)
  g.fx = cam[0]; g.fy = cam[1]; g.cx = cam[2]; g.cy = cam[3];
  g.G = G;
  double C[3];
  to_camera(P, c, C);
  if (!(C[2] > rho + 1.0)) return false;
  const double uc = g.fx * C[0] / C[2] + g.cx, vc = g.fy * C[1] / C[2] + g.cy;
  *rpx = fmax(g.fx, g.fy) * rho / (C[2] - rho);
  g.u0 = uc - *rpx;
  g.v0 = vc - *rpx;
  g.h = 2.0 * *rpx / (double)g.G;
  return true;
}

}  // namespace
