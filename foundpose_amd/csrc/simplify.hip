// Mesh simplification by vertex clustering with quadric error positions (simplify.py; tests/simplify_ref.py
// restates both kernels operation for operation).
//
// mesh_cell_keys_kernel   one thread per vertex: the cell of a uniform grid the vertex falls into, as one int64 key.
// mesh_cluster_kernel     one wave per occupied cell: the cell's vertex records (position, colour) and corner records (the plane quadric
//                         of the face the corner belongs to) are summed in a fixed order -- lane l takes records l, l + 64, ... in
//                         ascending order, then the xor butterfly of common.hpp's wave_sum -- and the cell's vertex is placed where the
//                         summed quadric is smallest, within the eigenvalues that are kept (Lindstrom's out-of-core simplification).
//
// Everything is fp64 and every operation is rounded on its own (rounded.hpp; contraction is off for the whole file as well, as in tsdf.hip).
// No atomics, no shared memory, and a cell reads its own records only: its outputs do not depend on what else is in the launch.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int MESH_THREADS = 256;
constexpr int MESH_WAVES = MESH_THREADS / 64;
constexpr int MESH_JACOBI_SWEEPS = 30;

// floor((x - o) / c) clamped to [0, n - 1]; a NaN lands in cell 0, so no key leaves the grid
FP_DEVICE int grid_index(float x, double o, double c, int n) {
  const double g = ddiv(dsub((double)x, o), c);
  if (!(g >= 0.0)) return 0;
  if (g >= (double)n) return n - 1;
  return (int)floor(g);
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_cell_keys_kernel(MeshKeysArgs a) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= a.num_vertices) return;
  const int i = grid_index(a.verts[3 * v], a.grid.ox, a.grid.c, a.grid.nx);
  const int j = grid_index(a.verts[3 * v + 1], a.grid.oy, a.grid.c, a.grid.ny);
  const int k = grid_index(a.verts[3 * v + 2], a.grid.oz, a.grid.c, a.grid.nz);
  a.keys[v] = ((long long)k * a.grid.ny + j) * a.grid.nx + i;
}

FP_DEVICE double wave_sum_f64(double v) {   // common.hpp's wave_sum on doubles
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = dadd(v, __shfl_xor(v, o, 64));
  return v;
}

// One Jacobi rotation of the pair (P, R), the scheme of depth_proposals.hip's jacobi3_smallest: columns, then rows, then the vectors.
template <int P, int R>
FP_DEVICE void jacobi_rotate(double* M, double* V) {
  const double apr = M[P * 3 + R];
  if (apr == 0.0) return;
  const double theta = ddiv(dsub(M[R * 3 + R], M[P * 3 + P]), dmul(2.0, apr));
  const double tt = ddiv(theta >= 0.0 ? 1.0 : -1.0, dadd(fabs(theta), __dsqrt_rn(dadd(dmul(theta, theta), 1.0))));
  const double c = ddiv(1.0, __dsqrt_rn(dadd(dmul(tt, tt), 1.0))), s = dmul(tt, c);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mkp = M[k * 3 + P], mkr = M[k * 3 + R];
    M[k * 3 + P] = dsub(dmul(c, mkp), dmul(s, mkr));
    M[k * 3 + R] = dadd(dmul(s, mkp), dmul(c, mkr));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mpk = M[P * 3 + k], mrk = M[R * 3 + k];
    M[P * 3 + k] = dsub(dmul(c, mpk), dmul(s, mrk));
    M[R * 3 + k] = dadd(dmul(s, mpk), dmul(c, mrk));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k * 3 + P], vkr = V[k * 3 + R];
    V[k * 3 + P] = dsub(dmul(c, vkp), dmul(s, vkr));
    V[k * 3 + R] = dadd(dmul(s, vkp), dmul(c, vkr));
  }
}

// Cyclic Jacobi on the symmetric M: on return its diagonal holds the eigenvalues and column j of V the vector of eigenvalue j.
FP_DEVICE void jacobi3(double* M, double* V) {
#pragma unroll
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < MESH_JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double sq = dmul(M[i], M[i]);
      all = dadd(all, sq);
      if (i % 4 != 0) off = dadd(off, sq);
    }
    if (!(off > dmul(1e-30, all))) break;
    jacobi_rotate<0, 1>(M, V);
    jacobi_rotate<0, 2>(M, V);
    jacobi_rotate<1, 2>(M, V);
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_cluster_kernel(MeshClusterArgs a) {
  const long long cell = (long long)blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
  if (cell >= a.num_cells) return;   // whole waves leave together
  const int lane = threadIdx.x & 63;

  // ---- vertex records: positions and colours.  A range or an id outside the arrays is never read.
  long long vb = a.vert_begin[cell], ve = a.vert_begin[cell + 1];
  vb = vb < 0 ? 0 : vb, ve = ve > a.num_vertices ? a.num_vertices : ve;
  double sp[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
  for (long long r = vb + lane; r < ve; r += 64) {
    const long long v = a.vert_order[r];
    if (v < 0 || v >= a.num_vertices) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sp[k] = dadd(sp[k], (double)a.verts[3 * v + k]);
      sc[k] = dadd(sc[k], (double)a.colors[3 * v + k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) sp[k] = wave_sum_f64(sp[k]), sc[k] = wave_sum_f64(sc[k]);

  // ---- corner records: the quadric of the corner's face, its vertices in the face's own order
  const long long corners = 3 * a.num_faces;
  long long cb = a.corner_begin[cell], ce = a.corner_begin[cell + 1];
  cb = cb < 0 ? 0 : cb, ce = ce > corners ? corners : ce;
  double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long r = cb + lane; r < ce; r += 64) {
    const long long corner = a.corner_order[r];
    if (corner < 0 || corner >= corners) continue;
    const int* f = a.faces + 3 * (corner / 3);
    const int i0 = f[0], i1 = f[1], i2 = f[2];
    if (i0 < 0 || i0 >= a.num_vertices || i1 < 0 || i1 >= a.num_vertices || i2 < 0 || i2 >= a.num_vertices) continue;
    const double p0x = a.verts[3ll * i0], p0y = a.verts[3ll * i0 + 1], p0z = a.verts[3ll * i0 + 2];
    const double ux = dsub((double)a.verts[3ll * i1], p0x), uy = dsub((double)a.verts[3ll * i1 + 1], p0y), uz = dsub((double)a.verts[3ll * i1 + 2], p0z);
    const double vx = dsub((double)a.verts[3ll * i2], p0x), vy = dsub((double)a.verts[3ll * i2 + 1], p0y), vz = dsub((double)a.verts[3ll * i2 + 2], p0z);
    const double mx = dsub(dmul(uy, vz), dmul(uz, vy)), my = dsub(dmul(uz, vx), dmul(ux, vz)), mz = dsub(dmul(ux, vy), dmul(uy, vx));
    const double L = __dsqrt_rn(sqdist(mx, my, mz));
    if (!(L > 0.0)) continue;
    const double nx = ddiv(mx, L), ny = ddiv(my, L), nz = ddiv(mz, L);
    const double w = dmul(0.5, L);
    const double d = -dot3(nx, ny, nz, p0x, p0y, p0z);
    const double wx = dmul(w, nx), wy = dmul(w, ny), wz = dmul(w, nz);
    q[0] = dadd(q[0], dmul(wx, nx)), q[1] = dadd(q[1], dmul(wx, ny)), q[2] = dadd(q[2], dmul(wx, nz));
    q[3] = dadd(q[3], dmul(wy, ny)), q[4] = dadd(q[4], dmul(wy, nz)), q[5] = dadd(q[5], dmul(wz, nz));
    q[6] = dadd(q[6], dmul(wx, d)), q[7] = dadd(q[7], dmul(wy, d)), q[8] = dadd(q[8], dmul(wz, d));
    q[9] = dadd(q[9], dmul(dmul(w, d), d));
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = wave_sum_f64(q[k]);

  // ---- the cell's vertex: every lane holds the same sums, so the wave stays uniform; lane 0 writes
  const double count = (double)(ve - vb);
  double mean[3], x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) mean[k] = ddiv(sp[k], count), x[k] = mean[k];
  double M[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]}, U[9];
  jacobi3(M, U);
  const double lmax = fmax(M[0], fmax(M[4], M[8]));
  int kept = 0;
  if (lmax > 0.0) {
    const double floor_l = dmul(a.eig_eps, lmax);
    const double g0 = -dadd(q[6], dot3(q[0], q[1], q[2], mean[0], mean[1], mean[2]));
    const double g1 = -dadd(q[7], dot3(q[1], q[3], q[4], mean[0], mean[1], mean[2]));
    const double g2 = -dadd(q[8], dot3(q[2], q[4], q[5], mean[0], mean[1], mean[2]));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double lam = M[j * 4];
      if (!(lam > floor_l)) continue;
      const double t = ddiv(dot3(U[j], U[3 + j], U[6 + j], g0, g1, g2), lam);
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = dadd(x[k], dmul(U[3 * k + j], t));
      ++kept;
    }
  }
  const long long key = a.cell_keys[cell];
  const long long idx[3] = {key % a.grid.nx, (key / a.grid.nx) % a.grid.ny, key / ((long long)a.grid.nx * a.grid.ny)};
  const double org[3] = {a.grid.ox, a.grid.oy, a.grid.oz};
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = dadd(org[k], dmul((double)idx[k], a.grid.c));
    inside = inside && isfinite(x[k]) && x[k] >= dsub(lo, dmul(0.5, a.grid.c)) && x[k] <= dadd(lo, dmul(1.5, a.grid.c));
  }
  int status = kept;
  if (!inside) {
    status = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = mean[k];
  }
  const double ax = dot3(q[0], q[1], q[2], x[0], x[1], x[2]), ay = dot3(q[1], q[3], q[4], x[0], x[1], x[2]), az = dot3(q[2], q[4], q[5], x[0], x[1], x[2]);
  const double err = dadd(dadd(dot3(x[0], x[1], x[2], ax, ay, az), dmul(2.0, dot3(q[6], q[7], q[8], x[0], x[1], x[2]))), q[9]);
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.pos[3 * cell + k] = (float)x[k];
    a.col[3 * cell + k] = (float)ddiv(sc[k], count);
    a.means[3 * cell + k] = mean[k];
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) a.quadrics[10 * cell + k] = q[k];
  a.err[cell] = err;
  a.status[cell] = status;
}

}  // namespace

int launch_mesh_cell_keys(const MeshKeysArgs& a, hipStream_t st) {
  if (a.num_vertices == 0) return FP_OK;
  hipLaunchKernelGGL(mesh_cell_keys_kernel, dim3((unsigned)((a.num_vertices + MESH_THREADS - 1) / MESH_THREADS)), dim3(MESH_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("mesh_cell_keys");
  return FP_OK;
}

int launch_mesh_cluster(const MeshClusterArgs& a, hipStream_t st) {
  if (a.num_cells == 0) return FP_OK;
  hipLaunchKernelGGL(mesh_cluster_kernel, dim3((unsigned)((a.num_cells + MESH_WAVES - 1) / MESH_WAVES)), dim3(MESH_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("mesh_cluster");
  return FP_OK;
}
