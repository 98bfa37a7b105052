// Template renderer: a batched, deterministic triangle rasterizer for one vertex-coloured mesh seen by B cameras, and the
// SSAA downsample that ends the template chain of scripts/gen_templates.py (DESIGN.md section 8 holds the contract).
//
//   render_vertex_kernel   per (view, vertex): world_to_eye in fp64 (operation for operation like crop.hip's chain),
//                          window position, snap to 8 sub-pixel bits, eye-space normal; min-z reduction (near plane)
//   render_setup_kernel    per (view, triangle): winding normalised by the sign of the exact area, edge functions as
//                          int64 coefficients, top-left bits, pixel box; per-tile counts (integer atomics, order-free)
//   render_scan_kernel     one workgroup: exclusive scan of the counts into int64 list offsets, the list total and the
//                          decoded min z for the host's one check per batch
//   (setup, pass 1)        per (view, triangle): the triangle id into every tile list its box touches (slot order is
//                          arbitrary; the raster's total order makes the result independent of it)
//   render_raster_kernel   one 256-thread workgroup per (view, 32 x 32 tile), 4 pixels per thread; triangle records staged
//                          through LDS; nearest z (fp32), ties to the lower triangle id; then the winners are shaded and
//                          the per-view box of covered pixels is reduced (integer atomics).  <false>: vertex colours;
//                          <true>: a trilinear sample of the texture pyramid at the interpolated uv, analytic LOD
//   texture_*_kernel       the mip pyramid of a texture (packed RGBA8, integer box filter, one launch per level)
//   downsample_kernel      ssaa x ssaa blocks -> template pixels: colour block mean -> trunc(255 c), depth / mask top-left
//
// Coverage, depth, mask and triangle id are exact functions of the inputs (integer edge functions, individually rounded
// fp64 / fp32 operations, no contraction, no float atomics): tests/render_ref.py restates them in numpy bit for bit.
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

namespace {

constexpr int TILE = FP_RENDER_TILE;  // 32 x 32 pixels per raster workgroup
constexpr int CHUNK = 256;            // triangle records staged through LDS per step

FP_DEVICE float fm(float a, float b) { return __fmul_rn(a, b); }
FP_DEVICE float fa(float a, float b) { return __fadd_rn(a, b); }
FP_DEVICE float fsub(float a, float b) { return __fsub_rn(a, b); }
FP_DEVICE float fdv(float a, float b) { return __fdiv_rn(a, b); }
FP_DEVICE float fsq(float a) { return __fsqrt_rn(a); }
FP_DEVICE float fclamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
FP_DEVICE float fdot3(float a0, float a1, float a2, float b0, float b1, float b2) { return fa(fa(fm(a0, b0), fm(a1, b1)), fm(a2, b2)); }

struct VertRec {        // per (view, vertex)
  long long X, Y;       // window position x 256, rounded half to even
  double z;             // eye-space z, mm
  float n[3];           // eye-space normal (R^T n, fp32)
  float pad;
};
static_assert(sizeof(VertRec) == FP_RENDER_VERT_BYTES, "vertex record size");

struct TriRec {         // per (view, triangle); vertex k is opposite edge k
  long long A[3], B[3], C[3];  // E_k(X, Y) = A_k X + B_k Y + C_k (exact in int64: |coords| <= 2^29)
  double z[3];
  long long area;       // sum of the three edge functions, > 0 (0: dropped)
  int vid[3];           // mesh vertex ids after the winding swap
  int x0, y0, x1, y1;   // pixel box, clamped to the viewport (x0 > x1: empty)
  int tl;               // bit k: edge k is a top or left edge
  int tri;              // face index (the tie-break)
};
static_assert(sizeof(TriRec) == FP_RENDER_TRI_BYTES, "triangle record size");

FP_DEVICE unsigned long long order_key(double z) {  // monotonic map of doubles onto unsigned integers
  const unsigned long long b = (unsigned long long)__double_as_longlong(z);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
FP_DEVICE double order_key_inv(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__global__ __launch_bounds__(256) void render_vertex_kernel(RenderArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < (long long)a.batch * a.num_verts;
  unsigned long long key = ~0ull;
  if (live) {
    const int b = (int)(i / a.num_verts), v = (int)(i % a.num_verts);
    const double* c = a.cams + (size_t)b * 16;  // f[2] c[2] R[9] (row-major T_world_from_eye) t[3]
    const double* R = c + 4;
    // world_to_eye: (w - t) @ R
    const double dx = dadd((double)a.verts[3 * v + 0], -c[13]), dy = dadd((double)a.verts[3 * v + 1], -c[14]),
                 dz = dadd((double)a.verts[3 * v + 2], -c[15]);
    const double ex = dot3(dx, dy, dz, R[0], R[3], R[6]);
    const double ey = dot3(dx, dy, dz, R[1], R[4], R[7]);
    const double ez = dot3(dx, dy, dz, R[2], R[5], R[8]);
    // eye_to_window, then 8 sub-pixel bits
    const double u = dadd(dmul(ddiv(ex, ez), c[0]), c[2]), w = dadd(dmul(ddiv(ey, ez), c[1]), c[3]);
    const double us = dmul(u, 256.0), ws = dmul(w, 256.0);
    VertRec r;
    const bool ok = fabs(us) <= FP_RENDER_MAX_FIXED && fabs(ws) <= FP_RENDER_MAX_FIXED && ez == ez;
    r.X = ok ? __double2ll_rn(us) : 0;
    r.Y = ok ? __double2ll_rn(ws) : 0;
    r.z = ez;
    const float n0 = a.normals[3 * v + 0], n1 = a.normals[3 * v + 1], n2 = a.normals[3 * v + 2];
    r.n[0] = fdot3(n0, n1, n2, (float)R[0], (float)R[3], (float)R[6]);
    r.n[1] = fdot3(n0, n1, n2, (float)R[1], (float)R[4], (float)R[7]);
    r.n[2] = fdot3(n0, n1, n2, (float)R[2], (float)R[5], (float)R[8]);
    r.pad = 0.f;
    reinterpret_cast<VertRec*>(a.vert_ws)[i] = r;
    key = order_key(ez);
    if (!ok) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), 1ull);
  }
  for (int o = 32; o >= 1; o >>= 1) key = min(key, __shfl_xor(key, o));
  if ((threadIdx.x & 63) == 0 && key != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(a.status), key);
}

FP_DEVICE long long floor_div256(long long v) { return v >> 8; }  // arithmetic shift: floor

__global__ __launch_bounds__(256) void render_setup_kernel(RenderArgs a, int pass) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.batch * a.num_faces) return;
  const int b = (int)(i / a.num_faces), f = (int)(i % a.num_faces);
  TriRec* rec = reinterpret_cast<TriRec*>(a.tri_ws) + i;
  const int tiles_x = (a.width + TILE - 1) / TILE, tiles = tiles_x * ((a.height + TILE - 1) / TILE);
  int x0, y0, x1, y1;
  if (pass == 0) {
    int vid[3] = {a.faces[3 * f + 0], a.faces[3 * f + 1], a.faces[3 * f + 2]};
    TriRec r;
    r.tri = f;
    r.x0 = r.y0 = 0;
    r.x1 = r.y1 = -1;
    r.area = 0;
    const VertRec* vw = reinterpret_cast<const VertRec*>(a.vert_ws) + (size_t)b * a.num_verts;
    long long X[3], Y[3];
    double z[3];
    for (int k = 0; k < 3; ++k) {
      if (vid[k] < 0 || vid[k] >= a.num_verts) {  // the loader checks ids; a bad one is reported, never read
        atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), 2ull);
        *rec = r;
        return;
      }
      const VertRec& v = vw[vid[k]];
      X[k] = v.X, Y[k] = v.Y, z[k] = v.z;
    }
    long long area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (area < 0) {  // no culling: normalise the winding
      long long t = X[1]; X[1] = X[2]; X[2] = t;
      t = Y[1]; Y[1] = Y[2]; Y[2] = t;
      const double tz = z[1]; z[1] = z[2]; z[2] = tz;
      const int tv = vid[1]; vid[1] = vid[2]; vid[2] = tv;
      area = -area;
    }
    r.tl = 0;
    for (int k = 0; k < 3; ++k) {
      const int ia = (k + 1) % 3, ib = (k + 2) % 3;  // edge k runs from vertex k+1 to vertex k+2
      const long long ddx = X[ib] - X[ia], ddy = Y[ib] - Y[ia];
      r.A[k] = -ddy;
      r.B[k] = ddx;
      r.C[k] = ddy * X[ia] - ddx * Y[ia];
      r.z[k] = z[k];
      r.vid[k] = vid[k];
      if (ddy < 0 || (ddy == 0 && ddx > 0)) r.tl |= 1 << k;
    }
    r.area = area;
    if (area > 0) {
      const long long mnx = min(X[0], min(X[1], X[2])), mxx = max(X[0], max(X[1], X[2]));
      const long long mny = min(Y[0], min(Y[1], Y[2])), mxy = max(Y[0], max(Y[1], Y[2]));
      // pixel x is sampled at 256 x + 128: the first centre >= min, the last <= max
      const long long px0 = -floor_div256(128 - mnx), px1 = floor_div256(mxx - 128);
      const long long py0 = -floor_div256(128 - mny), py1 = floor_div256(mxy - 128);
      r.x0 = (int)max(px0, 0ll), r.x1 = (int)min(px1, (long long)a.width - 1);
      r.y0 = (int)max(py0, 0ll), r.y1 = (int)min(py1, (long long)a.height - 1);
      if (r.x0 > r.x1 || r.y0 > r.y1) r.x0 = r.y0 = 0, r.x1 = r.y1 = -1;
    }
    *rec = r;
    x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1;
  } else {
    x0 = rec->x0, y0 = rec->y0, x1 = rec->x1, y1 = rec->y1;
  }
  if (x0 > x1) return;
  int* counts = a.tile_counts + (size_t)b * tiles;
  const long long* off = a.tile_offsets + (size_t)b * tiles;
  for (int ty = y0 / TILE; ty <= y1 / TILE; ++ty)
    for (int tx = x0 / TILE; tx <= x1 / TILE; ++tx) {
      const int t = ty * tiles_x + tx;
      if (pass == 0) {
        atomicAdd(counts + t, 1);
      } else {
        const int slot = atomicSub(counts + t, 1) - 1;  // counts run back down to 0
        a.lists[off[t] + slot] = f;
      }
    }
}

// one workgroup of 1024 threads: exclusive int64 scan of n counts (each thread owns a contiguous run)
__global__ __launch_bounds__(1024) void render_scan_kernel(RenderArgs a, long long n) {
  __shared__ long long part[1024];
  const long long per = (n + 1023) / 1024, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
  long long s = 0;
  for (long long i = lo; i < hi; ++i) s += a.tile_counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    const long long v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  long long run = part[threadIdx.x] - s;
  for (long long i = lo; i < hi; ++i) {
    a.tile_offsets[i] = run;
    run += a.tile_counts[i];
  }
  if (threadIdx.x == 1023) {
    a.tile_offsets[n] = part[1023];
    a.status[2] = part[1023];
    a.status[3] = __double_as_longlong(order_key_inv((unsigned long long)a.status[0]));
  }
}

__global__ __launch_bounds__(256) void render_init_kernel(RenderArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    a.status[0] = -1;  // min-z key: all ones
    a.status[1] = a.status[2] = a.status[3] = 0;
  }
  if (i < a.batch && a.boxes) {
    a.boxes[4 * i + 0] = a.boxes[4 * i + 1] = INT_MAX;
    a.boxes[4 * i + 2] = a.boxes[4 * i + 3] = INT_MIN;
  }
}

// Lighting of one covered pixel ("unpinned"): pyrender's metallic-roughness shader with the
// reference's spot light at the camera and its ambient term, evaluated in eye space (metres).
// metallic / alpha (= roughness^2): the material; the vertex-coloured path passes the constants 0.2 / 0.64.
FP_DEVICE float shade_channel(float base, float nl, float nv, float nh, float vh, float radiance, float F90, float kMetallic,
                              float kAlpha) {
  constexpr float kPi = 3.14159265358979f, kF0 = 0.04f;
  const float diffuse_color = fm(fm(base, fsub(1.f, kF0)), fsub(1.f, kMetallic));
  const float spec_color = fa(fm(kF0, fsub(1.f, kMetallic)), fm(base, kMetallic));
  const float one_vh = fclamp(fsub(1.f, vh), 0.f, 1.f);
  const float p5 = fm(fm(fm(fm(one_vh, one_vh), one_vh), one_vh), one_vh);
  const float F = fa(spec_color, fm(fsub(F90, spec_color), p5));
  const float a2 = fm(kAlpha, kAlpha);
  const float gl = fdv(fm(2.f, nl), fa(nl, fsq(fa(a2, fm(fsub(1.f, a2), fm(nl, nl))))));
  const float gv = fdv(fm(2.f, nv), fa(nv, fsq(fa(a2, fm(fsub(1.f, a2), fm(nv, nv))))));
  const float G = fm(gl, gv);
  const float fd = fa(fm(fsub(fm(nh, a2), nh), nh), 1.f);
  const float D = fdv(a2, fm(fm(kPi, fd), fd));
  const float diff = fm(fsub(1.f, F), fdv(diffuse_color, kPi));
  const float spec = fdv(fm(fm(F, G), D), fm(fm(4.f, nl), nv));
  const float c = fa(fm(fm(nl, radiance), fa(diff, spec)), fm(0.02f, base));
  return fclamp(c, 0.f, 1.f);
}

// GL REPEAT on an integer texel index, then a clamp: the result is inside [0, n) for every int i
FP_DEVICE int wrap_index(int i, int n) { return min(max(((i % n) + n) % n, 0), n - 1); }

// GL LINEAR on level l: s = u w - 1/2, t = (1 - v) h - 1/2 (row 0 of the image is v = 1), texels k / 255, fixed blend order
FP_DEVICE void sample_bilinear(const TexArgs& t, int l, float u, float v, float out[3]) {
  const int w = t.w[l], h = t.h[l];
  const float s = fsub(fm(u, (float)w), 0.5f), r = fsub(fm(fsub(1.f, v), (float)h), 0.5f);
  const float fs = floorf(s), fr = floorf(r);
  const float al = fsub(s, fs), be = fsub(r, fr);
  const int i0 = (int)fclamp(fs, -1073741824.f, 1073741824.f), j0 = (int)fclamp(fr, -1073741824.f, 1073741824.f);
  const int x0 = wrap_index(i0, w), x1 = wrap_index(i0 + 1, w), y0 = wrap_index(j0, h), y1 = wrap_index(j0 + 1, h);
  const unsigned* lv = t.texels + t.off[l];
  const unsigned p00 = lv[y0 * w + x0], p10 = lv[y0 * w + x1], p01 = lv[y1 * w + x0], p11 = lv[y1 * w + x1];
  const float a1 = fsub(1.f, al), b1 = fsub(1.f, be);
  for (int ch = 0; ch < 3; ++ch) {
    const int sh = 8 * ch;
    const float t00 = fdv((float)((p00 >> sh) & 255u), 255.f), t10 = fdv((float)((p10 >> sh) & 255u), 255.f);
    const float t01 = fdv((float)((p01 >> sh) & 255u), 255.f), t11 = fdv((float)((p11 >> sh) & 255u), 255.f);
    out[ch] = fa(fm(b1, fa(fm(a1, t00), fm(al, t10))), fm(be, fa(fm(a1, t01), fm(al, t11))));
  }
}

// Base colour of a textured winner: uv at the pixel centre (w_k as the colour path), its screen derivatives from the
// analytic d q_k / dx = ((256 A_k) / area) / z_k (fp64), GL's isotropic LOD, LINEAR / LINEAR_MIPMAP_LINEAR, sRGB decode,
// base factor.
FP_DEVICE void textured_base(const TexArgs& t, const TriRec& r, const double q[3], float w0, float w1, float w2, float base[3]) {
  const float2 t0 = reinterpret_cast<const float2*>(t.uv)[r.vid[0]], t1 = reinterpret_cast<const float2*>(t.uv)[r.vid[1]],
               t2 = reinterpret_cast<const float2*>(t.uv)[r.vid[2]];
  const float u = fa(fa(fm(w0, t0.x), fm(w1, t1.x)), fm(w2, t2.x)), v = fa(fa(fm(w0, t0.y), fm(w1, t1.y)), fm(w2, t2.y));
  const double ar = (double)r.area;
  double qx[3], qy[3];
  for (int e = 0; e < 3; ++e) {
    qx[e] = ddiv(ddiv(dmul(256.0, (double)r.A[e]), ar), r.z[e]);
    qy[e] = ddiv(ddiv(dmul(256.0, (double)r.B[e]), ar), r.z[e]);
  }
  const double D = dadd(dadd(q[0], q[1]), q[2]), Dx = dadd(dadd(qx[0], qx[1]), qx[2]), Dy = dadd(dadd(qy[0], qy[1]), qy[2]);
  const double u0 = t0.x, u1 = t1.x, u2 = t2.x, v0 = t0.y, v1 = t1.y, v2 = t2.y, ud = u, vd = v;
  const double ux = ddiv(dadd(dot3(qx[0], qx[1], qx[2], u0, u1, u2), -dmul(ud, Dx)), D);
  const double vx = ddiv(dadd(dot3(qx[0], qx[1], qx[2], v0, v1, v2), -dmul(vd, Dx)), D);
  const double uy = ddiv(dadd(dot3(qy[0], qy[1], qy[2], u0, u1, u2), -dmul(ud, Dy)), D);
  const double vy = ddiv(dadd(dot3(qy[0], qy[1], qy[2], v0, v1, v2), -dmul(vd, Dy)), D);
  const double W = t.w[0], H = t.h[0];
  const double ax = dmul(ux, W), bx = dmul(vx, H), ay = dmul(uy, W), by = dmul(vy, H);
  const double rho2 = fmax(dadd(dmul(ax, ax), dmul(bx, bx)), dadd(dmul(ay, ay), dmul(by, by)));
  const float lod = fm(0.5f, log2f((float)rho2));
  const int q_top = t.levels - 1;
  float c[3];
  if (!(lod > 0.f)) {  // magnification (and a degenerate uv map): LINEAR on level 0
    sample_bilinear(t, 0, u, v, c);
  } else {
    const bool top = lod >= (float)q_top;
    const float fl = floorf(lod);
    const int d1 = top ? q_top : (int)fl;
    const float f = top ? 0.f : fsub(lod, fl);
    sample_bilinear(t, d1, u, v, c);
    if (d1 < q_top) {  // d2 = d1 + 1; at the top level d2 = d1 and f = 0: the blend is c exactly
      float c2[3];
      sample_bilinear(t, d1 + 1, u, v, c2);
      const float f1 = fsub(1.f, f);
      for (int ch = 0; ch < 3; ++ch) c[ch] = fa(fm(f1, c[ch]), fm(f, c2[ch]));
    }
  }
  for (int ch = 0; ch < 3; ++ch) {
    float x = c[ch];
    if (t.srgb) x = x <= 0.04045f ? fdv(x, 12.92f) : powf(fdv(fa(x, 0.055f), 1.055f), 2.4f);
    base[ch] = fm(t.factor[ch], x);
  }
}

template <bool kTextured>
__global__ __launch_bounds__(256) void render_raster_kernel(RenderArgs a, TexArgs tex) {
  __shared__ TriRec lds[CHUNK];
  const int tiles_x = (a.width + TILE - 1) / TILE, tiles = tiles_x * ((a.height + TILE - 1) / TILE);
  const int tile = blockIdx.x, b = blockIdx.y;
  const int px = (tile % tiles_x) * TILE + (threadIdx.x & 31), py0 = (tile / tiles_x) * TILE + (threadIdx.x >> 5);
  const long long start = a.tile_offsets[(size_t)b * tiles + tile], end = a.tile_offsets[(size_t)b * tiles + tile + 1];
  const TriRec* recs = reinterpret_cast<const TriRec*>(a.tri_ws) + (size_t)b * a.num_faces;
  float best_z[4];
  int best_t[4];
  for (int k = 0; k < 4; ++k) best_z[k] = INFINITY, best_t[k] = -1;
  const long long PX = (long long)px * 256 + 128;
  for (long long base = start; base < end; base += CHUNK) {
    const int n = (int)min((long long)CHUNK, end - base);
    __syncthreads();
    if ((int)threadIdx.x < n) lds[threadIdx.x] = recs[a.lists[base + threadIdx.x]];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const TriRec& r = lds[j];
      if (px < r.x0 || px > r.x1) continue;
      for (int k = 0; k < 4; ++k) {
        const int py = py0 + 8 * k;
        if (py < r.y0 || py > r.y1) continue;
        const long long PY = (long long)py * 256 + 128;
        long long E[3];
        bool in = true;
        for (int e = 0; e < 3; ++e) {
          E[e] = r.A[e] * PX + r.B[e] * PY + r.C[e];
          in = in && (E[e] > 0 || (E[e] == 0 && ((r.tl >> e) & 1)));
        }
        if (!in) continue;
        const double ar = (double)r.area;
        const double q0 = ddiv(ddiv((double)E[0], ar), r.z[0]), q1 = ddiv(ddiv((double)E[1], ar), r.z[1]),
                     q2 = ddiv(ddiv((double)E[2], ar), r.z[2]);
        const float z = (float)ddiv(1.0, dadd(dadd(q0, q1), q2));
        if (z < best_z[k] || (z == best_z[k] && r.tri < best_t[k])) best_z[k] = z, best_t[k] = r.tri;
      }
    }
  }
  // shading of the winners, outputs, box of the covered pixels
  int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
  const double* cam = a.cams + (size_t)b * 16;
  const float fx = (float)cam[0], fy = (float)cam[1], cx = (float)cam[2], cy = (float)cam[3];
  // spot cone: pyrender's smoothstep-free falloff, scale = 1 / (cos(inner) - cos(outer)), offset = -cos(outer) scale
  constexpr float kCosInner = 0.98078528040323f /* cos(pi/16) */, kCosOuter = 0.86602540378444f /* cos(pi/6) */;
  const float spot_scale = fdv(1.f, fsub(kCosInner, kCosOuter)), spot_offset = fm(-kCosOuter, spot_scale);
  const VertRec* vw = reinterpret_cast<const VertRec*>(a.vert_ws) + (size_t)b * a.num_verts;
  for (int k = 0; k < 4; ++k) {
    const int py = py0 + 8 * k;
    if (px >= a.width || py >= a.height) continue;
    const size_t pix = ((size_t)b * a.height + py) * a.width + px;
    float rgb[3] = {0.f, 0.f, 0.f};
    const int t = best_t[k];
    if (t >= 0) {
      const TriRec& r = recs[t];
      const long long PY = (long long)py * 256 + 128;
      const double ar = (double)r.area;
      double q[3];
      for (int e = 0; e < 3; ++e) q[e] = ddiv(ddiv((double)(r.A[e] * PX + r.B[e] * PY + r.C[e]), ar), r.z[e]);
      const double zz = ddiv(1.0, dadd(dadd(q[0], q[1]), q[2]));
      const float w0 = (float)dmul(q[0], zz), w1 = (float)dmul(q[1], zz), w2 = (float)dmul(q[2], zz);  // perspective-correct
      const float* c0 = a.colors + 3 * r.vid[0];
      const float* c1 = a.colors + 3 * r.vid[1];
      const float* c2 = a.colors + 3 * r.vid[2];
      const VertRec &v0 = vw[r.vid[0]], &v1 = vw[r.vid[1]], &v2 = vw[r.vid[2]];
      float n[3];
      for (int ch = 0; ch < 3; ++ch) n[ch] = fa(fa(fm(w0, v0.n[ch]), fm(w1, v1.n[ch])), fm(w2, v2.n[ch]));
      const float nn = fsq(fdot3(n[0], n[1], n[2], n[0], n[1], n[2]));
      for (int ch = 0; ch < 3; ++ch) n[ch] = nn > 0.f ? fdv(n[ch], nn) : 0.f;
      // surface point in eye space, metres; the light and the eye sit at the origin
      const float zm = fm(best_z[k], 0.001f);
      const float pxe = fm(fdv(fsub(fa((float)px, 0.5f), cx), fx), zm), pye = fm(fdv(fsub(fa((float)py, 0.5f), cy), fy), zm);
      const float d2 = fdot3(pxe, pye, zm, pxe, pye, zm), dl = fsq(d2);
      const float l0 = fdv(-pxe, dl), l1 = fdv(-pye, dl), l2 = fdv(-zm, dl);  // to the light = to the eye
      const float h0 = fa(l0, l0), h1 = fa(l1, l1), h2 = fa(l2, l2), hn = fsq(fdot3(h0, h1, h2, h0, h1, h2));
      const float nl = fclamp(fdot3(n[0], n[1], n[2], l0, l1, l2), 0.001f, 1.f);
      const float nv = fclamp(fabsf(fdot3(n[0], n[1], n[2], l0, l1, l2)), 0.001f, 1.f);
      const float nh = fclamp(fdv(fdot3(n[0], n[1], n[2], h0, h1, h2), hn), 0.f, 1.f);
      const float vh = fclamp(fdv(fdot3(l0, l1, l2, h0, h1, h2), hn), 0.f, 1.f);
      const float cd = fdv(zm, dl);  // cos of the angle to the spot axis (+z)
      float sa = fclamp(fa(fm(cd, spot_scale), spot_offset), 0.f, 1.f);
      sa = fm(sa, sa);
      const float radiance = fdv(fm(2.4f, sa), d2);
      float base[3], metallic, alpha;
      if constexpr (kTextured) {
        textured_base(tex, r, q, w0, w1, w2, base);
        metallic = tex.metallic, alpha = fm(tex.roughness, tex.roughness);
      } else {
        for (int ch = 0; ch < 3; ++ch) base[ch] = fa(fa(fm(w0, c0[ch]), fm(w1, c1[ch])), fm(w2, c2[ch]));
        metallic = 0.2f, alpha = 0.64f;  // roughness 0.8 squared
      }
      // reflectance at 90 degrees from the largest specular colour component (the metallic mix of 0.04 and the base)
      float refl = 0.f;
      for (int ch = 0; ch < 3; ++ch) refl = fmaxf(refl, fa(fm(0.04f, fsub(1.f, metallic)), fm(base[ch], metallic)));
      const float F90 = fclamp(fm(refl, 25.f), 0.f, 1.f);
      for (int ch = 0; ch < 3; ++ch) {
        const float c = shade_channel(base[ch], nl, nv, nh, vh, radiance, F90, metallic, alpha);
        rgb[ch] = fdv((float)__float2int_rn(fm(c, 255.f)), 255.f);  // unorm8 framebuffer, then / 255
      }
      bx0 = min(bx0, px), bx1 = max(bx1, px), by0 = min(by0, py), by1 = max(by1, py);
    }
    a.depth[pix] = t >= 0 ? best_z[k] : 0.f;
    a.mask[pix] = t >= 0 ? 255 : 0;
    if (a.tri_id) a.tri_id[pix] = t;
    if (a.color)
      for (int ch = 0; ch < 3; ++ch) a.color[pix * 3 + ch] = rgb[ch];
  }
  if (a.boxes) {
    for (int o = 32; o >= 1; o >>= 1) {
      bx0 = min(bx0, __shfl_xor(bx0, o)), by0 = min(by0, __shfl_xor(by0, o));
      bx1 = max(bx1, __shfl_xor(bx1, o)), by1 = max(by1, __shfl_xor(by1, o));
    }
    if ((threadIdx.x & 63) == 0 && bx0 != INT_MAX) {
      atomicMin(a.boxes + 4 * b + 0, bx0), atomicMin(a.boxes + 4 * b + 1, by0);
      atomicMax(a.boxes + 4 * b + 2, bx1), atomicMax(a.boxes + 4 * b + 3, by1);
    }
  }
}

// level 0 of a pyramid: RGB bytes -> packed RGBA8, A = 255
__global__ __launch_bounds__(256) void texture_pack_kernel(const unsigned char* rgb, int n, unsigned* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (unsigned)rgb[3 * i] | ((unsigned)rgb[3 * i + 1] << 8) | ((unsigned)rgb[3 * i + 2] << 16) | 0xff000000u;
}

// level l + 1 from level l: the rounded mean of a 2 x 2 block, indices clamped to the source (integer, exact)
__global__ __launch_bounds__(256) void texture_reduce_kernel(const unsigned* src, int sw, int sh, unsigned* dst, int dw, int dh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= dw * dh) return;
  const int x = i % dw, y = i / dw;
  const int xa = min(2 * x, sw - 1), xb = min(2 * x + 1, sw - 1), ya = min(2 * y, sh - 1), yb = min(2 * y + 1, sh - 1);
  const unsigned p[4] = {src[ya * sw + xa], src[ya * sw + xb], src[yb * sw + xa], src[yb * sw + xb]};
  unsigned out = 0xff000000u;
  for (int ch = 0; ch < 3; ++ch) {
    const int sh8 = 8 * ch;
    const unsigned s = ((p[0] >> sh8) & 255u) + ((p[1] >> sh8) & 255u) + ((p[2] >> sh8) & 255u) + ((p[3] >> sh8) & 255u);
    out |= ((s + 2u) >> 2) << sh8;
  }
  dst[i] = out;
}

__global__ __launch_bounds__(256) void box_init_kernel(int* boxes, int batch) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < batch) boxes[4 * i + 0] = boxes[4 * i + 1] = INT_MAX, boxes[4 * i + 2] = boxes[4 * i + 3] = INT_MIN;
}

// cv2.resize by an integer factor f: INTER_AREA = the f x f block mean (summed along each row, the row sums in order,
// times 1/f^2), INTER_NEAREST = the block's top-left sample; then the reference's output casts.
__global__ __launch_bounds__(256) void downsample_kernel(DownsampleArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  const bool live = x < a.out_w && y < a.out_h;
  bool covered = false;
  if (live) {
    const int f = a.factor, sw = a.out_w * f, sh = a.out_h * f;
    const size_t plane = (size_t)sh * sw, opix = ((size_t)b * a.out_h + y) * a.out_w + x;
    const float inv = fdv(1.f, (float)(f * f));
    for (int ch = 0; ch < 3; ++ch) {
      const float* src = a.color + ((size_t)b * 3 + ch) * plane + (size_t)(y * f) * sw + x * f;
      float s = 0.f;
      for (int r = 0; r < f; ++r) {
        float row = src[(size_t)r * sw];
        for (int c = 1; c < f; ++c) row = fa(row, src[(size_t)r * sw + c]);
        s = r == 0 ? row : fa(s, row);
      }
      a.rgb[((size_t)b * 3 + ch) * a.out_h * a.out_w + (size_t)y * a.out_w + x] = (unsigned char)(int)fm(255.f, fm(s, inv));  // trunc
    }
    const size_t spix = (size_t)b * plane + (size_t)(y * f) * sw + x * f;
    const float d = rintf(a.depth[spix]);  // np.round: half to even
    a.depth_u16[opix] = (unsigned short)(d <= 0.f ? 0 : (d >= 65535.f ? 65535 : (int)d));
    const unsigned char m = a.mask[spix];
    a.mask_out[opix] = m;
    covered = m != 0;
  }
  if (a.boxes) {
    int bx0 = covered ? x : INT_MAX, by0 = covered ? y : INT_MAX, bx1 = covered ? x : INT_MIN, by1 = covered ? y : INT_MIN;
    for (int o = 32; o >= 1; o >>= 1) {
      bx0 = min(bx0, __shfl_xor(bx0, o)), by0 = min(by0, __shfl_xor(by0, o));
      bx1 = max(bx1, __shfl_xor(bx1, o)), by1 = max(by1, __shfl_xor(by1, o));
    }
    if ((threadIdx.x & 63) == 0 && bx0 != INT_MAX) {
      atomicMin(a.boxes + 4 * b + 0, bx0), atomicMin(a.boxes + 4 * b + 1, by0);
      atomicMax(a.boxes + 4 * b + 2, bx1), atomicMax(a.boxes + 4 * b + 3, by1);
    }
  }
}

}  // namespace

int launch_render_setup(const RenderArgs& a, hipStream_t st) {
  const int tiles = cdiv(a.width, TILE) * cdiv(a.height, TILE);
  const long long nv = (long long)a.batch * a.num_verts, nf = (long long)a.batch * a.num_faces;
  if (hipMemsetAsync(a.tile_counts, 0, sizeof(int) * (size_t)a.batch * tiles, st) != hipSuccess) {
    fp_set_error("render_setup: hipMemsetAsync failed");
    return FP_ERR_HIP;
  }
  hipLaunchKernelGGL(render_init_kernel, dim3(cdiv(a.batch, 256)), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("render_init");
  hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("render_vertex");
  hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, a, 0);
  FP_CHECK_LAUNCH("render_setup");
  hipLaunchKernelGGL(render_scan_kernel, dim3(1), dim3(1024), 0, st, a, (long long)a.batch * tiles);
  FP_CHECK_LAUNCH("render_scan");
  return FP_OK;
}

int launch_render_raster(const RenderArgs& a, hipStream_t st) {
  const int tiles = cdiv(a.width, TILE) * cdiv(a.height, TILE);
  const long long nf = (long long)a.batch * a.num_faces;
  hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, a, 1);
  FP_CHECK_LAUNCH("render_scatter");
  TexArgs none{};
  hipLaunchKernelGGL(render_raster_kernel<false>, dim3(tiles, a.batch), dim3(256), 0, st, a, none);
  FP_CHECK_LAUNCH("render_raster");
  return FP_OK;
}

int launch_render_raster_textured(const RenderArgs& a, const TexArgs& t, hipStream_t st) {
  const int tiles = cdiv(a.width, TILE) * cdiv(a.height, TILE);
  const long long nf = (long long)a.batch * a.num_faces;
  hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, a, 1);
  FP_CHECK_LAUNCH("render_scatter");
  hipLaunchKernelGGL(render_raster_kernel<true>, dim3(tiles, a.batch), dim3(256), 0, st, a, t);
  FP_CHECK_LAUNCH("render_raster_textured");
  return FP_OK;
}

int launch_texture_mips(const unsigned char* rgb, const TexArgs& t, unsigned* pyramid, hipStream_t st) {
  hipLaunchKernelGGL(texture_pack_kernel, dim3(cdiv(t.w[0] * t.h[0], 256)), dim3(256), 0, st, rgb, t.w[0] * t.h[0], pyramid);
  FP_CHECK_LAUNCH("texture_pack");
  for (int l = 1; l < t.levels; ++l) {
    hipLaunchKernelGGL(texture_reduce_kernel, dim3(cdiv(t.w[l] * t.h[l], 256)), dim3(256), 0, st, pyramid + t.off[l - 1],
                       t.w[l - 1], t.h[l - 1], pyramid + t.off[l], t.w[l], t.h[l]);
    FP_CHECK_LAUNCH("texture_reduce");
  }
  return FP_OK;
}

int launch_template_downsample(const DownsampleArgs& a, hipStream_t st) {
  if (a.boxes) {
    hipLaunchKernelGGL(box_init_kernel, dim3(cdiv(a.batch, 256)), dim3(256), 0, st, a.boxes, a.batch);
    FP_CHECK_LAUNCH("box_init");
  }
  hipLaunchKernelGGL(downsample_kernel, dim3(cdiv(a.out_w, 64), cdiv(a.out_h, 4), a.batch), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("template_downsample");
  return FP_OK;
}
