"""numpy restatement of fp_pts_diameter and fp_directed_hausdorff (include/foundpose_amd.h, csrc/point_extremes.hip), written
from the contract, not from the kernels: brute force, the contract's operation order, np.fmin.reduce(..., initial=inf) for the nearest neighbour,
the root after the reduction.  numpy's elementwise fp64 +, -, * and sqrt are IEEE operations rounded one by one, so the device must agree with
this file bit for bit.  `evaluator(pts)` is the Hausdorff evaluation the host logic of foundpose_amd.models_info takes as a callable."""

import numpy as np


def place(tf12, pts):
    """[12] = R row-major | t, pts [M, 3] -> [M, 3]: ((r0 x + r1 y) + r2 z) + t per row."""
    R, t = np.asarray(tf12, np.float64)[:9].reshape(3, 3), np.asarray(tf12, np.float64)[9:]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)


def _sq(A, B):
    """[M, V]: (dx dx + dy dy) + dz dz with d = a - b, one contiguous plane per coordinate."""
    dx, dy, dz = (A[:, None, i] - B[None, :, i] for i in range(3))
    return (dx * dx + dy * dy) + dz * dz


def diameter(pts, chunk=256):
    """-> (d, (i, j)): the maximum of d2 over i < j starts at 0 with the pair (0, 0) and a candidate, taken in lexicographic order, replaces it
    only when strictly greater (a NaN never does); one root at the end."""
    pts = np.asarray(pts, np.float64)
    V = len(pts)
    best, pair = 0.0, (0, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, V, chunk):
            s = _sq(pts[c0:c0 + chunk], pts)
            rows = np.arange(c0, min(V, c0 + chunk))
            s[np.arange(V)[None, :] <= rows[:, None]] = -1.0     # i < j only
            s[np.isnan(s)] = -1.0
            m = s.max(axis=1)
            if m.max() > best:
                r = int(np.argmax(m))                              # the first row, and in it the first column, that attain it
                best, pair = float(m[r]), (int(rows[r]), int(np.argmax(s[r])))
        return float(np.sqrt(np.float64(best))), pair


def nn_sq(Q, P, chunk=512):
    """Per row of Q the smallest squared distance to a row of P: from +inf, a candidate wins only when strictly smaller, a NaN never."""
    out = np.empty(Q.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, Q.shape[0], chunk):
            out[c0:c0 + chunk] = np.fmin.reduce(_sq(Q[c0:c0 + chunk], P), axis=1, initial=np.inf)
    return out


def directed_hausdorff(pts, tf12, stride=1):
    """-> (h, v): sqrt(max_v min_u d2(T p_v, p_u)) over v = 0, stride, ... and the lowest v that attains the maximum."""
    pts = np.asarray(pts, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = nn_sq(place(tf12, pts[::stride]), pts)
        k = int(np.argmax(m))                                      # m holds no NaN; argmax is the first occurrence
        return float(np.sqrt(m[k])), k * stride


def batch_hausdorff(pts, tfs, stride=1):
    """fp_directed_hausdorff: tfs [K, 12] -> (h [K], arg [K])."""
    r = [directed_hausdorff(pts, tf, stride) for tf in np.asarray(tfs, np.float64).reshape(-1, 12)]
    return np.array([x[0] for x in r], np.float64), np.array([x[1] for x in r], np.int32)


# ---------------------------------------------------------------------------------------------------------- the test shapes
SHIFT = np.array([13.0, -7.0, 21.0])    # so that the centre is not the origin


def box_lattice(nx, ny, nz, spacing=8.0, extra=None):
    """The boundary points of an nx x ny x nz integer grid at `spacing` (plus the points of `extra`), shifted."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    edge = np.any((g == 0) | (g == np.array([nx, ny, nz]) - 1), axis=1)
    pts = g[edge].astype(np.float64) * spacing
    if extra is not None:
        pts = np.concatenate([pts, np.asarray(extra, np.float64).reshape(-1, 3)])
    return pts + SHIFT


def prism(n, radius=40.0, height=100.0, levels=5):
    """Rings of n vertices at `levels` heights and the two cap centres, shifted."""
    a = 2.0 * np.pi * np.arange(n) / n
    ring = [np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1) for z in np.linspace(0.0, height, levels)]
    return np.concatenate(ring + [np.array([[0.0, 0.0, 0.0], [0.0, 0.0, height]])]) + SHIFT


def write_ply(path, vertices, faces=()):
    """A BOP-style ascii PLY: `float` vertices (the loader keeps float32), triangles."""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(vertices))
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces))
        for v in vertices:
            f.write("%s %s %s\n" % tuple(repr(float(x)) for x in v))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(i) for i in t))


def evaluator(pts):
    """The callable of models_info's host logic: (transforms [K, 12], query_stride) -> h [K]."""
    pts = np.asarray(pts, np.float64)
    return lambda tfs, stride: batch_hausdorff(pts, tfs, stride)[0]
