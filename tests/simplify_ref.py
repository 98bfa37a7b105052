"""Numpy fp64 restatement of mesh simplification by quadric vertex clustering (foundpose_amd/simplify.py, csrc/simplify.hip; DESIGN.md
section 32): the grid and the cell keys, the tables between the two kernels, the ordered sums (lane partition and xor butterfly), the
cyclic Jacobi, the solve, the box test, the face rules and the bisection on the cell size.  Every fp64 operation stands alone, in the
kernel's order; numpy never contracts two ufuncs into an FMA, and the per-cell part runs on Python floats (IEEE doubles).

The fixtures of tests/test_simplify_cpu.py and tests/test_gpu_simplify.py are built here as well."""
import math
from typing import Any, Dict, Optional, Tuple

import numpy as np

MAX_DIM = 1 << 20
EIG_EPS = 1e-3
JACOBI_SWEEPS = 30
BISECTION_ROUNDS = 32


# ------------------------------------------------------------------------------------------------------------------ grid and keys
def grid_for(vertices: np.ndarray, c: float) -> Optional[Tuple[np.ndarray, Tuple[int, int, int]]]:
    """(origin fp64 [3], (nx, ny, nz)) of the grid of cell size c anchored on the mesh, or None when a dimension exceeds 2^20."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    c = float(c)
    o = v.min(0) - c / 2
    g = (v.max(0) - o) / c
    if not np.all(np.isfinite(g)) or np.any(g >= MAX_DIM):
        return None
    return o, tuple(int(math.floor(x)) + 1 for x in g)


def cell_keys(vertices: np.ndarray, origin: np.ndarray, c: float, dims) -> np.ndarray:
    v = np.asarray(vertices, np.float32).astype(np.float64)
    idx = []
    for a in range(3):
        g = (v[:, a] - origin[a]) / float(c)
        i = np.where(g >= 0, np.where(g >= dims[a], dims[a] - 1, np.floor(np.where(np.isfinite(g), g, 0.0))), 0.0)
        idx.append(i.astype(np.int64))
    return (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]


def grid_coordinates(vertices: np.ndarray, origin: np.ndarray, c: float) -> np.ndarray:
    """g of every vertex and axis, for the fixture condition that none is close to an integer."""
    return (np.asarray(vertices, np.float32).astype(np.float64) - origin[None]) / float(c)


def tables(keys: np.ndarray, faces: np.ndarray) -> Dict[str, np.ndarray]:
    cells, rank = np.unique(keys, return_inverse=True)
    rank = rank.reshape(-1).astype(np.int64)

    def grouped(r):
        begin = np.zeros(len(cells) + 1, np.int64)
        begin[1:] = np.cumsum(np.bincount(r, minlength=len(cells)))
        return np.argsort(r, kind="stable").astype(np.int64), begin
    vert_order, vert_begin = grouped(rank)
    corner_order, corner_begin = grouped(rank[np.asarray(faces, np.int64).reshape(-1)])
    return {"cells": cells.astype(np.int64), "rank": rank, "vert_order": vert_order, "vert_begin": vert_begin, "corner_order": corner_order,
            "corner_begin": corner_begin}


# ------------------------------------------------------------------------------------------------------------------ the ordered sums
def lane_sums(records: np.ndarray, begin: np.ndarray) -> np.ndarray:
    """records fp64 [R, K] in record order, begin [C + 1] -> [C, K]: lane l starts from 0.0 and adds records begin + l, begin + l + 64,
    ... in ascending order; then the xor butterfly at distances 32 .. 1.  (A lane past the end adds +0.0, which changes no bit: a sum
    that started from +0.0 is never -0.0.)"""
    num_cells, k = len(begin) - 1, records.shape[1]
    acc = np.zeros((num_cells, 64, k))
    if len(records) == 0 or num_cells == 0:
        return acc[:, 0]
    lane = np.arange(64)
    rounds = int((np.diff(begin).max() + 63) // 64)
    for t in range(rounds):
        idx = begin[:-1, None] + t * 64 + lane[None]
        valid = idx < begin[1:, None]
        acc = acc + np.where(valid[..., None], records[np.minimum(idx, len(records) - 1)], 0.0)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def face_quadrics(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """fp64 [F, 10]: the ten terms a corner of each face adds (zeros where L is not > 0: nothing is added)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w_ = p1 - p0, p2 - p0
    mx = u[:, 1] * w_[:, 2] - u[:, 2] * w_[:, 1]
    my = u[:, 2] * w_[:, 0] - u[:, 0] * w_[:, 2]
    mz = u[:, 0] * w_[:, 1] - u[:, 1] * w_[:, 0]
    L = np.sqrt((mx * mx + my * my) + mz * mz)
    ok = L > 0
    Ls = np.where(ok, L, 1.0)
    nx, ny, nz = mx / Ls, my / Ls, mz / Ls
    w = 0.5 * Ls
    d = -_dot3(nx, ny, nz, p0[:, 0], p0[:, 1], p0[:, 2])
    wx, wy, wz = w * nx, w * ny, w * nz
    q = np.stack([wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, wx * d, wy * d, wz * d, (w * d) * d], 1)
    return np.where(ok[:, None], q, 0.0)


# ------------------------------------------------------------------------------------------------------------------ Jacobi and the solve
def jacobi3(M):
    """Cyclic Jacobi on the symmetric 3 x 3 M (a list of 9 floats, changed in place) -> V (9 floats): the diagonal of M holds the
    eigenvalues, column j of V the vector of eigenvalue j.  The kernel's operations in the kernel's order."""
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(JACOBI_SWEEPS):
        off = all_ = 0.0
        for i in range(9):
            sq = M[i] * M[i]
            all_ = all_ + sq
            if i % 4 != 0:
                off = off + sq
        if not off > 1e-30 * all_:
            break
        for p, r in ((0, 1), (0, 2), (1, 2)):
            apr = M[p * 3 + r]
            if apr == 0.0:
                continue
            theta = (M[r * 3 + r] - M[p * 3 + p]) / (2.0 * apr)
            tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(tt * tt + 1.0)
            s = tt * c
            for k in range(3):
                mkp, mkr = M[k * 3 + p], M[k * 3 + r]
                M[k * 3 + p] = c * mkp - s * mkr
                M[k * 3 + r] = s * mkp + c * mkr
            for k in range(3):
                mpk, mrk = M[p * 3 + k], M[r * 3 + k]
                M[p * 3 + k] = c * mpk - s * mrk
                M[r * 3 + k] = s * mpk + c * mrk
            for k in range(3):
                vkp, vkr = V[k * 3 + p], V[k * 3 + r]
                V[k * 3 + p] = c * vkp - s * vkr
                V[k * 3 + r] = s * vkp + c * vkr
    return V


def cluster(vertices: np.ndarray, colors: np.ndarray, faces: np.ndarray, tb: Dict[str, np.ndarray], origin: np.ndarray, c: float, dims,
            eig_eps: float = EIG_EPS) -> Dict[str, Any]:
    """fp_mesh_cluster.  Besides the kernel's outputs: x64 (the fp64 position before the store), ratios [C, 3] (l_j / lmax, NaN where
    lmax is not > 0) and margin [C] (the solved x's smallest distance to a bound of the box test over c, negative when outside; NaN
    without a solve) for the fixture conditions."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    col = np.asarray(colors, np.float32).astype(np.float64)
    c = float(c)
    num_cells = len(tb["cells"])
    vsum = lane_sums(np.concatenate([v, col], 1)[tb["vert_order"]], tb["vert_begin"])
    fq = face_quadrics(vertices, faces)
    qsum = lane_sums(fq[tb["corner_order"] // 3], tb["corner_begin"]) if len(fq) else np.zeros((num_cells, 10))
    count = np.diff(tb["vert_begin"]).astype(np.float64)
    mean = vsum[:, :3] / count[:, None]
    out_col = (vsum[:, 3:] / count[:, None]).astype(np.float32)
    x64, status, err = np.empty((num_cells, 3)), np.empty(num_cells, np.int32), np.empty(num_cells)
    ratios, margin = np.full((num_cells, 3), np.nan), np.full(num_cells, np.nan)
    nx, ny = int(dims[0]), int(dims[1])
    for ci in range(num_cells):
        q = [float(t) for t in qsum[ci]]
        m = [float(t) for t in mean[ci]]
        x = list(m)
        M = [q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]]
        U = jacobi3(M)
        lmax = max(M[0], max(M[4], M[8]))
        kept = 0
        if lmax > 0.0:
            floor_l = eig_eps * lmax
            g = [-(q[6] + _dot3(q[0], q[1], q[2], *m)), -(q[7] + _dot3(q[1], q[3], q[4], *m)), -(q[8] + _dot3(q[2], q[4], q[5], *m))]
            for j in range(3):
                lam = M[j * 4]
                ratios[ci, j] = lam / lmax
                if not lam > floor_l:
                    continue
                t = _dot3(U[j], U[3 + j], U[6 + j], *g) / lam
                for k in range(3):
                    x[k] = x[k] + U[3 * k + j] * t
                kept += 1
        key = int(tb["cells"][ci])
        idx = (key % nx, (key // nx) % ny, key // (nx * ny))
        inside, worst = True, math.inf
        for k in range(3):
            lo = float(origin[k]) + float(idx[k]) * c
            lower, upper = lo - 0.5 * c, lo + 1.5 * c
            inside = inside and math.isfinite(x[k]) and lower <= x[k] <= upper
            if math.isfinite(x[k]):
                worst = min(worst, (x[k] - lower) / c, (upper - x[k]) / c)
            else:
                worst = -math.inf
        if kept:
            margin[ci] = worst
        st = kept
        if not inside:
            st, x = -1, list(m)
        ax, ay, az = _dot3(q[0], q[1], q[2], *x), _dot3(q[1], q[3], q[4], *x), _dot3(q[2], q[4], q[5], *x)
        err[ci] = (_dot3(x[0], x[1], x[2], ax, ay, az) + 2.0 * _dot3(q[6], q[7], q[8], *x)) + q[9]
        x64[ci], status[ci] = x, st
    return {"positions": x64.astype(np.float32), "colors": out_col, "quadrics": qsum, "means": mean, "err": err, "status": status, "x64": x64,
            "ratios": ratios, "margin": margin}


# ------------------------------------------------------------------------------------------------------------------ faces
def output_faces(rank: np.ndarray, faces: np.ndarray, num_cells: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (faces int32 [F', 3] over the kept cells, kept int64 [C']: the cells that stay, ascending).  A face with two equal cells is
    dropped; among faces with the same vertex set the lowest input index stays, whatever its orientation; input order; with faces, the
    cells no face uses are removed; without, all stay."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 3), np.int32), np.arange(num_cells, dtype=np.int64)
    r = rank[f]
    alive = np.flatnonzero((r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2]))
    seen, keep = set(), []
    for i in alive:
        s = tuple(sorted(int(t) for t in r[i]))
        if s not in seen:
            seen.add(s)
            keep.append(i)
    r = r[np.asarray(keep, np.int64)].reshape(-1, 3)
    used = np.zeros(num_cells, bool)
    used[r.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return remap[r].astype(np.int32), np.flatnonzero(used).astype(np.int64)


def simplify(vertices: np.ndarray, colors: np.ndarray, faces: np.ndarray, c: float, eig_eps: float = EIG_EPS) -> Dict[str, Any]:
    """The whole chain at cell size c -> dict(vertices fp32, colors fp32, faces int32, x64, cluster: the per-cell record, tables, origin, dims)."""
    origin, dims = grid_for(vertices, c)
    tb = tables(cell_keys(vertices, origin, c, dims), faces)
    cl = cluster(vertices, colors, faces, tb, origin, c, dims, eig_eps)
    out_faces, kept = output_faces(tb["rank"], faces, len(tb["cells"]))
    return {"vertices": cl["positions"][kept], "colors": cl["colors"][kept], "faces": out_faces, "x64": cl["x64"][kept], "kept": kept, "cluster": cl,
            "tables": tb, "origin": origin, "dims": dims}


# ------------------------------------------------------------------------------------------------------------------ the bisection
def count_cells(vertices: np.ndarray, c: float) -> Optional[int]:
    """Occupied cells at cell size c, or None when the grid exceeds the limits."""
    grid = grid_for(vertices, c)
    if grid is None:
        return None
    return len(np.unique(cell_keys(vertices, grid[0], c, grid[1])))


def bbox_diagonal(vertices: np.ndarray) -> float:
    v = np.asarray(vertices, np.float32).astype(np.float64)
    d = [float(t) for t in v.max(0) - v.min(0)]
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def choose_cell(vertices: np.ndarray, target: int) -> float:
    """The cell size for at most `target` occupied cells: 32 rounds of bisection between 0 and the bounding-box diagonal."""
    if target < 8:
        raise ValueError("target_vertices must be >= 8")
    lo, hi = 0.0, bbox_diagonal(vertices)
    for _ in range(BISECTION_ROUNDS):
        mid = (lo + hi) / 2
        n = count_cells(vertices, mid) if mid > 0 else None
        if n is None or n > target:
            lo = mid
        else:
            hi = mid
    return hi


# ------------------------------------------------------------------------------------------------------------------ fixtures
def fixture_colors(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(0, 1, (n, 3)).astype(np.float32)


def cube_mesh(half: float = 30.0, quads: int = 24):
    """A welded cube of +-half, each face quads x quads quads, outward -> (vertices fp32, faces int32)."""
    n = quads
    ids: Dict[Tuple[int, int, int], int] = {}
    lattice = sorted({p for a in range(3) for s in (0, n) for i in range(n + 1) for j in range(n + 1)
                      for p in [tuple(np.roll([s, i, j], a).tolist())]})
    for p in lattice:
        ids[p] = len(ids)
    faces = []
    for a in range(3):
        for s in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = [ids[tuple(np.roll([s, i + di, j + dj], a).tolist())] for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1))]
                    if s == 0:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    v = (np.array(lattice, np.float64) * (2 * half / n) - half).astype(np.float32)
    return v, np.array(faces, np.int32)


def plate_mesh(half: float = 30.0, quads: int = 12, gap: float = 1.0):
    """Two quads x quads sheets of +-half, `gap` apart in z, facing outward."""
    n = quads
    xs = np.arange(n + 1) * (2 * half / n) - half
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    sheet = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
    v = np.concatenate([np.concatenate([sheet, np.full((len(sheet), 1), z)], 1) for z in (gap / 2, -gap / 2)])
    faces = []
    for side in (0, 1):
        base = side * (n + 1) ** 2
        for i in range(n):
            for j in range(n):
                a, b, c, d = (base + (i + di) * (n + 1) + (j + dj) for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)))
                faces += [(a, b, c), (a, c, d)] if side == 0 else [(a, c, b), (a, d, c)]
    return v.astype(np.float32), np.array(faces, np.int32)


def sphere_mesh(radius: float = 40.0, num_lat: int = 60, num_lon: int = 60):
    """A UV sphere, outward (make_blob_mesh's indexing, no bumps)."""
    th = np.linspace(0, np.pi, num_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, num_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    d = np.concatenate([[[0.0, 0.0, 1.0]], d, [[0.0, 0.0, -1.0]]])
    ring = lambda i, j: 1 + i * num_lon + (j % num_lon)            # noqa: E731
    faces = []
    for j in range(num_lon):
        faces.append((0, ring(0, j), ring(0, j + 1)))
        faces.append((len(d) - 1, ring(num_lat - 2, j + 1), ring(num_lat - 2, j)))
    for i in range(num_lat - 2):
        for j in range(num_lon):
            faces.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            faces.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return (d * radius).astype(np.float32), np.array(faces, np.int32)


STRIDE_CELL = 10.0
STRIDE_FANS = (63, 64, 65, 130)


def stride_mesh():
    """The hand-built mesh of the lane-stride edges, for cell size STRIDE_CELL: four cone fans whose apex cells hold 63, 64, 65 and 130
    corner records (the apex alone in its cell, the rim 30 mm away), one far triangle whose three corners lie in three cells of one
    record each, 130 points in one cell that no face uses (vertex records that stride, no corner record), and a cell whose solve is
    rejected by the box test."""
    rng = np.random.default_rng(11)
    verts, faces = [], []
    for h, n in enumerate(STRIDE_FANS):
        apex = np.array([200.0 * h + 3.1, 2.7, 14.3])
        base = len(verts)
        verts.append(apex)
        ang = np.linspace(0.2, 5.6, n + 1) + rng.uniform(-0.004, 0.004, n + 1)
        for t in ang:
            verts.append(apex + np.array([30.0 * math.cos(t), 30.0 * math.sin(t), -12.0 + 3.0 * math.sin(3 * t)]))
        faces += [(base, base + 1 + i, base + 2 + i) for i in range(n)]
    base = len(verts)
    verts += [np.array([903.3, 1.9, 2.2]), np.array([951.7, 3.4, 6.1]), np.array([927.2, 44.6, 21.8])]
    faces.append((base, base + 1, base + 2))
    # what follows is placed relative to the grid, whose origin the fans fix (everything below lies above their minimum on every axis)
    c = STRIDE_CELL
    origin = np.array(verts).astype(np.float32).astype(np.float64).min(0) - c / 2
    lo = lambda x: origin + np.floor((np.array([x, 20.0, 20.0]) - origin) / c) * c   # noqa: E731
    verts += list(lo(1000.0) + 5.0 + rng.uniform(-2.0, 2.0, (130, 3)))
    # two unconnected triangles with a corner each in one cell, their planes 0.1 rad apart: both eigenvalues are kept and the planes meet
    # 18 mm from those corners, outside the box test: the cell falls back to its mean (status -1)
    a0 = lo(1100.0) + np.array([8.0, 5.0, 5.0])
    b0 = lo(1100.0) + np.array([8.3, 4.2, 6.83])
    base = len(verts)
    verts += [a0, a0 + np.array([25.0, 3.0, 0.0]), a0 + np.array([4.0, 27.0, 0.0]),
              b0, b0 + np.array([26.0, -3.0, 2.6]), b0 + np.array([3.0, -28.0, 0.3])]
    faces += [(base, base + 1, base + 2), (base + 3, base + 5, base + 4)]
    return np.array(verts, np.float64).astype(np.float32), np.array(faces, np.int32)


def check_fixture(vertices: np.ndarray, origin: np.ndarray, c: float, cl: Dict[str, Any], eig_eps: float = EIG_EPS) -> Dict[str, float]:
    """The conditions under which the device comparison needs no exclusions; raises AssertionError, returns the measured margins."""
    g = grid_coordinates(vertices, origin, c)
    near_int = float(np.abs(g - np.rint(g)).min())
    assert near_int > 1e-7, f"a grid coordinate lies {near_int} from an integer"
    r = cl["ratios"][np.isfinite(cl["ratios"])]
    near_eps = float(np.abs(r / eig_eps - 1.0).min()) if len(r) else math.inf
    assert near_eps > 1e-6, f"an eigenvalue ratio lies a relative {near_eps} from eig_eps"
    m = cl["margin"][np.isfinite(cl["margin"])]
    near_box = float(np.abs(m).min()) if len(m) else math.inf
    assert near_box > 1e-7, f"a solved position lies {near_box} c from a bound of the box test"
    assert not np.any(np.isinf(cl["margin"])), "a solve gave a non-finite position"
    return {"grid": near_int, "eig": near_eps, "box": near_box}
