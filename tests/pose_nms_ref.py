"""numpy fp64 restatement of fp_pose_overlap's and fp_pose_nms_greedy's contracts (include/foundpose_amd.h), and the
fixture the CPU and GPU tests share.  Every step of the overlap is one rounded fp64 operation in the stated order, so a correct
implementation makes every decision identically: its integer outputs are EQUAL and the overlap, one division of two of them, is the same
bits.  The greedy pass is integer logic on those bits.

Besides the results the overlap restatement returns `min_margin`: the smallest relative distance (pose_verify_ref.Margin) of any compared
quantity from its decision boundary -- a point of j's sample, (x - x0) / h, from the cell edges 1 .. G - 1 (beyond them the clamp decides);
a point of i's sample seen from j, (y - x0) / h, from the integers 0 .. G (no clamp: 0 and G are the cube's faces); d^2 from s^2; and (in
the fixture builder) every scored overlap from the threshold.  A NaN among the sphere quantities is NOT a small margin: `!(NaN <= s s)` is
status 1 in every implementation, whatever its rounding; such a pair adds nothing to the margin.
"""

import numpy as np

from tests import pose_verify_ref as pv
from tests.pose_verify_ref import Margin


def _mat3(M, x):
    """Products summed k ascending, per row; x [..., 3] -> [..., 3]."""
    return np.stack([(M[i, 0] * x[..., 0] + M[i, 1] * x[..., 1]) + M[i, 2] * x[..., 2] for i in range(3)], -1)


def overlap_pair(Xi, Xj, ci, rho_i, cj, rho_j, Ri, ti, Rj, tj, G, margin=None):
    """One ordered pair of valid poses with non-empty samples.  Xi [n_i, 3], Xj [n_j, 3] float32: the samples of i's and j's objects; c,
    rho: their spheres; R, t: the poses, in one common frame.  -> (n_in, n_cells, overlap, status)."""
    margin = Margin() if margin is None else margin
    Ri, ti, Rj, tj, ci, cj = (np.asarray(v, np.float64) for v in (Ri, ti, Rj, tj, ci, cj))
    rho_i, rho_j = np.float64(rho_i), np.float64(rho_j)
    with np.errstate(all="ignore"):
        if not rho_j > 0.0:
            return 0, 0, 0.0, 2
        Ci, Cj = _mat3(Ri, ci) + ti, _mat3(Rj, cj) + tj
        d = Ci - Cj
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        s = rho_i + rho_j
        if not np.isnan(d2):
            margin.add(abs(d2 - s * s) / max(1.0, s * s))
        if not d2 <= s * s:
            return 0, 0, 0.0, 1
        x0 = cj - rho_j
        h = 2.0 * rho_j / np.float64(G)
        # pass 1: the cells j's sample occupies in j's own model frame
        q = (np.asarray(Xj, np.float32).astype(np.float64) - x0) / h
        margin.add(np.abs(q - np.clip(np.rint(q), 1.0, G - 1.0)) / np.maximum(1.0, np.abs(q)))
        idx = np.fmin(np.fmax(np.floor(q), 0.0), G - 1.0).astype(np.int64)
        occ = np.zeros(G * G * G, bool)
        occ[(idx[:, 2] * G + idx[:, 1]) * G + idx[:, 0]] = True
        # pass 2: i's sample at i's pose, taken back into j's model frame
        X = _mat3(Ri, np.asarray(Xi, np.float32).astype(np.float64)) + ti
        y = _mat3(Rj.T, X - tj)   # row k of R_j^T: (R_j[0,k] d_0 + R_j[1,k] d_1) + R_j[2,k] d_2
        q = (y - x0) / h
        margin.add(np.abs(q - np.clip(np.rint(q), 0.0, np.float64(G))) / np.maximum(1.0, np.abs(q)))
        f = np.floor(q)
        inside = ((f >= 0.0) & (f < G)).all(1)   # (a NaN is not inside)
        cell = np.where(inside[:, None], f, 0.0).astype(np.int64)
        n_in = int((inside & occ[(cell[:, 2] * G + cell[:, 1]) * G + cell[:, 0]]).sum())
    return n_in, int(occ.sum()), float(np.float64(n_in) / np.float64(len(Xi))), 0


def pose_overlap_ref(points, ranges, centers, radii, pose_obj, valid, R, t, pairs, G):
    """points [M_total, 3] float32; per object: ranges [O, 2], centers [O, 3], radii [O]; per pose: pose_obj, valid, R [N, 3, 3], t [N, 3];
    pairs [P, 2].  -> dict: counts [P, 2], overlap [P], status [P], min_margin."""
    P, M = len(pairs), len(points)
    out = {"counts": np.zeros((P, 2), np.int64), "overlap": np.zeros(P), "status": np.zeros(P, np.int64)}
    margin = Margin()
    rng = [tuple(int(min(max(int(v), 0), M)) for v in r) for r in ranges]
    for p, (i, j) in enumerate(np.asarray(pairs).tolist()):
        oi, oj = int(pose_obj[i]), int(pose_obj[j])
        (bi, ei), (bj, ej) = rng[oi], rng[oj]
        if not valid[i] or not valid[j] or bi >= ei or bj >= ej:
            out["status"][p] = 2
            continue
        n_in, n_cells, ov, st = overlap_pair(points[bi:ei], points[bj:ej], centers[oi], radii[oi], centers[oj], radii[oj], R[i], t[i], R[j], t[j], G, margin)
        out["counts"][p], out["overlap"][p], out["status"][p] = (n_in, n_cells), ov, st
    out["min_margin"] = margin.value
    return out


def conflicts(n, begin, pairs, overlap, status, thr):
    """The symmetric conflict matrix of one frame's n poses [begin, begin + n): some pair (a, b) or (b, a) has status 0 and overlap >= thr."""
    conf = np.zeros((n, n), bool)
    for (a, b), ov, st in zip(np.asarray(pairs).reshape(-1, 2).tolist(), overlap, status):
        a, b = a - begin, b - begin
        if st == 0 and ov >= thr and 0 <= a < n and 0 <= b < n and a != b:
            conf[a, b] = conf[b, a] = True
    return conf


def greedy_from_conflicts(conf):
    """Poses in rank order: a pose still alive suppresses every later alive pose it conflicts with.  -> (keep [n] bool, by [n], -1 = kept)."""
    n = len(conf)
    keep, by = np.ones(n, bool), np.full(n, -1, np.int64)
    for r in range(n):
        if keep[r]:
            for c in range(r + 1, n):
                if keep[c] and conf[r, c]:
                    keep[c], by[c] = False, r
    return keep, by


def nms_greedy_ref(group_off, pair_off, pairs, overlap, status, thr):
    """-> (keep [N] int, suppressed_by [N] int: the global pose index of the suppressor, -1 for a kept pose)."""
    N = int(group_off[-1])
    keep, by = np.ones(N, np.int64), np.full(N, -1, np.int64)
    for g in range(len(group_off) - 1):
        b, e = int(group_off[g]), int(group_off[g + 1])
        pb, pe = int(pair_off[g]), int(pair_off[g + 1])
        k, s = greedy_from_conflicts(conflicts(e - b, b, pairs[pb:pe], overlap[pb:pe], status[pb:pe], thr))
        keep[b:e] = k
        by[b:e] = np.where(s >= 0, s + b, -1)
    return keep, by


# ---------------------------------------------------------------------------------------------------- the tests' frame
POSE_NAMES = ("planted", "the same again", "shifted by rho / 16", "shifted by rho / 2", "object 1 interpenetrating", "disjoint spheres", "invalid", "NaN in t")


def gpu_fixture(seed=6, grid=16, thr=0.3):
    """One frame of 8 poses in rank order (POSE_NAMES), on the blob objects of pose_verify_ref.gpu_fixture: 600 and 602 sampled points
    (object 1 sampled with stride 2), so more than two rounds of the 256-thread point loops.  Poses 0-3 and 5-7 are of object 0 at the
    fixture's planted rotation: the planted pose, the same pose again, the pose shifted sideways by rho / 16 (half a cell at G = 16) and by
    rho / 2, a pose 5 rho away (disjoint spheres), the planted pose with valid = 0 and the planted pose with a NaN in t; pose 4 is object 1
    at its own planted rotation with its centre 0.9 rho from object 0's: the two surfaces cross.  pairs: every ordered pair of the frame
    (cross_object) -- 56.  -> dict with the tables of pose_overlap_ref, group_off, pair_off, scores, grid, thr, and ref: the restatement's
    result with `min_margin` extended by every scored overlap's relative distance from thr.
    min_margin by seed (G = 8 / G = 16): see tests/test_pose_nms_cpu.py, which asserts the seeds the GPU tests use."""
    from foundpose_amd import pose_nms
    fix = pv.gpu_fixture(seed)
    points, ranges, centers, radii = pv.fixture_bank_tables(fix)
    R0, t0, R1 = fix["R"][0], fix["t"][0], fix["R"][4]
    rho = radii[0]
    # pose p of object o puts the object's centre at R c + t; object 1's centre goes 0.9 rho beside object 0's
    C0 = R0 @ centers[0] + t0
    t1 = C0 + np.array([0.9 * rho, 0.2 * rho, -0.1 * rho]) - R1 @ centers[1]
    nan_t = t0.copy()
    nan_t[1] = np.nan
    R = np.stack([R0, R0, R0, R0, R1, R0, R0, R0])
    t = np.stack([t0, t0, t0 + np.array([rho / 16.0, 0.0, 0.0]), t0 + np.array([rho / 2.0, 0.0, 0.0]), t1, t0 + np.array([5.0 * rho, 0.0, 0.0]), t0, nan_t])
    pose_obj = np.array([0, 0, 0, 0, 1, 0, 0, 0], np.int32)
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.int32)
    scores = np.array([0.9, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3])   # the layout IS the rank order (the tie keeps the input order)
    group_off = np.array([0, 8], np.int32)
    pairs, pair_off = pose_nms.frame_pairs(group_off, pose_obj, cross_object=True)
    ref = pose_overlap_ref(points, ranges, centers, radii, pose_obj, valid, R, t, pairs, grid)
    margin = Margin()
    margin.add(ref["min_margin"])
    scored = ref["status"] == 0
    margin.add(np.abs(ref["overlap"][scored] - thr) / thr)
    ref["min_margin"] = margin.value
    return dict(points=points, ranges=ranges, centers=centers, radii=radii, pose_obj=pose_obj, valid=valid, R=R, t=t, pairs=pairs, pair_off=pair_off,
                group_off=group_off, scores=scores, grid=grid, thr=thr, ref=ref)


def pair_index(fix, i, j):
    """The place of the ordered pair (i, j) in the fixture's pairs."""
    return int(np.nonzero((fix["pairs"] == (i, j)).all(1))[0][0])


def synthetic_groups(seed=0, sizes=(0, 1, 2, 65, 256), density=0.02):
    """Frames of the given sizes with every ordered pair of each, seeded random overlaps and statuses: a pair's overlap reaches thr = 0.5
    with probability `density` (so an unordered pair conflicts with about twice that: each pose of the 256-frame has about ten conflicts and
    chains of suppressions form), 15 % of the pairs are not scored (status 1 or 2) -- some of them with an overlap above thr, which must not
    count.  -> dict: group_off, pair_off, pairs, overlap, status, thr."""
    from foundpose_amd import pose_nms
    rng = np.random.default_rng(seed)
    group_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pairs, pair_off = pose_nms.frame_pairs(group_off, np.zeros(int(group_off[-1]), np.int32))
    P = len(pairs)
    high = rng.random(P) < density
    overlap = np.where(high, rng.uniform(0.5, 1.0, P), rng.uniform(0.0, 0.5 - 1e-3, P))
    status = rng.choice([0, 1, 2], P, p=[0.85, 0.1, 0.05]).astype(np.int32)
    return dict(group_off=group_off, pair_off=pair_off, pairs=pairs, overlap=overlap, status=status, thr=0.5)
