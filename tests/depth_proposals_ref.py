"""numpy restatement of the depth proposals of DESIGN.md section 28 (csrc/depth_proposals.hip): planes by keyed RANSAC and a twofold
least-squares refit, foreground, connected components, the components' table and COCO run lengths.  Plain numpy / scipy: the yardstick of
the tests, not a fast path.

fp64 with one rounding per operation, in the order the header states, so the points, the heights, the hypotheses' planes and every integer
that follows from them are the device's bit for bit.  Only the refit is not: numpy.linalg.eigh and pairwise sums here, cyclic Jacobi and
chunked sums there; refit_sensitivity() measures what the order of summation alone moves.
"""

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from foundpose_amd.infer_pose_util import binary_mask_to_rle
from tests.kabsch_ref import sample3                 # the keyed draw: valid and not repeated, 1 + 64 draws per index
from tests.pnp_ref import hyp_key, pair_base         # uint64 arithmetic of ransac.hpp

THIN2 = 1e-12
DEFAULTS = dict(num_planes=1, plane_hypotheses=256, plane_stride=4, plane_thresh_mm=10.0, min_plane_share=0.05, max_depth_mm=0.0,
                object_margin_mm=15.0, connect_mm=(5.0,), connect_slope=4.0, min_pixels=200, max_area_share=0.5, max_proposals=64, seed=0)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    if not isinstance(o["connect_mm"], (tuple, list)):
        o["connect_mm"] = (o["connect_mm"],)
    return o


# ------------------------------------------------------------------------------------------------------------------------------ geometry
def valid_mask(D, max_depth_mm=0.0):
    D = np.asarray(D, np.float32)
    return (D > 0) & ((max_depth_mm == 0.0) | (D.astype(np.float64) <= max_depth_mm))


def points(D, cam):
    """-> X [H, W, 3] fp64: ((u - cx) / fx z, (v - cy) / fy z, z), every operation rounded on its own."""
    fx, fy, cx, cy = (np.float64(c) for c in cam)
    H, W = D.shape
    z = np.asarray(D, np.float32).astype(np.float64)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    return np.stack([((u - cx) / fx) * z, ((v - cy) / fy) * z, z], -1)


def height(pl, X):
    """((n0 x + n1 y) + n2 z) + d"""
    pl = np.asarray(pl, np.float64)
    return ((pl[0] * X[..., 0] + pl[1] * X[..., 1]) + pl[2] * X[..., 2]) + pl[3]


def eligible_mask(D, cam, prior, thresh, max_depth_mm=0.0):
    el = valid_mask(D, max_depth_mm)
    X = points(D, cam)
    for pl in prior:
        el &= ~(np.abs(height(pl, X)) <= thresh)
    return el


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def plane_from_ids(X, ids):
    """X [H W, 3]; -> (n0, n1, n2, d) with d >= 0, or None (dead)."""
    X0, X1, X2 = (X[i] for i in ids)
    e1, e2 = X1 - X0, X2 - X0
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    nn, l1, l2 = _dot(n, n), _dot(e1, e1), _dot(e2, e2)
    if not nn > THIN2 * (l1 * l2):
        return None
    norm = np.sqrt(nn)
    if not norm > 1e-300:
        return None
    n = n / norm
    d = -_dot(n, X0)
    if d < 0.0:
        n, d = -n, -d
    return np.array([n[0], n[1], n[2], d])


def hypotheses(D, cam, frame_key, k, prior, o):
    """All hypotheses of plane k of a frame -> dict(ids [list or None], planes [array or None], counts int64 [hyp], eligible, valid)."""
    H, W = D.shape
    el = eligible_mask(D, cam, prior, o["plane_thresh_mm"], o["max_depth_mm"])
    X = points(D, cam)
    Xf, elf = X.reshape(-1, 3), el.reshape(-1)
    s = o["plane_stride"]
    Xs, els = X[::s, ::s].reshape(-1, 3), el[::s, ::s].reshape(-1)
    base = pair_base(o["seed"], (int(frame_key) * 8 + k) & ((1 << 64) - 1))
    ids, planes, counts = [], [], np.zeros(o["plane_hypotheses"], np.int64)
    for h in range(o["plane_hypotheses"]):
        i3 = sample3(hyp_key(base, h), H * W, elf)
        pl = plane_from_ids(Xf, i3) if i3 is not None else None
        ids.append(i3)
        planes.append(pl)
        if pl is not None:
            counts[h] = int(np.sum(els & (np.abs(height(pl, Xs)) <= o["plane_thresh_mm"])))
    return dict(ids=ids, planes=planes, counts=counts, eligible=int(el.sum()), valid=int(valid_mask(D, o["max_depth_mm"]).sum()),
                el=el, X=X)


def refit_once(pl, X, el, thresh, ascending=False):
    """One least-squares refit over the eligible pixels within the threshold of pl -> (plane, count).  ascending: sums in index order
    (a Python loop's order) instead of numpy's pairwise order."""
    m = el & (np.abs(height(pl, X)) <= thresh)
    P = X[m]
    if len(P) < 3:
        return np.array(pl, np.float64), len(P)
    if ascending:
        c = np.cumsum(P, 0)[-1] / len(P)
        Q = P - c
        S = np.cumsum(Q[:, :, None] * Q[:, None, :], 0)[-1]
    else:
        c = P.sum(0) / len(P)
        Q = P - c
        S = Q.T @ Q
    w, V = np.linalg.eigh(S)
    n = V[:, 0]
    d = -float(n @ c)
    if d < 0:
        n, d = -n, -d
    return np.array([n[0], n[1], n[2], d]), len(P)


def fit_plane(D, cam, frame_key, k, prior, o, ascending=False):
    """Plane k of a frame -> dict(plane, winner, subgrid_count, support, eligible, valid, accepted, counts, ids, planes)."""
    hy = hypotheses(D, cam, frame_key, k, prior, o)
    win = int(np.argmax(hy["counts"]))   # the first of the highest
    out = dict(winner=win, subgrid_count=int(hy["counts"][win]), eligible=hy["eligible"], valid=hy["valid"], counts=hy["counts"], ids=hy["ids"],
               planes=hy["planes"], plane=np.zeros(4), support=0, accepted=False, hypothesis_plane=hy["planes"][win])
    pl = hy["planes"][win]
    if pl is None:
        return out
    for _ in range(2):
        pl, _n = refit_once(pl, hy["X"], hy["el"], o["plane_thresh_mm"], ascending)
    support = int(np.sum(hy["el"] & (np.abs(height(pl, hy["X"])) <= o["plane_thresh_mm"])))
    out.update(plane=pl, support=support,
               accepted=bool(support >= 3 and np.float64(support) >= np.float64(o["min_plane_share"]) * np.float64(hy["valid"])))
    return out


def fit_planes(D, cam, frame_key, o):
    """The frame's sequence: -> (accepted planes [list of 4-vectors], the records of every plane tried)."""
    planes, records = [], []
    for k in range(o["num_planes"]):
        r = fit_plane(D, cam, frame_key, k, planes, o)
        records.append(r)
        if not r["accepted"]:
            break
        planes.append(r["plane"])
    return planes, records


def plane_difference(a, b):
    """-> (angle between the normals in rad, |d_a - d_b| in mm)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a[:3], b[:3])), a[:3] @ b[:3])), float(abs(a[3] - b[3]))


def refit_sensitivity(D, cam, frame_key, k, prior, o):
    """What the order of summation alone moves in the restatement's refit: (rad, mm) between pairwise and ascending sums."""
    return plane_difference(fit_plane(D, cam, frame_key, k, prior, o)["plane"], fit_plane(D, cam, frame_key, k, prior, o, ascending=True)["plane"])


# ---------------------------------------------------------------------------------------------------------------------------- components
def foreground(D, cam, planes, margin, max_depth_mm=0.0):
    fg = valid_mask(D, max_depth_mm)
    X = points(D, cam)
    for pl in planes:
        fg &= height(pl, X) > margin
    return fg


def _connected(za, zb, connect_mm, slope_fx):
    za, zb = za.astype(np.float32), zb.astype(np.float32)
    return np.abs(za - zb) <= (np.float32(connect_mm) + np.float32(slope_fx) * np.minimum(za, zb))


def components(D, fg, connect_mm, slope_fx):
    """-> labels int32 [H, W]: the smallest linear index of the pixel's component, -1 for background."""
    D = np.asarray(D, np.float32)
    H, W = D.shape
    idx = np.arange(H * W).reshape(H, W)
    eh = fg[:, 1:] & fg[:, :-1] & _connected(D[:, 1:], D[:, :-1], connect_mm, slope_fx)
    ev = fg[1:, :] & fg[:-1, :] & _connected(D[1:, :], D[:-1, :], connect_mm, slope_fx)
    a = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    b = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(H * W, H * W))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1, H * W, np.int64)
    np.minimum.at(smallest, comp, idx.reshape(-1))
    lab = smallest[comp].reshape(H, W).astype(np.int32)
    lab[~fg] = -1
    return lab


def slope_fx_of(o, cam):
    return np.float32(np.float64(o["connect_slope"]) / np.float64(cam[0]))


def table(labels, min_pixels, max_area, max_proposals, level=0, finer=()):
    """-> (rows int32 [kept, 7] = (label, area, x0, y0, x1, y1, level) by rank, counts (components, within limits, kept, dropped as a
    finer level's), rank_map int32 [H, W])."""
    H, W = labels.shape
    flat = labels.reshape(-1)
    roots, area = np.unique(flat[flat >= 0], return_counts=True)
    known = {(int(r[0]), int(r[1])) for t in finer for r in t}
    cand, within, dup = [], 0, 0
    for L, a in zip(roots.tolist(), area.tolist()):
        if a < min_pixels or a > max_area:
            continue
        within += 1
        if (L, a) in known:
            dup += 1
            continue
        cand.append((-a, L))
    cand.sort()
    rows, rank_map = [], np.full((H, W), -1, np.int32)
    for r, (na, L) in enumerate(cand[:max_proposals]):
        ys, xs = np.nonzero(labels == L)
        rows.append([L, -na, xs.min(), ys.min(), xs.max(), ys.max(), level])
        rank_map[labels == L] = r
    return np.array(rows, np.int32).reshape(-1, 7), (len(roots), within, len(rows), dup), rank_map


def runs(rank_map, kept):
    """-> the uncompressed counts of every rank below kept."""
    return [binary_mask_to_rle(rank_map == r)["counts"] for r in range(kept)]


def max_area_of(o, H, W):
    return int(np.floor(np.float64(o["max_area_share"]) * np.float64(H * W)))


def propose_frame(D, cam, frame_key, o, planes=None):
    """One frame end to end.  planes: use these accepted planes instead of fitting (the GPU tests pass the kernel's own)."""
    H, W = D.shape
    records = None
    if planes is None:
        planes, records = fit_planes(D, cam, frame_key, o)
    fg = foreground(D, cam, planes, o["object_margin_mm"], o["max_depth_mm"])
    levels, finer = [], []
    for lv, cmm in enumerate(o["connect_mm"]):
        lab = components(D, fg, cmm, slope_fx_of(o, cam))
        rows, counts, rank_map = table(lab, o["min_pixels"], max_area_of(o, H, W), o["max_proposals"], lv, finer)
        finer.append(rows)
        levels.append(dict(labels=lab, table=rows, counts=counts, rank_map=rank_map, runs=runs(rank_map, len(rows))))
    return dict(planes=planes, records=records, foreground=fg, levels=levels)


# -------------------------------------------------------------------------------------------------------------------------------- scenes
E2E_CAM = (143.0, 143.0, 83.3, 58.3)
E2E_SIZE = (120, 160)
E2E_SPHERES = [(40.0, -150.0, -60.0), (45.0, 0.0, 40.0), (35.0, 150.0, -20.0), (30.0, 62.0, 95.0)]   # radius, in-plane offsets (mm)
E2E_KEY = (1 << 32) + 7


def e2e_scene(wall=False, seed=5, scale=1):
    """The analytic scene of section 28: a plane through (0, 0, 1000) tilted 35 degrees about x, four spheres resting on it, noise
    sigma 1 mm quantised to 0.1 mm, a 15 x 10 hole; with `wall` a fronto-parallel wall at 1150 mm behind it.
    scale: the same scene at `scale` times the resolution (camera E2E_CAM * scale).
    -> (depth fp32 [H, W], the planted plane (n, d), [the visible pixels of each sphere])."""
    H, W = E2E_SIZE[0] * scale, E2E_SIZE[1] * scale
    fx, fy, cx, cy = (c * scale for c in E2E_CAM)
    a = np.deg2rad(35.0)
    n = np.array([0.0, -np.sin(a), -np.cos(a)])            # towards the camera
    ex, ey = np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(a), -np.sin(a)])
    p0 = np.array([0.0, 0.0, 1000.0])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (n @ p0) / (ray @ n)
    z = np.where(t > 0, t, np.inf)
    if wall:
        z = np.minimum(z, 1150.0)
    owner = np.full((H, W), -1)
    for i, (r, ox, oy) in enumerate(E2E_SPHERES):
        c = p0 + ox * ex + oy * ey + r * n
        b = ray @ c
        aa = (ray * ray).sum(-1)
        disc = b * b - aa * (c @ c - r * r)
        with np.errstate(invalid="ignore"):
            ts = (b - np.sqrt(disc)) / aa
        hit = (disc > 0) & (ts > 0) & (ts < z)
        z = np.where(hit, ts, z)
        owner[hit] = i
    rng = np.random.default_rng(seed)
    z = z + rng.normal(0.0, 1.0, z.shape)
    D = (np.rint(z * 10.0) / 10.0).astype(np.float32)
    D[~np.isfinite(D)] = 0
    D[8 * scale:18 * scale, 20 * scale:35 * scale] = 0.0    # 15 wide, 10 high
    owner[D == 0] = -1
    d = -float(n @ p0)
    plane = np.array([n[0], n[1], n[2], d]) if d >= 0 else np.array([-n[0], -n[1], -n[2], -d])
    return D, plane, [owner == i for i in range(len(E2E_SPHERES))]


def iou(a, b):
    return float((a & b).sum()) / max(int((a | b).sum()), 1)


# ------------------------------------------------------------------------------------------------------------- hand-made component frames
PATTERN_SIZES = [(56, 80), (67, 131)]     # (H, W): no side a multiple of the 32-pixel tile, several tiles each way
PATTERN_CMM, PATTERN_SLOPE_FX = np.float32(5.0), np.float32(4.0 / 143.0)
Z0 = np.float32(1000.0)


def serpentine(H, W):
    """One component: one-pixel corridors on every other row, joined alternately at the right and the left end."""
    m = np.zeros((H, W), bool)
    m[::2, :] = True
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = True
    return m


def comb(H, W):
    """One component: a spine along the top row, one-pixel teeth on every other column down to the last row."""
    m = np.zeros((H, W), bool)
    m[0, :] = True
    m[:, ::2] = True
    return m


def spiral(H, W):
    """One component: a rectangular spiral of one-pixel corridors with one-pixel walls."""
    m = np.zeros((H, W), bool)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    first = True
    while y1 - y0 >= 2 and x1 - x0 >= 2:
        m[y0, (x0 if first else x0 - 1):x1 + 1] = True
        m[y0:y1 + 1, x1] = True
        m[y1, x0:x1 + 1] = True
        m[y0 + 2:y1 + 1, x0] = True
        first = False
        m[y0 + 2, x0:x0 + 2] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return m


def pattern_masks(H, W):
    """name -> foreground mask [H, W]."""
    yy, xx = np.mgrid[:H, :W]
    ring = np.zeros((H, W), bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    ring[H // 2, :] = True                                   # ... and a bar through the middle: still one component
    holes = np.ones((H, W), bool)
    holes[5:9, 7:40] = False
    holes[30:50, 33:35] = False
    holes[::7, ::5] = False
    wrap = np.zeros((H, W), bool)
    wrap[10, W - 1] = wrap[11, 0] = True                     # adjacent in memory, no neighbours
    blocks = np.zeros((H, W), bool)                          # many components with ties in area: 3 x 3 and 3 x 4 blocks
    for by in range(1, H - 4, 5):
        for bx in range(1, W - 5, 6):
            blocks[by:by + 3, bx:bx + (4 if (by + bx) % 3 == 0 else 3)] = True
    last_row = np.zeros((H, W), bool)
    last_row[-1, :] = True
    first_row = np.zeros((H, W), bool)
    first_row[0, :] = True
    return {"serpentine": serpentine(H, W), "comb": comb(H, W), "spiral": spiral(H, W), "checkerboard": (yy + xx) % 2 == 0,
            "all": np.ones((H, W), bool), "none": np.zeros((H, W), bool), "ring": ring, "holes": holes, "wrap": wrap, "blocks": blocks,
            "last_row": last_row, "first_row": first_row}


def ulp_frame(H, W):
    """Pairs of neighbours whose depth step sits at the fp32 threshold: -> (D, slope_fx, expected: {(y, x): connected to (y, x + 1)}).
    With slope 0 the threshold is connect_mm itself: a step of exactly 5 connects, one ulp more does not.  The frame's slope is 0; the
    companion frame ulp_frame_slope uses the sloped threshold."""
    D = np.zeros((H, W), np.float32)
    D[3, 3], D[3, 4] = Z0, Z0 + PATTERN_CMM
    D[6, 3], D[6, 4] = Z0, np.nextafter(Z0 + PATTERN_CMM, np.float32(np.inf))
    D[9, 31], D[9, 32] = Z0 + PATTERN_CMM, Z0                                            # across a tile border, descending
    D[12, 31], D[12, 32] = np.nextafter(Z0 + PATTERN_CMM, np.float32(np.inf)), Z0
    D[31, 5], D[32, 5] = Z0, Z0 + PATTERN_CMM                                            # vertical, across a tile border
    D[31, 9], D[32, 9] = Z0, np.nextafter(Z0 + PATTERN_CMM, np.float32(np.inf))
    return D, np.float32(0.0), {(3, 3): True, (6, 3): False, (9, 31): True, (12, 31): False}


def ulp_frame_slope(H, W):
    """The same with the sloped threshold t = fl(connect_mm + fl(slope_fx * za)): zb is the largest fp32 with zb - za <= t (the
    difference of two fp32 this close is exact), and its successor."""
    za = Z0
    t = np.float32(PATTERN_CMM + np.float32(PATTERN_SLOPE_FX * za))
    zb = np.float32(za + t)
    while np.float32(zb - za) > t:
        zb = np.nextafter(zb, np.float32(0))
    while np.float32(np.nextafter(zb, np.float32(np.inf)) - za) <= t:
        zb = np.nextafter(zb, np.float32(np.inf))
    D = np.zeros((H, W), np.float32)
    D[3, 3], D[3, 4] = za, zb
    D[6, 3], D[6, 4] = za, np.nextafter(zb, np.float32(np.inf))
    D[31, 40], D[32, 40] = zb, za
    D[31, 44], D[32, 44] = np.nextafter(zb, np.float32(np.inf)), za
    return D, PATTERN_SLOPE_FX, {(3, 3): True, (6, 3): False}


def pattern_batches():
    """[(name, D fp32 [3, H, W], slope_fx fp32 [3])]: batches of three frames with different content, per size.  Foreground = D > 0
    (no planes); the depth is Z0 with a gentle ramp that never exceeds the threshold."""
    out = []
    for H, W in PATTERN_SIZES:
        m = pattern_masks(H, W)
        ramp = (Z0 + 0.5 * np.arange(W, dtype=np.float32)[None, :] + 0.25 * np.arange(H, dtype=np.float32)[:, None]).astype(np.float32)
        frames = lambda names: np.stack([np.where(m[n], ramp, np.float32(0)) for n in names]).astype(np.float32)
        s3 = np.full(3, PATTERN_SLOPE_FX, np.float32)
        out.append((f"winding {W}x{H}", frames(["serpentine", "spiral", "comb"]), s3))
        out.append((f"dense {W}x{H}", frames(["checkerboard", "all", "none"]), s3))
        out.append((f"borders {W}x{H}", frames(["ring", "wrap", "holes"]), s3))
        out.append((f"rows {W}x{H}", frames(["last_row", "first_row", "blocks"]), s3))
        u0, s0, _ = ulp_frame(H, W)
        u1, s1, _ = ulp_frame_slope(H, W)
        out.append((f"ulp {W}x{H}", np.stack([u0, u1, frames(["blocks"])[0]]), np.array([s0, s1, PATTERN_SLOPE_FX], np.float32)))
    return out


# ------------------------------------------------------------------------------------------------------------------- further fixed frames
def foreground_frames(H=40, W=48):
    """Fronto-parallel planes make the height exact: (0, 0, -1, 1200) gives h = 1200 - z and (0, 0, 1, -1000) gives h = z - 1000, both
    without rounding for an fp32 z near 1000.  -> [(D, planes, margin, max_depth_mm, the foreground wanted)]: pixels at h = margin, one
    ulp above and one ulp below it for either plane, and at max_depth_mm and one ulp beyond."""
    up, down = np.float32(np.inf), np.float32(0)
    p_far, p_near = np.array([0.0, 0.0, -1.0, 1200.0]), np.array([0.0, 0.0, 1.0, -1000.0])
    D = np.full((H, W), 1100.0, np.float32)
    D[0, :8] = [1185.0, np.nextafter(np.float32(1185.0), down), np.nextafter(np.float32(1185.0), up), 0.0,
                1015.0, np.nextafter(np.float32(1015.0), down), np.nextafter(np.float32(1015.0), up), 1300.0]
    D[33, 31:34] = [1185.0, np.nextafter(np.float32(1185.0), down), np.nextafter(np.float32(1185.0), up)]    # on a tile corner
    z = D.astype(np.float64)
    two = (D > 0) & (1200.0 - z > 15.0) & (z - 1000.0 > 15.0)
    E = np.full((H, W), 1050.0, np.float32)
    E[5, :4] = [1100.0, np.nextafter(np.float32(1100.0), up), np.nextafter(np.float32(1100.0), down), 0.0]
    one = (E > 0) & (E.astype(np.float64) <= 1100.0) & (1200.0 - E.astype(np.float64) > 15.0)
    return [(D, [p_far, p_near], 15.0, 0.0, two), (E, [p_far], 15.0, 1100.0, one)]


def sparse_scene(share=0.6, seed=11):
    """The analytic scene with `share` of its pixels punched out."""
    D, plane, visible = e2e_scene()
    D = D.copy()
    D[np.random.default_rng(seed).random(D.shape) < share] = 0.0
    return D, plane
