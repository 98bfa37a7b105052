"""numpy fp64 restatement of the silhouette refinement contract (csrc/mask_refine.hip computes it on the GPU),
TEST HELPER, one function per step of the contract.

Per detection: the whole-model sample X [N, 3] (model mm), the detection's mask [H, W] uint8 (non-zero = set) in the frame's pinhole
camera (fx, fy, cx, cy) with pixel centres at integer coordinates, the input pose (R, t), the Huber delta in pixels.
"""

import numpy as np

from tests import lm_ref
from tests.depth_refine_ref import lm_solve

D2_EMPTY = 1 << 30
FAR = 1 << 15


# ---------------------------------------------------------------------------------------------------------------- the distance field
def mask_distance(mask):
    """d2 [H, W] int64: the exact squared distance to the nearest set pixel; D2_EMPTY everywhere when there is none.  A column pass
    (distance in rows to the column's nearest set pixel) and per row the minimum over all columns of (x - x')^2 + g[x']^2, in integers."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    if not m.any():
        return np.full((H, W), D2_EMPTY, np.int64)
    ys = np.arange(H, dtype=np.int64)
    g = np.full((H, W), FAR, np.int64)
    for x in range(W):
        rows = ys[m[:, x]]
        if rows.size:
            g[:, x] = np.abs(ys[:, None] - rows[None, :]).min(1)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                # [x, x']
    return np.stack([(dx2 + (g[y] ** 2)[None, :]).min(1) for y in range(H)])


def mask_distance_brute(mask):
    """The definition: the minimum over all set pixels, pixel pair by pixel pair."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    if not m.any():
        return np.full((H, W), D2_EMPTY, np.int64)
    sy, sx = np.nonzero(m)
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2).min(-1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the contour rows
def contour_pixels(mask):
    """(x, y) int32 [K, 2] in row-major order: the set pixels with at least one of their four neighbours inside the image unset."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    rows = []
    for y in range(H):
        for x in range(W):
            if m[y, x] and any(0 <= yy < H and 0 <= xx < W and not m[yy, xx] for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1))):
                rows.append((x, y))
    return np.array(rows, np.int32).reshape(-1, 2)


def subsample_indices(K, K_max):
    """Which of K contour rows are kept under the cap K_max: all, or floor(j K / K_max) for j < K_max (python integers)."""
    return list(range(K)) if K <= K_max else [(j * K) // K_max for j in range(K_max)]


def contour_rows(mask, K_max):
    c = contour_pixels(mask)
    return c[subsample_indices(len(c), K_max)].reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------- the two terms
def project(R, t, X, cam):
    """-> Xc [N, 3], u, v [N], front [N] bool (z > 1)."""
    fx, fy, cx, cy = cam
    Xc = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy
    return Xc, u, v, z > 1.0


def huber(r_abs, delta):
    """-> rho, w of |r|."""
    inl = r_abs <= delta
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inl, r_abs ** 2, 2.0 * delta * r_abs - delta * delta), np.where(inl, 1.0, delta / r_abs), inl


def _uv_jacobian(Xc, cam):
    """The rows of d(u, v)/dXc [-[Xc]x | I]: Ju, Jv [N, 6]."""
    fx, fy = cam[0], cam[1]
    iz = 1.0 / Xc[:, 2]
    zero = np.zeros(len(Xc))
    px = np.stack([fx * iz, zero, -fx * Xc[:, 0] * iz * iz], 1)
    py = np.stack([zero, fy * iz, -fy * Xc[:, 1] * iz * iz], 1)
    return np.concatenate([np.cross(Xc, px), px], 1), np.concatenate([np.cross(Xc, py), py], 1)


def forward_terms(R, t, X, cam, d2, delta):
    """Model -> mask, one row per point.  -> dict measurable [N], r (the bilinear distance, 0 where not measurable), rho, w, J [N, 6], and
    u, v, z for the margin checks."""
    H, W = d2.shape
    Xc, u, v, front = project(R, t, X, cam)
    with np.errstate(invalid="ignore"):
        x0f, y0f = np.floor(u), np.floor(v)
        ok = front & (x0f >= 0) & (x0f + 1 <= W - 1) & (y0f >= 0) & (y0f + 1 <= H - 1)
    x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
    if H < 2 or W < 2:
        ok = np.zeros(len(Xc), bool)
        x1, y1 = x0, y0
    else:
        x1, y1 = x0 + 1, y0 + 1
    al, be = np.where(ok, u - x0, 0.0), np.where(ok, v - y0, 0.0)
    D = np.sqrt(d2.astype(np.float64))
    D00, D10, D01, D11 = D[y0, x0], D[y0, x1], D[y1, x0], D[y1, x1]
    r = np.where(ok, (1 - be) * ((1 - al) * D00 + al * D10) + be * ((1 - al) * D01 + al * D11), 0.0)
    du = (1 - be) * (D10 - D00) + be * (D11 - D01)
    dv = (1 - al) * (D01 - D00) + al * (D11 - D10)
    Xs = np.where(ok[:, None], Xc, np.array([0.0, 0.0, 1.0]))
    Ju, Jv = _uv_jacobian(Xs, cam)
    J = du[:, None] * Ju + dv[:, None] * Jv
    J[~ok] = 0.0
    rho, w, _ = huber(np.abs(r), delta)
    rho, w = np.where(ok, rho, 0.0), np.where(ok, w, 0.0)
    return dict(measurable=ok, r=r, rho=rho, w=w, J=J, u=u, v=v, z=Xc[:, 2], front=front)


def nearest_points(u, v, front, q):
    """Per contour row the in-front point of the least squared pixel distance (ties: the lowest index) and the two smallest squared
    distances.  -> j [K] (-1: no point in front), s1 [K], s2 [K]."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    idx = np.nonzero(front)[0]
    if idx.size == 0:
        return np.full(len(q), -1, np.int64), np.full(len(q), np.inf), np.full(len(q), np.inf)
    s = (u[idx][None, :] - q[:, :1]) ** 2 + (v[idx][None, :] - q[:, 1:]) ** 2
    first = s.argmin(1)                                   # numpy's argmin returns the first of equal minima
    s1 = s[np.arange(len(q)), first]
    s_rest = s.copy()
    s_rest[np.arange(len(q)), first] = np.inf
    return idx[first], s1, s_rest.min(1) if idx.size > 1 else np.full(len(q), np.inf)


def backward_terms(R, t, X, cam, q, delta):
    """Mask contour -> model, one row per contour row.  -> dict j [K], e [K, 2], rho, w, Ju, Jv [K, 6], s1, s2; rho = inf when no point is
    in front."""
    Xc, u, v, front = project(R, t, X, cam)
    q = np.asarray(q, np.float64).reshape(-1, 2)
    j, s1, s2 = nearest_points(u, v, front, q)
    K = len(q)
    if K and j[0] < 0:
        return dict(j=j, e=np.zeros((K, 2)), rho=np.full(K, np.inf), w=np.zeros(K), Ju=np.zeros((K, 6)), Jv=np.zeros((K, 6)), s1=s1, s2=s2)
    e = np.stack([u[j] - q[:, 0], v[j] - q[:, 1]], 1)
    rs = np.sqrt((e ** 2).sum(1))
    rho, w, _ = huber(rs, delta)
    rho = np.where(rs <= delta, (e ** 2).sum(1), rho)     # an inlier's rho is s itself, not sqrt(s) squared again
    Ju, Jv = _uv_jacobian(Xc[j], cam)
    return dict(j=j, e=e, rho=rho, w=w, Ju=Ju, Jv=Jv, s1=s1, s2=s2, rs=rs)


def system(R, t, X, cam, d2, q, delta):
    """E = 1/2 sum_fwd rho / N + 1/2 sum_bwd rho / K, H [6, 6] and g [6] the same weighted sums, the measurable mask."""
    f = forward_terms(R, t, X, cam, d2, delta)
    b = backward_terms(R, t, X, cam, q, delta)
    N, K = len(X), len(np.asarray(q).reshape(-1, 2))
    Ef, Eb = float(f["rho"].sum()) / N, float(b["rho"].sum()) / K
    Jf = f["J"]
    Hf, gf = (Jf * f["w"][:, None]).T @ Jf, Jf.T @ (f["w"] * f["r"])
    wb = b["w"][:, None]
    Hb = (b["Ju"] * wb).T @ b["Ju"] + (b["Jv"] * wb).T @ b["Jv"]
    gb = b["Ju"].T @ (b["w"] * b["e"][:, 0]) + b["Jv"].T @ (b["w"] * b["e"][:, 1])
    return 0.5 * Ef + 0.5 * Eb, 0.5 * (Hf / N) + 0.5 * (Hb / K), 0.5 * (gf / N) + 0.5 * (gb / K), f["measurable"]


def normal_equations(R, t, X, cam, d2, q, delta):
    """The kernel's optional [28] output at the input pose: H upper triangle row-major (21), g (6), E."""
    E, Hm, g, _ = system(R, t, X, cam, d2, q, delta)
    return np.concatenate([Hm[np.triu_indices(6)], g, [E]])


# ---------------------------------------------------------------------------------------------------------------- the LM loop
def refine(R, t, X, cam, mask, delta, iters=30, K_max=1024, has_pose=True, d2=None, q=None, **lm):
    """The Levenberg-Marquardt loop of section 11 on the two terms.  -> dict R, t, cost_in, cost_out, num_points (measurable forward rows
    at the input pose), iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    d2 = mask_distance(mask) if d2 is None else d2
    q = contour_rows(mask, K_max) if q is None else q
    if not has_pose or len(X) == 0 or len(q) < 6:
        return out
    E, Hm, g, ok = system(R, t, X, cam, d2, q, delta)
    out.update(cost_in=E, cost_out=E, num_points=int(ok.sum()))
    if ok.sum() < 6 or not np.isfinite(E):
        return out
    out.update(lm_ref.lm_loop(lambda R, t: system(R, t, X, cam, d2, q, delta), R, t, E, Hm, g, iters, lm_solve, **lm))
    return out


# ---------------------------------------------------------------------------------------------------------------- silhouettes
def splat_mask(R, t, X, cam, H, W):
    """The rint splat of the in-front points: uint8 [H, W]."""
    _, u, v, front = project(R, t, X, cam)
    m = np.zeros((H, W), np.uint8)
    with np.errstate(invalid="ignore"):
        x, y = np.rint(u), np.rint(v)
        ok = front & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    m[y[ok].astype(np.int64), x[ok].astype(np.int64)] = 1
    return m


def splat_iou(R, t, X, cam, mask):
    """Silhouette IoU of the dense splat of the pose against the mask."""
    m = np.asarray(mask) != 0
    s = splat_mask(R, t, X, cam, *m.shape) != 0
    return float((m & s).sum()) / max(1, int((m | s).sum()))
