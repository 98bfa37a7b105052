"""numpy fp64 restatement of the featuremetric refinement contract (csrc/refine.hip computes it on the GPU).

Per detection: the template's points X [P, 3] (model mm) with features f [P, C], the query's projected map M [gh, gw, C] fp32,
a pinhole camera (fx, fy, cx, cy) of a W x H image, and the input pose (R, t).  Map coordinates follow grid_sample with
align_corners=False: x_m = u gw / W - 1/2.  The bilinear residual and its map gradient are fp32, the six C-length dot products
per point are accumulated in fp32, everything after them is fp64.
"""

import numpy as np

from tests import lm_ref
from tests.lm_ref import rot_exp, update  # noqa: F401  (the twist and the update live beside the loop; the other restatements import them from here)


def map_coords(R, t, X, cam, W, H, gw, gh):
    fx, fy, cx, cy = cam
    Xc = X.astype(np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        xm = (fx * Xc[:, 0] / z + cx) * (gw / W) - 0.5
        ym = (fy * Xc[:, 1] / z + cy) * (gh / H) - 0.5
    return Xc, z, xm, ym


def valid_set(R, t, X, cam, W, H, M):
    gh, gw = M.shape[:2]
    _, z, xm, ym = map_coords(R, t, X, cam, W, H, gw, gh)
    return (z > 1.0) & (xm >= 0) & (xm <= gw - 1) & (ym >= 0) & (ym <= gh - 1)


def point_terms(R, t, X, f, cam, W, H, M, dtype=np.float32):
    """-> dict: Xc, z, clamped flags, residual r [P, C], map gradients gx, gy [P, C] (dtype), and the rows ax, ay [P, 6] of
    d(x_m, y_m)/d xi (zero along a clamped axis).  M [gh, gw, C]."""
    gh, gw = M.shape[:2]
    Xc, z, xm, ym = map_coords(R, t, X, cam, W, H, gw, gh)
    clx = ~((xm >= 0) & (xm <= gw - 1))
    cly = ~((ym >= 0) & (ym <= gh - 1))
    xm = np.clip(xm, 0, gw - 1)
    ym = np.clip(ym, 0, gh - 1)
    x0 = np.minimum(np.floor(xm), gw - 2).astype(np.int64)
    y0 = np.minimum(np.floor(ym), gh - 2).astype(np.int64)
    al = (xm - x0).astype(dtype)[:, None]
    be = (ym - y0).astype(dtype)[:, None]
    Md = M.astype(dtype)
    m00, m10, m01, m11 = Md[y0, x0], Md[y0, x0 + 1], Md[y0 + 1, x0], Md[y0 + 1, x0 + 1]
    one = dtype(1)
    F = (one - be) * ((one - al) * m00 + al * m10) + be * ((one - al) * m01 + al * m11)
    r = F - f.astype(dtype)
    gx = (one - be) * (m10 - m00) + be * (m11 - m01)
    gy = (one - al) * (m01 - m00) + al * (m11 - m10)
    fx, fy = cam[0], cam[1]
    sx, sy = gw / W, gh / H
    iz = 1.0 / z
    px = np.stack([sx * fx * iz, np.zeros_like(z), -sx * fx * Xc[:, 0] * iz * iz], 1)
    py = np.stack([np.zeros_like(z), sy * fy * iz, -sy * fy * Xc[:, 1] * iz * iz], 1)
    ax = np.concatenate([np.cross(Xc, px), px], 1)
    ay = np.concatenate([np.cross(Xc, py), py], 1)
    ax[clx] = 0.0
    ay[cly] = 0.0
    return dict(Xc=Xc, z=z, r=r, gx=gx, gy=gy, ax=ax, ay=ay)


def jacobian(R, t, X, f, cam, W, H, M, dtype=np.float64):
    """Per-point J [P, C, 6] = gx ax^T + gy ay^T and residuals r [P, C] (dtype arithmetic for the map part)."""
    p = point_terms(R, t, X, f, cam, W, H, M, dtype)
    J = p["gx"].astype(np.float64)[:, :, None] * p["ax"][:, None, :] + p["gy"].astype(np.float64)[:, :, None] * p["ay"][:, None, :]
    return J, p["r"].astype(np.float64)


def system(R, t, X, f, cam, W, H, M, valid, sigma2):
    """Cost E, H [6, 6], g [6] over the valid points at (R, t), and whether a valid point has z <= 1 mm."""
    Xv, fv = X[valid], f[valid]
    p = point_terms(R, t, Xv, fv, cam, W, H, M)
    zbad = bool((~(p["z"] > 1.0)).any())
    d = lambda a, b: np.sum(a * b, axis=1, dtype=np.float32).astype(np.float64)
    gxx, gxy, gyy = d(p["gx"], p["gx"]), d(p["gx"], p["gy"]), d(p["gy"], p["gy"])
    gxr, gyr, rr = d(p["gx"], p["r"]), d(p["gy"], p["r"]), d(p["r"], p["r"])
    q = rr / sigma2
    w = 1.0 / (1.0 + q)
    ax, ay = p["ax"], p["ay"]
    Hm = np.einsum("p,pi,pj->ij", w * gxx, ax, ax) + np.einsum("p,pi,pj->ij", w * gxy, ax, ay) \
        + np.einsum("p,pi,pj->ij", w * gxy, ay, ax) + np.einsum("p,pi,pj->ij", w * gyy, ay, ay)
    g = (w * gxr) @ ax + (w * gyr) @ ay
    E = float(np.sum(sigma2 * np.log1p(q)))
    return E, Hm, g, zbad


def sigma2_at(R, t, X, f, cam, W, H, M, valid):
    p = point_terms(R, t, X[valid], f[valid], cam, W, H, M)
    s = np.sum(p["r"] * p["r"], axis=1, dtype=np.float32).astype(np.float64)
    return max(float(s.sum()) / max(int(valid.sum()), 1), 1e-12)


def normal_equations(R, t, X, f, cam, W, H, M):
    """The kernel's optional [28] output at the input pose: H upper triangle row-major (21), g (6), E."""
    valid = valid_set(R, t, X, cam, W, H, M)
    s2 = sigma2_at(R, t, X, f, cam, W, H, M, valid)
    E, Hm, g, _ = system(R, t, X, f, cam, W, H, M, valid, s2)
    iu = np.triu_indices(6)
    return np.concatenate([Hm[iu], g, [E]])


def lm_solve(Hm, g, lam):
    A = Hm + lam * np.diag(np.diag(Hm))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(L)):
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, -g))


def refine(R, t, X, f, cam, W, H, M, iters=30, has_pose=True, **lm):
    """The Levenberg-Marquardt loop.  -> dict R, t, cost_in, cost_out, num_points, iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(X) == 0:
        return out
    valid = valid_set(R, t, X, cam, W, H, M)
    out["num_points"] = int(valid.sum())
    if valid.sum() < 6:
        return out
    s2 = sigma2_at(R, t, X, f, cam, W, H, M, valid)
    E, Hm, g, _ = system(R, t, X, f, cam, W, H, M, valid, s2)
    out["cost_in"] = E
    out.update(lm_ref.lm_loop(lambda R, t: system(R, t, X, f, cam, W, H, M, valid, s2), R, t, E, Hm, g, iters, lm_solve, admissible=lambda zbad: not zbad,
                              z_gap=lambda R, t: 1.0 - float(point_terms(R, t, X[valid], f[valid], cam, W, H, M)["z"].min()), **lm))
    return out


def smooth_field(gh, gw, C, seed, wavelengths=(6.0, 15.0), terms=4):
    """A smooth random map [gh, gw, C] fp32: per channel a sum of sinusoids with wavelengths in the given range (cells)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    M = np.zeros((gh, gw, C), np.float64)
    for c in range(C):
        for _ in range(terms):
            lam = rng.uniform(*wavelengths)
            th = rng.uniform(0, 2 * np.pi)
            ph = rng.uniform(0, 2 * np.pi)
            M[:, :, c] += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi / lam * (np.cos(th) * xx + np.sin(th) * yy) + ph)
    return M.astype(np.float32)


def sample_at(M, R, t, X, cam, W, H):
    """Bilinear fp32 features of M at the projections of X (clamped) -- what planted f_i are made of."""
    p = point_terms(R, t, X, np.zeros((len(X), M.shape[2]), np.float32), cam, W, H, M)
    return p["r"].astype(np.float32)


def rot_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra).T @ np.asarray(Rb)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
