"""numpy fp64 restatement of multi-view pose consensus (TEST HELPER): the per-row term of csrc/multiview.hip with its
Levenberg-Marquardt loop (tests/lm_ref.lm_loop), and the whole of foundpose_amd/multiview.py -- the lift of a camera-frame estimate into
the world, a brute-force symmetric distance, the greedy clustering, the targets, the write-back -- as `fuse`, end to end.

rows are eval_bop19.load_results_csv's dicts; scene_cameras {scene_id: {str(im_id): {"cam_K", "cam_R_w2c", "cam_t_w2c"}}} (a scene's
scene_camera.json); models {obj_id: anything with .pts [V, 3], .syms [{"R", "t"}], .diameter}."""

import numpy as np

from tests import lm_ref
from tests.depth_refine_ref import lm_solve

DEFAULTS = dict(match_thresh=1.0, huber_px=10.0, points=64, min_views=2, iters=20)


# ---------------------------------------------------------------------------------------------------------- the term
def row_terms(R, t, Y, uv, view, view_cam, view_T, delta):
    """Rows (Y [N, 3] model points, uv [N, 2] targets, view [N]) under the world pose (R, t).  -> dict: Xw, Xc, z, measurable, e [N, 2],
    rs = |e|, inlier, w, rho, Jx, Jy [N, 6] (the Jacobian rows of e_u and e_v; 0 where not measurable)."""
    Y, uv, view = np.asarray(Y, np.float64), np.asarray(uv, np.float64), np.asarray(view, np.int64)
    cam = np.asarray(view_cam, np.float64)[view]
    Rv, tv = np.asarray(view_T, np.float64)[view, :9].reshape(-1, 3, 3), np.asarray(view_T, np.float64)[view, 9:]
    Xw = Y @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    Xc = np.einsum("nij,nj->ni", Rv, Xw) + tv
    z = Xc[:, 2]
    ok = z > 1.0
    zs = np.where(ok, z, 1.0)
    e = np.stack([cam[:, 0] * Xc[:, 0] / zs + cam[:, 2], cam[:, 1] * Xc[:, 1] / zs + cam[:, 3]], 1) - uv
    e[~ok] = 0.0
    s = (e * e).sum(1)
    rs = np.sqrt(s)
    inl = ok & (rs <= delta)
    w = np.where(inl, 1.0, delta / np.where(rs > 0, rs, 1.0))
    w[~ok] = 0.0
    rho = np.where(ok, np.where(inl, s, 2.0 * delta * rs - delta * delta), delta * delta)
    zero = np.zeros_like(zs)
    px = np.stack([cam[:, 0] / zs, zero, -cam[:, 0] * Xc[:, 0] / (zs * zs)], 1)
    py = np.stack([zero, cam[:, 1] / zs, -cam[:, 1] * Xc[:, 1] / (zs * zs)], 1)
    qx, qy = np.einsum("nji,nj->ni", Rv, px), np.einsum("nji,nj->ni", Rv, py)     # R_v^T p
    Jx, Jy = np.concatenate([np.cross(Xw, qx), qx], 1), np.concatenate([np.cross(Xw, qy), qy], 1)
    Jx[~ok] = 0.0
    Jy[~ok] = 0.0
    return dict(Xw=Xw, Xc=Xc, z=z, measurable=ok, e=e, rs=rs, inlier=inl, w=w, rho=rho, Jx=Jx, Jy=Jy)


def system(R, t, Y, uv, view, view_cam, view_T, delta):
    """cost = sum rho / N, H [6, 6], g [6], the inlier mask."""
    p = row_terms(R, t, Y, uv, view, view_cam, view_T, delta)
    w, Jx, Jy, e = p["w"], p["Jx"], p["Jy"], p["e"]
    H = (Jx * w[:, None]).T @ Jx + (Jy * w[:, None]).T @ Jy
    g = Jx.T @ (w * e[:, 0]) + Jy.T @ (w * e[:, 1])
    return float(p["rho"].sum()) / len(Y), H, g, p["inlier"]


def normal_equations(R, t, Y, uv, view, view_cam, view_T, delta):
    """The kernel's optional [28] output at the input pose: H upper triangle row-major (21), g (6), cost."""
    E, H, g, _ = system(R, t, Y, uv, view, view_cam, view_T, delta)
    return np.concatenate([H[np.triu_indices(6)], g, [E]])


def branch_gap(R, t, Y, uv, view, view_cam, view_T, delta):
    """How far the nearest per-row branch (z > 1, |e| <= delta) is from flipping at a pose, relative."""
    p = row_terms(R, t, Y, uv, view, view_cam, view_T, delta)
    m = p["measurable"]
    gaps = [np.abs(p["z"] - 1.0), np.abs(p["rs"][m] - delta) / delta]
    return min([float(g.min()) for g in gaps if g.size] or [np.inf])


def refine(R, t, Y, uv, view, view_cam, view_T, delta, iters=20, has_pose=True, **lm):
    """-> dict R, t, cost_in, cost_out, num_points (inliers at the input pose), iters_used, status, trace (tests/lm_ref.lm_loop)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(Y) == 0:
        return out
    args = (Y, uv, view, view_cam, view_T, delta)
    E, H, g, inl = system(R, t, *args)
    out.update(cost_in=E, cost_out=E, num_points=int(inl.sum()))
    if inl.sum() < 6:
        return out
    out.update(lm_ref.lm_loop(lambda R, t: system(R, t, *args), R, t, E, H, g, iters, lm_solve, **lm))
    return out


# ---------------------------------------------------------------------------------------------------------- poses
def mat(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return T


def camera_entry(scene_cameras, sid, iid):
    sc = scene_cameras.get(sid, scene_cameras.get(str(sid))) if scene_cameras else None
    if sc is None:
        return None
    return sc.get(str(iid), sc.get(iid))


def w2c(entry):
    return mat(np.asarray(entry["cam_R_w2c"], np.float64).reshape(3, 3), np.asarray(entry["cam_t_w2c"], np.float64).reshape(3))


def lift(row, entry):
    """W = T_w2c^-1 T_m2c."""
    return np.linalg.inv(w2c(entry)) @ mat(row["R"], row["t"])


def sample(pts, points):
    """bank.sample_verify_points' rule: rows 0, s, 2 s, ... with s = ceil(V / points), as the fp32 values the device holds."""
    P = np.asarray(pts)
    return P[::max(1, -(-len(P) // points))].astype(np.float32).astype(np.float64)


def sym_distance(Wi, Wj, syms, X):
    """min over S of max over x of |Wi x - Wj S x| -> (d, the first S that attains it)."""
    a = X @ Wi[:3, :3].T + Wi[:3, 3]
    best, arg = np.inf, -1
    for k, s in enumerate(syms):
        WS = Wj @ mat(s["R"], s["t"])
        d = float(np.linalg.norm(a - (X @ WS[:3, :3].T + WS[:3, 3]), axis=1).max())
        if d < best:
            best, arg = d, k
    return best, arg


def greedy_clusters(cands, W, image, score, syms, X, bar):
    """cands: input rows of one (scene, object).  -> clusters [{"seed", "members": [(row, sym index or -1 for the seed, d)]}] in the
    order they were seeded."""
    clusters = []
    for i in sorted(cands, key=lambda i: (-score[i], i)):
        best = None
        for c in clusters:
            if any(image[m] == image[i] for m, _, _ in c["members"]):
                continue
            d, k = sym_distance(W[i], W[c["seed"]], syms, X)
            if d <= bar and (best is None or d < best[1]):
                best = (c, d, k)
        if best is None:
            clusters.append({"seed": i, "members": [(i, -1, 0.0)]})
        else:
            best[0]["members"].append((i, best[2], best[1]))
    return clusters


def rotation_deg(Ra, Rb):
    c = 0.5 * (np.trace(np.asarray(Ra) @ np.asarray(Rb).T) - 1.0)
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def fuse(rows, scene_cameras, models, match_thresh=1.0, huber_px=10.0, points=64, min_views=2, iters=20):
    """-> (rows', report): report["rows"][i] = dict(cluster, seed, views, sym, d, fused, reason), report["clusters"][c] = dict(seed,
    members, status, cost_in, cost_out, iters_used, num_points, dropped, R, t), report["unfused_scenes"] = {scene_id: reason}."""
    out = [dict(r) for r in rows]
    rep_rows = [dict(cluster=None, seed=None, views=0, sym=None, d=None, fused=False, reason=None) for _ in rows]
    unfused, clusters_out = {}, []
    scenes = {}
    for i, r in enumerate(rows):
        scenes.setdefault(r["scene_id"], []).append(i)
    for sid, members in scenes.items():
        for i in members:
            e = camera_entry(scene_cameras, sid, rows[i]["im_id"])
            if e is None or "cam_R_w2c" not in e or "cam_t_w2c" not in e or "cam_K" not in e:
                unfused[sid] = f"image {rows[i]['im_id']} has no cam_K / cam_R_w2c / cam_t_w2c"
                break
        if sid in unfused:
            for i in members:
                rep_rows[i]["reason"] = "scene not fused: " + unfused[sid]
            continue
        W = {i: lift(rows[i], camera_entry(scene_cameras, sid, rows[i]["im_id"])) for i in members}
        image = {i: rows[i]["im_id"] for i in members}
        score = {i: rows[i]["score"] for i in members}
        objs = {}
        for i in members:
            objs.setdefault(rows[i]["obj_id"], []).append(i)
        for oid, cands in objs.items():
            model = models[oid]
            X = sample(model.pts, points)
            for c in greedy_clusters(cands, W, image, score, model.syms, X, match_thresh * model.diameter):
                cid = len(clusters_out)
                rec = dict(scene_id=sid, obj_id=oid, seed=c["seed"], members=[m for m, _, _ in c["members"]], status=None, cost_in=None,
                           cost_out=None, iters_used=None, num_points=None, dropped=0, R=None, t=None)
                clusters_out.append(rec)
                for m, k, d in c["members"]:
                    rep_rows[m].update(cluster=cid, seed=c["seed"], views=len(c["members"]), sym=k, d=d)
                if len(c["members"]) < min_views:
                    for m, _, _ in c["members"]:
                        rep_rows[m]["reason"] = "singleton" if len(c["members"]) == 1 else f"fewer than {min_views} views"
                    continue
                Y, uv, view, cams, Ts = [], [], [], [], []
                for v, (m, k, _) in enumerate(c["members"]):
                    e = camera_entry(scene_cameras, sid, image[m])
                    K = np.asarray(e["cam_K"], np.float64).reshape(3, 3)
                    T = w2c(e)
                    cams.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
                    Ts.append(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]))
                    S = np.eye(4) if k < 0 else mat(model.syms[k]["R"], model.syms[k]["t"])
                    M = mat(rows[m]["R"], rows[m]["t"]) @ np.linalg.inv(S)
                    Xc = X @ M[:3, :3].T + M[:3, 3]
                    keep = Xc[:, 2] > 1.0
                    rec["dropped"] += int((~keep).sum())
                    Y.append(X[keep])
                    uv.append(np.stack([cams[-1][0] * Xc[keep, 0] / Xc[keep, 2] + cams[-1][2], cams[-1][1] * Xc[keep, 1] / Xc[keep, 2] + cams[-1][3]], 1))
                    view.append(np.full(int(keep.sum()), v))
                res = refine(W[c["seed"]][:3, :3], W[c["seed"]][:3, 3], np.concatenate(Y), np.concatenate(uv), np.concatenate(view), np.array(cams),
                             np.array(Ts), huber_px, iters)
                rec.update(status=res["status"], cost_in=res["cost_in"], cost_out=res["cost_out"], iters_used=res["iters_used"],
                           num_points=res["num_points"], R=res["R"], t=res["t"])
                if res["status"] == 2:
                    for m, _, _ in c["members"]:
                        rep_rows[m]["reason"] = "fewer than 6 inliers at the seed's pose"
                    continue
                Wo = mat(res["R"], res["t"])
                for v, (m, k, _) in enumerate(c["members"]):
                    S = np.eye(4) if k < 0 else mat(model.syms[k]["R"], model.syms[k]["t"])
                    Tn = w2c(camera_entry(scene_cameras, sid, image[m])) @ Wo @ S
                    out[m]["R"], out[m]["t"] = Tn[:3, :3].copy(), Tn[:3, 3].copy()
                    rep_rows[m]["fused"] = True
    return out, dict(rows=rep_rows, clusters=clusters_out, unfused_scenes=unfused)


# ---------------------------------------------------------------------------------------------------------- planted scenes
def ring_cameras(n=6, radius=800.0, elevation=0.5, K=(600.0, 600.0, 160.0, 120.0), im0=0):
    """n cameras on a ring around the origin, looking at it.  -> {str(im_id): scene_camera.json entry}."""
    out = {}
    for k in range(n):
        az = 2.0 * np.pi * k / n
        c = radius * np.array([np.cos(elevation) * np.cos(az), np.cos(elevation) * np.sin(az), np.sin(elevation)])
        zc = -c / np.linalg.norm(c)
        xc = np.cross(zc, [0.0, 0.0, 1.0])
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])        # world -> camera
        out[str(im0 + k)] = {"cam_K": [K[0], 0.0, K[2], 0.0, K[1], K[3], 0.0, 0.0, 1.0], "cam_R_w2c": R.reshape(9).tolist(),
                             "cam_t_w2c": (-R @ c).tolist(), "depth_scale": 1.0}
    return out


def ray_noise(rng, T_m2c, frac=(0.02, 0.05), trans_mm=1.0, rot_deg=0.5):
    """An RGB-like error: the translation pushed 2 .. 5 % of its distance along its own ray with a random sign, plus a little noise."""
    T = T_m2c.copy()
    t = T[:3, 3]
    T[:3, 3] = t + rng.choice([-1.0, 1.0]) * rng.uniform(*frac) * t + rng.normal(size=3) * trans_mm
    ax = rng.normal(size=3)
    T[:3, :3] = lm_ref.rot_exp(ax / np.linalg.norm(ax) * np.radians(rot_deg) * rng.normal()) @ T[:3, :3]
    return T


def view_rows(cams, W_by_image, scene_id=1, obj_id=1, scores=None, estimates=None):
    """One csv row per image of `cams`: the object at world pose W_by_image[im] (or `estimates[im]`, a model -> camera matrix)."""
    rows = []
    for n, (im, e) in enumerate(cams.items()):
        T = estimates[im] if estimates is not None else w2c(e) @ W_by_image[im]
        rows.append({"scene_id": scene_id, "im_id": int(im), "obj_id": obj_id, "score": 0.9 - 0.01 * n if scores is None else scores[n],
                     "R": T[:3, :3].copy(), "t": T[:3, 3].copy(), "time": 0.5})
    return rows


def cloud_model(rng, n=64, sigma=30.0, syms=None):
    """n model points drawn from N(0, sigma^2) as an eval_util.EvalModel (the identity as its only symmetry unless given)."""
    from foundpose_amd.eval_util import EvalModel
    pts = rng.normal(size=(n, 3)) * sigma
    diameter = float(np.linalg.norm(pts[:, None] - pts[None], axis=2).max())
    return EvalModel(pts, syms or [{"R": np.eye(3), "t": np.zeros((3, 1))}], diameter)


def fourfold_model(rng, n=16, sigma=30.0):
    """A point set with a four-fold symmetry about z: n points and their turns by 90, 180 and 270 degrees; the four rotations as syms."""
    from foundpose_amd.eval_util import EvalModel
    base = rng.normal(size=(n, 3)) * sigma
    turns = [lm_ref.rot_exp(np.array([0.0, 0.0, k * np.pi / 2.0])) for k in range(4)]
    turns = [np.rint(T) for T in turns]                       # exact quarter turns
    pts = np.concatenate([base @ T.T for T in turns])
    diameter = float(np.linalg.norm(pts[:, None] - pts[None], axis=2).max())
    return EvalModel(pts, [{"R": T, "t": np.zeros((3, 1))} for T in turns], diameter)


def random_pose(rng, spread=20.0):
    return mat(lm_ref.rot_exp(rng.normal(size=3)), rng.normal(size=3) * spread)


def scene_ring(seed):
    """The planted ring: 6 cameras, one object, every view's estimate off along its own ray.  -> (rows, scene_cameras, models, W_true)."""
    rng = np.random.default_rng(seed)
    cams = ring_cameras()
    model = cloud_model(rng)
    Wt = random_pose(rng)
    est = {im: ray_noise(rng, w2c(e) @ Wt) for im, e in cams.items()}
    return view_rows(cams, None, estimates=est), {1: cams}, {1: model}, Wt


def scene_outlier(seed=11, view="2"):
    """scene_ring with the estimate of one view turned by 90 degrees about the object's own x axis."""
    rows, sc, models, Wt = scene_ring(seed)
    for r in rows:
        if str(r["im_id"]) == view:
            r["R"] = r["R"] @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    return rows, sc, models, Wt


def scene_two_instances(seed=12):
    """Two instances of one object three diameters apart, both seen in every view."""
    rng = np.random.default_rng(seed)
    cams = ring_cameras(radius=1200.0)
    model = cloud_model(rng)
    Wa = random_pose(rng)
    Wb = random_pose(rng)
    Wa[:3, 3] += np.array([1.5, 0.0, 0.0]) * model.diameter
    Wb[:3, 3] -= np.array([1.5, 0.0, 0.0]) * model.diameter
    rows = []
    for n, W in enumerate((Wa, Wb)):
        est = {im: ray_noise(rng, w2c(e) @ W) for im, e in cams.items()}
        rows += view_rows(cams, None, estimates=est, scores=[0.9 - 0.01 * k - 0.005 * n for k in range(len(cams))])
    rows.sort(key=lambda r: r["im_id"])
    return rows, {1: cams}, {1: model}, (Wa, Wb)


def scene_fourfold(seed=13):
    """A four-fold symmetric object whose views' estimates are turned by random multiples of 90 degrees about the symmetry axis."""
    rng = np.random.default_rng(seed)
    cams = ring_cameras()
    model = fourfold_model(rng)
    Wt = random_pose(rng)
    est = {}
    for im, e in cams.items():
        S = mat(model.syms[int(rng.integers(4))]["R"], np.zeros(3))
        est[im] = ray_noise(rng, w2c(e) @ Wt @ S)
    return view_rows(cams, None, estimates=est), {1: cams}, {1: model}, Wt


def scene_missing_pose(seed=14):
    """Two scenes: scene 1 complete, scene 2 the same ring with one image lacking cam_R_w2c."""
    rows, sc, models, Wt = scene_ring(seed)
    rows2 = [dict(r, scene_id=2, R=r["R"].copy(), t=r["t"].copy()) for r in rows]
    cams2 = {im: dict(e) for im, e in sc[1].items()}
    del cams2["3"]["cam_R_w2c"]
    return rows + rows2, {1: sc[1], 2: cams2}, models, Wt


SCENES = {"ring0": lambda: scene_ring(0), "outlier": scene_outlier, "two_instances": scene_two_instances, "fourfold": scene_fourfold,
          "missing_pose": scene_missing_pose}
SCENE_OPTS = {"outlier": dict(match_thresh=0.5)}     # see tests/test_multiview_cpu.py: a quarter turn about the centroid stays within one diameter


# ---------------------------------------------------------------------------------------------------------- the kernel's problems
NROWS = 70              # tests/lm_steps.NPTS: three chunks of FP_REFINE_CHUNK = 32, the last one ragged
DELTA = 10.0


def view_tables():
    """Five ring views and a sixth whose camera stands 60 mm from the world's origin: -> (view_cam [6, 4], view_T [6, 12])."""
    cams = ring_cameras(5)
    near = ring_cameras(1, radius=60.0, elevation=0.2)["0"]
    cam, T = [], []
    for e in list(cams.values()) + [near]:
        K = np.asarray(e["cam_K"]).reshape(3, 3)
        M = w2c(e)
        cam.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        T.append(np.concatenate([M[:3, :3].reshape(9), M[:3, 3]]))
    return np.array(cam), np.array(T)


def kernel_problem(seed, views, behind=False, rot_deg=3.0, trans_mm=10.0, outliers=4, noise_px=1.5):
    """NROWS rows from the given views (NROWS / len(views) model points each): targets are the projections under each view's own
    ray-noised estimate plus pixel noise -- the minimum's cost is not a handful of rounding errors --, `outliers` of them 25 .. 60 px
    further off (rows on both sides of delta); the start is a view's estimate lifted and pushed off.  behind: one model point lies
    behind the last view's camera.  -> dict Y fp32 [NROWS, 3], uv, view, R, t (the start)."""
    rng = np.random.default_rng(seed)
    cam, T = view_tables()
    P = NROWS // len(views)
    Wt = mat(lm_ref.rot_exp(rng.normal(size=3)), rng.normal(size=3) * 5.0)
    X = (rng.normal(size=(P, 3)) * 30.0)
    if behind:      # a world point 100 mm out along the near camera's direction, beyond the camera at 60 mm
        Tn = mat(T[views[-1], :9].reshape(3, 3), T[views[-1], 9:])
        c = np.linalg.inv(Tn)[:3, 3]
        X[3] = np.linalg.inv(Wt)[:3, :3] @ (c / np.linalg.norm(c) * 100.0) + np.linalg.inv(Wt)[:3, 3]
    X = X.astype(np.float32)
    Y, uv, vi = [], [], []
    for v in views:
        Tv = mat(T[v, :9].reshape(3, 3), T[v, 9:])
        est = ray_noise(rng, Tv @ Wt)
        Xc = X.astype(np.float64) @ est[:3, :3].T + est[:3, 3]
        ok = Xc[:, 2] > 1.0
        z = np.where(ok, Xc[:, 2], 1.0)
        p = np.stack([cam[v, 0] * Xc[:, 0] / z + cam[v, 2], cam[v, 1] * Xc[:, 1] / z + cam[v, 3]], 1)
        p[~ok] = (cam[v, 2], cam[v, 3])
        Y.append(X)
        uv.append(p + rng.normal(size=p.shape) * noise_px)
        vi.append(np.full(P, v))
    Y, uv, vi = np.concatenate(Y), np.concatenate(uv), np.concatenate(vi)
    for r in rng.choice(len(Y), outliers, replace=False):
        a = rng.uniform(0, 2 * np.pi)
        uv[r] += rng.uniform(25.0, 60.0) * np.array([np.cos(a), np.sin(a)])
    ax, dt = rng.normal(size=3), rng.normal(size=3)
    R0 = lm_ref.rot_exp(ax / np.linalg.norm(ax) * np.radians(rot_deg)) @ Wt[:3, :3]
    t0 = Wt[:3, 3] + dt * trans_mm / np.linalg.norm(dt)
    return dict(Y=Y, uv=uv, view=vi.astype(np.int32), R=R0, t=t0)


class KernelFixture:
    """What tests/lm_steps.pinned_prefix asks of a fixture, for one kernel_problem (entry "depth": its MARGIN and bars)."""
    entry = "depth"

    def __init__(self, name, det, K):
        self.name, self.det, self.K = name, det, K
        self.tables = view_tables()

    def __repr__(self):
        return f"multiview:{self.name}"

    def args(self, reverse=False):
        o = slice(None, None, -1) if reverse else slice(None)
        d = self.det
        return (d["Y"].astype(np.float64)[o], d["uv"][o], d["view"][o], *self.tables, DELTA)

    def run(self, iters, reverse=False, **lm):
        return refine(self.det["R"], self.det["t"], *self.args(reverse), iters, self.det.get("has_pose", True), **lm)

    def gaps(self, R, t):
        return branch_gap(R, t, *self.args())


# name -> (seed, views, keywords, K): K iterations lie inside the pinned prefix (tests/test_multiview_cpu.py recomputes it)
KERNEL_SPECS = {
    "one_view": (1, (2,), {}, 3),
    "two_views": (2, (0, 3), {}, 2),
    "five_views": (3, (0, 1, 2, 3, 4), {}, 3),
    "behind": (4, (1, 5), dict(behind=True), 24),
}
_FIXTURES = {}


def kernel_fixture(name):
    if name not in _FIXTURES:
        seed, views, kw, K = KERNEL_SPECS[name]
        _FIXTURES[name] = KernelFixture(name, kernel_problem(seed, views, **kw), K)
    return _FIXTURES[name]
