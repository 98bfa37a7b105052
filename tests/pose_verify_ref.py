"""numpy fp64 restatement of fp_pose_verify_depth's contract (include/foundpose_amd.h): the frame pose, the cell
grid of the projected bounding sphere, the z-buffer of the point sample (rounded to fp32 per cell) and the classification of every visible
point against the depth image.  Every step is one rounded fp64 operation in the stated order, so a correct implementation makes every
decision identically and its integer outputs are EQUAL.

Besides the results it returns `min_margin`: the smallest relative distance of any compared quantity from its decision boundary -- u, v
from half-integers (the image border is one), the cell coordinate from the cell edges, z from 1, z from zbuf + tau, |r| from tau, a
measured D from 0 (D == 0 exactly is the "no measurement" marker, an input and not a rounded quantity), C.z from rho + 1 and n_vis from
min_visible.  A fixture whose min_margin is far above fp64 rounding noise has the same counts in any correct fp64 implementation,
whatever its FMA use.
"""

import numpy as np

from tests import kabsch_ref
from tests.kabsch_ref import camera_tuple, rot_xyz  # noqa: F401  (shared helpers of the depth stages' restatements)


class Margin(kabsch_ref.Margin):
    """kabsch_ref's running minimum, with a NaN margin counted as 0: a NaN among the compared quantities must fail `min_margin > bound`
    (a plain `NaN < value` would skip it)."""

    def add(self, rel):
        rel = np.asarray(rel, np.float64)
        super().add(np.where(np.isnan(rel), 0.0, rel))


def _mat3(M, x):
    """M x + nothing: products summed k ascending, per row; x [..., 3] -> [..., 3]."""
    return np.stack([(M[i, 0] * x[..., 0] + M[i, 1] * x[..., 1]) + M[i, 2] * x[..., 2] for i in range(3)], -1)


def verify_pair(R, t, A, cam, depth, tau, X, c, rho, G, min_visible=16, margin=None, zbuffer=True):
    """One pair with a pose.  R / t: model -> solve camera; A: solve -> frame; cam: the frame camera's (fx, fy, cx, cy); depth [H, W]
    float32; X [M, 3] float32 (the object's sample, M >= 1); c [3], rho: its sphere.  -> (counts [6], score, status).  zbuffer=False counts
    every point with z > 1 as visible (what the z-buffer removes is then the difference)."""
    margin = Margin() if margin is None else margin
    fx, fy, cx, cy = (np.float64(v) for v in cam)
    R, t, A, c = (np.asarray(v, np.float64) for v in (R, t, A, c))
    rho, tau = np.float64(rho), np.float64(tau)
    H, W = depth.shape
    Rf = np.stack([_mat3(A, R[:, j]) for j in range(3)], -1)   # Rf[i, j] = sum_k A[i, k] R[k, j]
    tf = _mat3(A, t)
    C = _mat3(Rf, c) + tf
    zero = np.zeros(6, np.int64)
    with np.errstate(all="ignore"):
        margin.add(abs(C[2] - (rho + 1.0)) / max(1.0, abs(rho + 1.0)))
        if not C[2] > rho + 1.0:
            return zero, 0.0, 2
        uc, vc = fx * C[0] / C[2] + cx, fy * C[1] / C[2] + cy
        rpx = max(fx, fy) * rho / (C[2] - rho)
        u0, v0, h = uc - rpx, vc - rpx, 2.0 * rpx / np.float64(G)
        Xc = _mat3(Rf, np.asarray(X, np.float32).astype(np.float64)) + tf
        z = Xc[:, 2]
        margin.add(np.abs(z - 1.0) / np.maximum(1.0, np.abs(z)))
        front = z > 1.0
        Xc, z = Xc[front], z[front]
        u, v = fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy
        qx, qy = (u - u0) / h, (v - v0) / h
        for q in (qx, qy):   # the edges between cells are the integers 1 .. G - 1; beyond them the clamp decides, whatever the rounding
            margin.add(np.abs(q - np.clip(np.rint(q), 1.0, G - 1.0)) / np.maximum(1.0, np.abs(q)))
        ix = np.fmin(np.fmax(np.floor(qx), 0.0), G - 1.0).astype(np.int64)
        iy = np.fmin(np.fmax(np.floor(qy), 0.0), G - 1.0).astype(np.int64)
        cell = iy * G + ix
        zbuf = np.full(G * G, np.inf, np.float32)
        np.minimum.at(zbuf, cell, z.astype(np.float32))   # round to nearest
        if zbuffer:
            lim = zbuf[cell].astype(np.float64) + tau
            margin.add(np.abs(z - lim) / tau)
            vis = z <= lim
        else:
            vis = np.ones(z.shape, bool)
        u, v, z = u[vis], v[vis], z[vis]
        for w in (u, v):
            margin.add(np.abs(w - (np.floor(w) + 0.5)) / np.maximum(1.0, np.abs(w)))
        px, py = np.rint(u), np.rint(v)   # half to even
        inside = (px >= 0.0) & (px <= W - 1.0) & (py >= 0.0) & (py <= H - 1.0)
        D = depth[py[inside].astype(np.int64), px[inside].astype(np.int64)]
        margin.add(np.abs(D[D != 0].astype(np.float64)))
        meas = D > 0
        r = D[meas].astype(np.float64) - z[inside][meas]
        margin.add(np.abs(np.abs(r) - tau) / tau)
        n_vis = int(vis.sum())
        n_in = int((np.abs(r) <= tau).sum())
        n_occ = int((~(np.abs(r) <= tau) & (r < 0.0)).sum())
        n_free = int(meas.sum()) - n_in - n_occ
        counts = np.array([n_vis, n_in, n_occ, n_free, int((~meas).sum()), int((~inside).sum())], np.int64)
        margin.add(abs(n_vis - (min_visible - 0.5)) / min_visible)
        if n_vis < min_visible:
            return counts, 0.0, 1
        return counts, float(np.float64(n_in) / np.float64(n_vis)), 0


def pose_verify_ref(success, R, t, cams, A, image_index, tau, ranges, centers, radii, points, depth, n_slots, G, min_visible=16, zbuffer=True):
    """success [P], R [P, 3, 3], t [P, 3]; per detection (P / n_slots): cams [., 4], A [., 3, 3], image_index [.], tau [.], ranges [., 2],
    centers [., 3], radii [.]; points [M_total, 3] float32; depth [N, H, W] float32.
    -> dict: counts [P, 6], score [P], status [P], min_margin."""
    P = len(success)
    M_total, N = len(points), len(depth)
    out = {"counts": np.zeros((P, 6), np.int64), "score": np.zeros(P), "status": np.zeros(P, np.int64)}
    margin = Margin()
    for pair in range(P):
        det = pair // n_slots
        image, th = int(image_index[det]), float(tau[det])
        if not 0 <= image < N or not (th > 0 and np.isfinite(th)):
            out["status"][pair] = -1
            continue
        b, e = (int(min(max(int(v), 0), M_total)) for v in ranges[det])
        if not success[pair] or b >= e:
            out["status"][pair] = 2
            continue
        out["counts"][pair], out["score"][pair], out["status"][pair] = verify_pair(
            R[pair], t[pair], A[det], cams[det], depth[image], th, points[b:e], centers[det], radii[det], G, min_visible, margin, zbuffer)
    out["min_margin"] = margin.value
    return out


# ---------------------------------------------------------------------------------------------------- planted scenes for the tests
def blob_radius(dirs, bump_dir, radius=40.0, bump=0.45, width=0.5):
    """Radius of the blob's surface along unit directions: a sphere with one smooth bump (no symmetry about any axis but the bump's own)."""
    ang = np.arccos(np.clip(dirs @ bump_dir, -1.0, 1.0))
    return radius * (1.0 + bump * np.exp(-(ang / width) ** 2))


def sphere_dirs(n, rng=None):
    """n unit directions: a Fibonacci lattice, jittered when rng is given."""
    i = np.arange(n) + 0.5
    zz = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([np.sqrt(1.0 - zz * zz) * np.cos(phi), np.sqrt(1.0 - zz * zz) * np.sin(phi), zz], 1)
    if rng is not None:
        d = d + rng.normal(0.0, 0.02, d.shape)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d


def splat(depth, cam, R, t, bump_dir, n=150000):
    """The blob's dense surface at the frame pose (R, t) z-buffered into `depth` (nearest pixel, the nearest surface wins)."""
    fx, fy, cx, cy = cam
    d = sphere_dirs(n)
    Xc = (d * blob_radius(d, bump_dir)[:, None]) @ R.T + t
    px = np.rint(fx * Xc[:, 0] / Xc[:, 2] + cx).astype(np.int64)
    py = np.rint(fy * Xc[:, 1] / Xc[:, 2] + cy).astype(np.int64)
    H, W = depth.shape
    ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    np.minimum.at(depth, (py[ok], px[ok]), Xc[ok, 2].astype(np.float32))


def along_ray(t, mm):
    """t moved by mm along the ray from the camera centre through it."""
    t = np.asarray(t, np.float64)
    return t + t / np.linalg.norm(t) * mm


def gpu_fixture(seed=6):
    """The tests' batch: 2 detections of 2 different objects x 3 slots, G = 16, two 48 x 64 depth images splatted from the planted poses
    over a background at 1000 mm and quantised to 0.1 mm.  Object 0 has 600 vertices, object 1 has 1203 of which every second is sampled
    (max_points = 700).  Detection 0 (object 0, A = I): the planted pose, the pose pushed 3 tau along the ray, the pose turned 180 degrees
    about the view axis through the blob; a 40 mm occluder strip lies over part of the blob.  Detection 1 (object 1, a crop camera: a
    rotated A): a slot with success false, the planted pose -- partly outside the image, a rectangle of holes over part of it -- and a pose
    whose sphere reaches the camera (C.z <= rho + 1).  -> dict (see the code).  Seeds tried for min_margin > 1e-6: 5 (1.005e-6: above the bar by a hair, not kept) and 6 (2.4e-5, kept)."""
    from foundpose_amd import crop_util
    rng = np.random.default_rng(seed)
    Tw = np.eye(4)
    Tw[:3, :3], Tw[:3, 3] = rot_xyz(0.3, -0.2, 0.5), (120.0, -40.0, 800.0)
    frame = crop_util.PinholePlaneCameraModel(64, 48, (150.0, 152.0), (31.5, 23.5), Tw)
    crop = crop_util.construct_crop_camera(crop_util.AlignedBox2f(36.0, 10.0, 64.0, 38.0), frame, (100, 100), 0.2)
    solve, frames = [frame, crop], [frame, frame]
    A = np.stack([np.eye(3), (np.linalg.inv(frame.T_world_from_eye) @ crop.T_world_from_eye)[:3, :3]])
    cam = camera_tuple(frame)
    bumps = [np.array([0.6, 0.64, -0.48]), np.array([-0.8, 0.0, -0.6])]
    verts = []
    for o, n in enumerate((600, 1203)):
        d = sphere_dirs(n, rng)
        rng.shuffle(d)   # (the stride of the sample must not follow the lattice)
        verts.append((d * blob_radius(d, bumps[o])[:, None]).astype(np.float32))
    tau = [3.0, 2.5]
    # planted poses, model -> SOLVE camera
    R0 = rot_xyz(*rng.uniform(-0.4, 0.4, 3))
    t0 = np.array([-12.0 + rng.uniform(-1, 1), 3.0 + rng.uniform(-1, 1), 400.0 + rng.uniform(-5, 5)])
    R1 = rot_xyz(*rng.uniform(-0.4, 0.4, 3))
    # the crop camera looks at a box at the right border: on its axis the blob's right part leaves the 64-pixel-wide frame
    t1 = np.array([14.0 + rng.uniform(-1, 1), 2.0 + rng.uniform(-1, 1), 410.0 + rng.uniform(-5, 5)])
    depth = np.full((2, 48, 64), 1000.0, np.float32)
    splat(depth[0], cam, A[0] @ R0, A[0] @ t0, bumps[0])
    splat(depth[1], cam, A[1] @ R1, A[1] @ t1, bumps[1])
    depth[0, 26:31, 8:40] = np.minimum(depth[0, 26:31, 8:40], np.float32(t0[2] - 80.0))   # the occluder: 40 mm in front of the blob's front
    depth[1, 14:22, 40:52] = 0.0                                                            # holes
    depth = (np.rint(depth.astype(np.float64) / 0.1).astype(np.int64).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    axis = t0 / np.linalg.norm(t0)  # the view axis through the blob: a turn about it keeps the blob where it is
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rturn = np.eye(3) + 2.0 * K @ K   # the rotation by pi about `axis`
    R = np.stack([R0, R0, Rturn @ R0, R1, R1, R1])
    t = np.stack([t0, along_ray(t0, 3.0 * tau[0]), Rturn @ t0, t1, t1, np.array([2.0, 1.0, 30.0])])
    success = np.array([True, True, True, False, True, True])
    return dict(success=success, R=R, t=t, solve=solve, frames=frames, A=A, image_index=[0, 1], tau=tau, depth=depth, verts=verts,
                det_obj=[0, 1], n_slots=3, grid=16, max_points=700, planted=(0, 4), bumps=bumps)


def fixture_bank_tables(fix):
    """The fixture's compact samples as DeviceBank.verify_points builds them, from the product's own host functions (no device).  Comparing
    DeviceBank.verify_points with this is therefore a comparison of the product with itself: the independent check of the sampling rule, the
    centres and the radii is tests/test_pose_verify_cpu.py::test_bank_sample_is_every_sth_row (plain slices and numpy) -- keep it."""
    import torch
    from foundpose_amd import bank
    V = torch.from_numpy(np.concatenate(fix["verts"]))
    n0 = len(fix["verts"][0])
    pts, ranges = bank.sample_verify_points(V, [(0, n0), (n0, len(V))], fix["max_points"])
    centers, radii = bank.sample_spheres(pts, ranges)
    return pts.numpy(), ranges, centers, radii


def run_ref_on(fix, R=None, t=None, success=None, zbuffer=True, min_visible=16):
    pts, ranges, centers, radii = fixture_bank_tables(fix)
    objs = fix["det_obj"]
    return pose_verify_ref(fix["success"] if success is None else success, fix["R"] if R is None else R, fix["t"] if t is None else t,
                           [camera_tuple(c) for c in fix["frames"]], fix["A"], fix["image_index"], fix["tau"], [ranges[o] for o in objs],
                           centers[objs], radii[objs], pts, fix["depth"], fix["n_slots"], fix["grid"], min_visible, zbuffer)


def make_bank(fix):
    """A DeviceBank whose two objects carry the fixture's vertices (one template each, a few random features: nothing here matches)."""
    import torch
    from foundpose_amd import repre_util
    from foundpose_amd.bank import DeviceBank
    g = torch.Generator().manual_seed(0)
    repres = []
    for V in fix["verts"]:
        n = len(V)
        repres.append(repre_util.FeatureBasedObjectRepre(
            vertices=torch.from_numpy(V), feat_vectors=torch.randn(n, 8, generator=g), feat_to_template_ids=torch.zeros(n, dtype=torch.int32),
            feat_cluster_centroids=torch.randn(4, 8, generator=g), feat_cluster_idfs=torch.ones(4), template_descs=torch.rand(1, 4, generator=g) + 0.1,
            template_desc_opts=repre_util.TemplateDescOpts()))
    return DeviceBank(repres)
