"""GPU: fp_vsd_counts (csrc/vsd.hip) against the numpy restatement tests/vsd_ref.py count for count on rasterizer renders
(occluders, holes, boxes on the image border, empty renders) and on depths built to land exactly on a tau; determinism, batch
independence, argument checks; eval_bop19.evaluate_bop19 and its CLI end to end on a BOP tree written to tmp_path."""
import json

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, eval_bop19 as eb, ops, synthetic
from foundpose_amd.eval_bop19 import _Camera
from foundpose_amd.renderer import HipRasterizer, load_ply
from tests import vsd_ref

pytestmark = pytest.mark.gpu
TAUS = eb.VSD_TAUS
W, H = 160, 120
K = np.array([[150.0, 0, 81.5], [0, 151.0, 58.0], [0, 0, 1]])


def _rot(rng, deg=180.0):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    ang = np.deg2rad(rng.uniform(-deg, deg))
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _render(ras, lid, poses):
    out = ras.render_views(lid, [_Camera(K, W, H, np.linalg.inv(T)) for T in poses], with_color=False)
    return out["depth"], out["boxes"].cpu().numpy()


def _union(a, b):
    x0, y0, x1, y1 = min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])
    return (0, 0, -1, -1) if x0 > x1 else (x0, y0, x1, y1)


@pytest.fixture(scope="module")
def scene():
    """Renders of two blob meshes: GT poses (one on the image border, one off screen, so empty), estimates near them, and
    test images composited from the GT renders, an occluder object in front, a background plane and holes."""
    rng = np.random.default_rng(11)
    ras = HipRasterizer("cuda")
    meshes = {1: synthetic.make_blob_mesh(30, 30, radius=40.0, seed=3), 2: synthetic.make_blob_mesh(24, 24, radius=30.0, seed=4)}
    for lid, m in meshes.items():
        ras.add_object_model(lid, mesh=m)
    gt_t = [np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(500, 800)]) for _ in range(6)]
    gt_t[4] = np.array([300.0, 10.0, 600.0])    # across the right border
    gt_t[5] = np.array([3000.0, 0.0, 600.0])    # off screen: an empty render
    gt = [_pose(_rot(rng), t) for t in gt_t]
    est = []
    for T in gt:
        for k in range(2):
            est.append(_pose(T[:3, :3] @ _rot(rng, 8 * (k + 1)), T[:3, 3] + rng.normal(0, 6 * (k + 1), 3)))
    lid_of_gt = [1, 2, 1, 2, 1, 1]
    dg, bg, de, be = [], [], [], []
    for i, T in enumerate(gt):
        d, b = _render(ras, lid_of_gt[i], [T])
        dg.append(d[0]), bg.append(b[0])
        d, b = _render(ras, lid_of_gt[i], est[2 * i:2 * i + 2])
        de += [d[0], d[1]]
        be += [b[0], b[1]]
    occ, _ = _render(ras, 2, [_pose(_rot(rng), [0.0, 0.0, 420.0])])
    tests = []
    for i in range(len(gt)):
        t = torch.full((H, W), 900.0, device="cuda")
        for g in (dg[i], occ[0]):
            t = torch.where((g > 0) & (g < t), g, t)
        t[rng.integers(0, H - 10):, rng.integers(0, W - 30):][:10, :30] = 0.0    # a hole
        t[::7, ::5] = 0.0
        tests.append(t)
    return dict(dt=torch.stack(tests), dg=torch.stack(dg), de=torch.stack(de), bg=bg, be=be, n=len(gt))


def _pairs(sc, delta=15.0, diam=90.0):
    pairs, params = [], []
    for i in range(sc["n"]):
        for k in range(2):
            e = 2 * i + k
            pairs.append((i, e, i) + _union(sc["be"][e], sc["bg"][i]))
            params.append((K[0, 0], K[1, 1], K[0, 2], K[1, 2], delta, diam))
        pairs.append((i, 2 * ((i + 1) % sc["n"]), i) + _union(sc["be"][2 * ((i + 1) % sc["n"])], sc["bg"][i]))   # a wrong GT
        params.append((K[0, 0], K[1, 1], K[0, 2], K[1, 2], delta, diam))
    return np.array(pairs), np.array(params)


def _ref(sc, pairs, params):
    dt, de, dg = (sc[k].cpu().numpy() for k in ("dt", "de", "dg"))
    Kp = lambda q: np.array([[q[0], 0, q[2]], [0, q[1], q[3]], [0, 0, 1]])
    return np.stack([vsd_ref.vsd_counts(dt[p[0]], de[p[1]], dg[p[2]], Kp(q), q[4], q[5], TAUS) for p, q in zip(pairs, params)])


def test_counts_equal_the_numpy_restatement_on_renders(scene):
    pairs, params = _pairs(scene)
    assert scene["bg"][4][2] == W - 1                                              # a box on the border
    assert scene["bg"][5][0] > scene["bg"][5][2]                                     # an empty GT render
    got = ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs, params, TAUS).cpu().numpy()
    want = _ref(scene, pairs, params)
    assert np.array_equal(got, want)
    assert want[:, 0].min() == 0 and want[:, 0].max() > 300 and (want[:, 0] > want[:, 1]).any() and (want[:, 2:] > 0).any()
    # another delta, a non-integer one, and a smaller diameter
    for delta, diam in ((5.0, 40.0), (25.5, 200.0), (0.1, 60.0)):
        pairs, params = _pairs(scene, delta, diam)
        assert np.array_equal(ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs, params, TAUS).cpu().numpy(),
                              _ref(scene, pairs, params)), (delta, diam)


def test_distances_landing_exactly_on_a_tau():
    """Constant planes: at the principal point dist = depth exactly, so |500 - 532| / diameter is an exact fp64 quotient;
    the diameter is chosen (by ulp steps) so that it equals tau_k exactly."""
    Kc = np.array([[200.0, 0, 40.0], [0, 200.0, 30.0], [0, 0, 1]])
    h, w = 60, 80
    dt = torch.zeros(1, h, w, device="cuda")
    dg = torch.full((1, h, w), 500.0, device="cuda")
    de = torch.full((1, h, w), 532.0, device="cuda")
    pairs, params, want = [], [], []
    for k, tau in enumerate(TAUS):
        diam = 32.0 / tau
        for _ in range(64):
            if 32.0 / diam == tau:
                break
            diam = np.nextafter(diam, np.inf if 32.0 / diam > tau else -np.inf)
        if 32.0 / diam != tau:   # no fp64 diameter gives this quotient exactly (0.45)
            continue
        pairs.append((0, 0, 0, 0, 0, w - 1, h - 1))
        params.append((Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2], 15.0, diam))
        want.append(vsd_ref.vsd_counts(dt[0].cpu().numpy(), de[0].cpu().numpy(), dg[0].cpu().numpy(), Kc, 15.0, diam, TAUS))
        # the principal-point pixel is counted for tau_k (e >= tau) and not for tau_k+1
        d0 = abs(vsd_ref.dist_im(dg[0].cpu().numpy(), Kc)[30, 40] - vsd_ref.dist_im(de[0].cpu().numpy(), Kc)[30, 40]) / diam
        assert d0 == tau
    assert len(pairs) >= 9
    got = ops.vsd_counts(dt, de, dg, np.array(pairs), np.array(params), TAUS).cpu().numpy()
    assert np.array_equal(got, np.stack(want))


def test_deterministic_and_independent_of_the_batch(scene):
    pairs, params = _pairs(scene)
    a = ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs, params, TAUS).cpu().numpy()
    b = ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs, params, TAUS).cpu().numpy()
    assert np.array_equal(a, b)
    perm = np.random.default_rng(0).permutation(len(pairs))
    c = ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs[perm], params[perm], TAUS).cpu().numpy()
    assert np.array_equal(c, a[perm])
    for p in range(len(pairs)):
        one = ops.vsd_counts(scene["dt"], scene["de"], scene["dg"], pairs[p:p + 1], params[p:p + 1], TAUS[3:5]).cpu().numpy()
        assert np.array_equal(one[0], np.concatenate([a[p, :2], a[p, 5:7]])), p


def test_invalid_arguments_write_nothing():
    lib = _lib.lib()
    d = torch.zeros(2, 8, 10, device="cuda")
    counts = torch.full((2, 12), -7, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    good_p = np.array([[0, 1, 1, 0, 0, 9, 7], [1, 0, 0, 2, 3, 1, 2]], np.int32)    # the second box is empty
    good_q = np.array([[100.0, 100, 5, 4, 15, 50]] * 2)
    taus = np.ascontiguousarray(TAUS)

    def call(p=good_p, q=good_q, n=2, t=taus, nt=10, h=8, w=10, nbytes=1024, null=None):
        ptrs = [_lib.ptr(d)] * 3
        if null is not None:
            ptrs[null] = _lib.vp(0)
        p, q, t = (np.ascontiguousarray(x) for x in (np.asarray(p, np.int32), np.asarray(q, np.float64), np.asarray(t, np.float64)))
        return lib.fp_vsd_counts(ptrs[0], 2, ptrs[1], 2, ptrs[2], 2, h, w, p.ctypes.data_as(_lib.vp), q.ctypes.data_as(_lib.vp), n,
                                 t.ctypes.data_as(_lib.vp), nt, _lib.ptr(scratch), nbytes, _lib.ptr(counts), _lib.stream())
    bad = [call(n=0), call(n=-1), call(nt=0), call(nt=17), call(nbytes=100), call(h=0)] + [call(null=k) for k in range(3)]
    for row, col, v in ((0, 0, 2), (0, 1, -1), (1, 2, 2), (0, 5, 10), (0, 6, 8), (0, 3, -1), (1, 3, 3), (1, 5, 0)):
        p = good_p.copy()
        p[row, col] = v
        bad.append(call(p=p))
    for col, v in ((0, 0.0), (1, -1.0), (5, 0.0), (5, np.nan), (4, np.nan)):
        q = good_q.copy()
        q[1, col] = v
        bad.append(call(q=q))
    t = taus.copy()
    t[3] = np.nan
    bad.append(call(t=t))
    torch.cuda.synchronize()
    assert bad == [1] * len(bad)   # FP_ERR_INVALID
    assert (counts == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (counts[1] == 0).all() and counts[0, 0] == 0      # zero depths everywhere: empty unions


def test_cpu_tensors_raise():
    z = torch.zeros(1, 4, 4)
    with pytest.raises(_lib.FoundPoseNativeError, match="CPU tensor"):
        ops.vsd_counts(z, z, z, [[0, 0, 0, 0, 0, 3, 3]], [[1.0, 1, 0, 0, 15, 10]], TAUS)


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluate_bop19_on_a_bop_tree(tmp_path):
    meta = synthetic.make_bop_eval_scene(str(tmp_path), num_images=3, num_objects=2, gts_per_image=2, depth_scale=0.1, seed=5)
    images, diam = meta["images"], meta["diameters"]

    def write(path, ests):
        synthetic.write_bop_results_csv(str(path), [(1, im, lid, score, T, 0.5 + im) for im, lid, score, T in ests])
        return str(path)

    # estimates equal to the GT: every recall is 1
    perfect = [(im, lid, 1.0, T) for im, inst in images for lid, T in inst]
    s = eb.evaluate_bop19(write(tmp_path / "perfect.csv", perfect), meta["split_dir"])
    assert s["bop19_average_recall"] == 1.0 and np.all(np.array(s["recall_vsd"]) == 1.0)
    assert s["recall_mssd"] == [1.0] * 10 and s["recall_mspd"] == [1.0] * 10
    assert s["num_unrenderable_estimates"] == 0 and s["num_estimates_evaluated"] == len(perfect) == s["num_target_instances"]
    assert abs(s["bop19_average_time_per_image"] - 1.5) < 1e-12

    # every estimate shifted along x by 0.12 diameter: MSSD = 0.12 d (correct for 0.15 .. 0.5), MSPD = fx s / min z
    shifted, want_mspd = [], []
    for im, inst in images:
        for lid, T in inst:
            T2 = T.copy()
            T2[0, 3] += 0.12 * diam[lid]
            shifted.append((im, lid, 1.0, T2))
            v = load_ply(f"{meta['models_dir']}/obj_{lid:06d}.ply").vertices.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            want_mspd.append(meta["K"][0, 0] * 0.12 * diam[lid] / v[:, 2].min())
    s2 = eb.evaluate_bop19(write(tmp_path / "shifted.csv", shifted), meta["split_dir"], details=True)
    assert s2["recall_mssd"] == [0.0, 0.0] + [1.0] * 8
    ths = np.arange(5, 51, 5) * (meta["width"] / 640.0)
    want = np.mean([[m < th for th in ths] for m in want_mspd], axis=0)
    assert all(min(abs(m - ths)) > 0.05 for m in want_mspd)       # no value near a threshold
    assert np.array_equal(np.array(s2["recall_mspd"]), want)
    # its VSD errors are the numpy restatement's on the same renders and the same stored depths
    ras = HipRasterizer("cuda")
    for lid in diam:
        ras.add_object_model(lid, mesh=load_ply(f"{meta['models_dir']}/obj_{lid:06d}.ply"))
    cams = json.load(open(f"{meta['split_dir']}/000001/scene_camera.json"))
    gts = json.load(open(f"{meta['split_dir']}/000001/scene_gt.json"))
    checked = 0
    for e in s2["errors"]:
        im, lid = e["im_id"], e["obj_id"]
        dt = eb.load_depth(f"{meta['split_dir']}/000001/depth/{im:06d}.png", cams[str(im)]["depth_scale"])
        g = gts[str(im)][e["gt_id"]]
        Tg = eb._m2c(g["cam_R_m2c"], g["cam_t_m2c"])
        Te = [x[3] for x in shifted if x[0] == im and x[1] == lid][0]
        render = lambda T: ras.render_views(lid, [_Camera(meta["K"], meta["width"], meta["height"], np.linalg.inv(T))], with_color=False)["depth"][0].cpu().numpy()
        want_vsd = vsd_ref.vsd(dt, render(Te), render(Tg), meta["K"], 15.0, diam[lid], TAUS)
        assert e["vsd"] == want_vsd.tolist()
        checked += 1
    assert checked == len(shifted)

    # top-n: a better-scored bad estimate pushes the perfect one out; a near-plane estimate is unrenderable and never VSD-correct
    im0, (lid0, T0) = images[0][0], images[0][1][0]
    bad = T0.copy()
    bad[:3, 3] += [1.5 * diam[lid0], 0, 0]
    near = images[1][1][0][1].copy()
    near[2, 3] = 50.0
    ests = [(im, lid, 1.0, T) for im, inst in images for lid, T in inst if (im, lid) not in ((im0, lid0), (images[1][0], images[1][1][0][0]))]
    ests += [(im0, lid0, 0.5, T0), (im0, lid0, 0.9, bad), (images[1][0], images[1][1][0][0], 1.0, near)]
    s3 = eb.evaluate_bop19(write(tmp_path / "mixed.csv", ests), meta["split_dir"], details=True)
    n = s3["num_target_instances"]
    assert s3["num_unrenderable_estimates"] == 1 and s3["num_estimates_evaluated"] == n
    assert s3["recall_mssd"][-1] == (n - 2) / n                        # the bad one (kept) and the near-plane one are wrong
    assert np.all(np.array(s3["recall_vsd"]) == (n - 2) / n)
    near_rows = [e for e in s3["errors"] if not e["renderable"]]
    assert len(near_rows) == 1 and near_rows[0]["vsd"] == [1.0] * 10
    assert all(e["score"] != 0.5 for e in s3["errors"])               # the lower-scored estimate was dropped

    # the CLI writes what the function returns
    out = tmp_path / "scores.json"
    eb.main(["--result-csv", str(tmp_path / "mixed.csv"), "--dataset-dir", meta["split_dir"], "--output", str(out)])
    s4 = eb.evaluate_bop19(str(tmp_path / "mixed.csv"), meta["split_dir"])
    assert json.load(open(out)) == json.loads(json.dumps(s4))
