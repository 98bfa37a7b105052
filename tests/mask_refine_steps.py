"""The fixtures of the silhouette refinement's tests (TEST HELPER; tests/test_mask_refine_cpu.py, tests/test_gpu_mask_refine.py), in the
manner of tests/lm_steps.py: small problems on the blob of tests/pose_verify_ref.py whose restated trajectory (tests/mask_refine_ref.py)
is decided on clear margins, and the four recovery starts on the 144 x 192 image.

A fixture is a MaskFixture: det (X fp32 [N, 3], R, t the start pose, cam, mask uint8 [H, W], delta, K_max), run(iters, reverse=False) -> the
restatement's dict, gaps(R, t) -> the smallest relative distance of a per-row branch from flipping at a pose.  It carries entry = "depth"
so that tests/lm_steps.pinned_prefix holds it to the margin of the fp64 depth entry, 1e-6.
"""

import functools

import numpy as np

from tests import lm_steps
from tests import mask_refine_ref as mr
from tests import pose_verify_ref as pv

BUMP = np.array([0.6, 0.64, 0.48])
TILE = 256                                     # FP_MASK_REFINE_TILE: the contour pass's LDS tile of projected points
SMALL = dict(H=48, W=64, cam=(120.0, 125.0, 31.0, 25.0), t=(6.0, -5.0, 400.0))
LARGE = dict(H=144, W=192, cam=(360.0, 375.0, 93.0, 75.0), t=(6.0, -5.0, 400.0))
R_TRUE = lm_steps.fr.rot_exp(np.array([0.3, -0.2, 0.25]))


def blob_points(n, rng=None):
    d = pv.sphere_dirs(n, rng)
    return (d * pv.blob_radius(d, BUMP / np.linalg.norm(BUMP))[:, None]).astype(np.float32)


DENSE = 120000


@functools.lru_cache(maxsize=None)
def dense_points():
    return blob_points(DENSE).astype(np.float64)


@functools.lru_cache(maxsize=None)
def planted_mask(size):
    """The rint splat of the dense blob (DENSE points: a filled silhouette, as a detection's mask is) at the planted pose.  Shared: leave
    it unchanged."""
    s = LARGE if size == "large" else SMALL
    X = dense_points()
    m = mr.splat_mask(R_TRUE, np.array(s["t"]), X, s["cam"], s["H"], s["W"])
    m.setflags(write=False)
    return m


class MaskFixture:
    entry = "depth"

    def __init__(self, name, det, K):
        self.name, self.det, self.K = name, det, K
        self.d2 = mr.mask_distance(det["mask"])
        self.q = mr.contour_rows(det["mask"], det["K_max"])

    def __repr__(self):
        return f"mask:{self.name}"

    def run(self, iters, reverse=False, **lm):
        d = self.det
        X = np.asarray(d["X"], np.float32).astype(np.float64)[::-1 if reverse else 1]
        return mr.refine(d["R"], d["t"], X, d["cam"], d["mask"], d["delta"], iters, d["K_max"], d.get("has_pose", True), d2=self.d2, q=self.q, **lm)

    def gaps(self, R, t):
        """floor(u), floor(v) (which hold the image bounds, integers too), z against 1, |r| against delta of both terms, and for every
        contour row the best against the second-best squared distance."""
        d = self.det
        X = np.asarray(d["X"], np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            f = mr.forward_terms(R, t, X, d["cam"], self.d2, d["delta"])
            b = mr.backward_terms(R, t, X, d["cam"], self.q, d["delta"])
            fr_ = f["front"]
            parts = [f["z"] - 1.0, (f["u"][fr_] - np.rint(f["u"][fr_])) / np.maximum(np.abs(f["u"][fr_]), 1.0),
                     (f["v"][fr_] - np.rint(f["v"][fr_])) / np.maximum(np.abs(f["v"][fr_]), 1.0),
                     (np.abs(f["r"][f["measurable"]]) - d["delta"]) / d["delta"]]
            if "rs" in b:
                parts += [(b["rs"] - d["delta"]) / d["delta"], (b["s2"] - b["s1"]) / np.maximum(b["s1"], 1e-300)]
            return lm_steps._rel(*parts)


def small_fixture(seed, n, K_max, rot_deg, trans_mm, delta=4.0, K=12):
    rng = np.random.default_rng(seed)
    X = blob_points(n, rng)
    R0, t0 = lm_steps._off(rng, R_TRUE, np.array(SMALL["t"]), rot_deg, trans_mm)
    return MaskFixture(f"n{n}_k{K_max}_s{seed}", dict(X=X, R=R0, t=t0, cam=SMALL["cam"], mask=planted_mask("small"), delta=delta, K_max=K_max), K)


# "name" -> (seed, N, K_max, start rotation in degrees, start translation in mm): N = 70 is three chunks of FP_REFINE_CHUNK = 32 with a ragged
# last one, N = TILE + 1 one more point than the contour pass's LDS tile; K' = 6 (the least that is refined), 33 (two chunks, one row in the
# second), 70.  The seeds are those whose restated trajectory alone holds the margins tests/test_mask_refine_cpu.py asserts.
SPECS = {
    "n70_k70": (4, 70, 70, 8.0, 25.0),        # accepts, then a run of rejections, accepts again
    "n70_k33": (1, 70, 33, 8.0, 25.0),
    "n70_k6": (1, 70, 6, 12.0, 35.0),         # rejections and accepts in turn
    "n257_k70": (3, TILE + 1, 70, 8.0, 25.0),
}
IDS = tuple(SPECS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    seed, n, K_max, rot, trans = SPECS[name]
    fx = small_fixture(seed, n, K_max, rot, trans)
    fx.name = name
    return fx


def prefix(fx, iters=30):
    """tests/lm_steps.pinned_prefix of a mask fixture."""
    return lm_steps.pinned_prefix(fx, iters)


# ---------------------------------------------------------------------------------------------------------- recovery
def _lateral(t):
    """t's component across the planted ray, and along it."""
    ray = np.array(LARGE["t"]) / np.linalg.norm(LARGE["t"])
    d = np.asarray(t) - np.array(LARGE["t"])
    along = float(d @ ray)
    return float(np.linalg.norm(d - along * ray)), abs(along)


def recovery_starts():
    """The four starts of the 144 x 192 fixture: 17 mm sideways, 60 mm along the ray, 12 degrees + 20 mm, a mix.  -> [(name, R, t, lateral?)]."""
    t = np.array(LARGE["t"])
    ray = t / np.linalg.norm(t)
    side = np.cross(ray, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    up = np.cross(ray, side)
    turn = lm_steps.fr.rot_exp(np.radians(12.0) * np.array([0.0, 0.0, 1.0]))
    mix = lm_steps.fr.rot_exp(np.radians(6.0) * np.array([0.6, 0.0, 0.8]))
    return [("sideways", R_TRUE, t + 17.0 * side, True), ("along", R_TRUE, t + 60.0 * ray, False),
            ("turned", turn @ R_TRUE, t + 20.0 * up, True), ("mix", mix @ R_TRUE, t + 10.0 * side - 8.0 * up + 35.0 * ray, True)]


@functools.lru_cache(maxsize=None)
def recovery_problem():
    """X fp32 [4000, 3], the planted mask, its distance field and contour rows (cap 1024).  Shared: leave unchanged."""
    X = blob_points(4000)
    mask = planted_mask("large")
    return X, mask, mr.mask_distance(mask), mr.contour_rows(mask, 1024)


@functools.lru_cache(maxsize=None)
def recovery_run(name, iters=30, delta=8.0):
    """The restatement from one of the four starts.  -> dict: the restatement's, + iou_in, iou_out, lat_in, lat_out, along_in, along_out."""
    X, mask, d2, q = recovery_problem()
    _, R0, t0, _ = next(s for s in recovery_starts() if s[0] == name)
    Xd = X.astype(np.float64)
    out = mr.refine(R0, t0, Xd, LARGE["cam"], mask, delta, iters, 1024, d2=d2, q=q)
    return dict(out, **recovery_scores(R0, t0, out["R"], out["t"]))


def recovery_scores(R0, t0, R1, t1):
    _, mask, _, _ = recovery_problem()
    Xd = dense_points()          # the silhouette of a pose is the dense blob's, not the 4 000-point sample's
    (lat_in, along_in), (lat_out, along_out) = _lateral(t0), _lateral(t1)
    return dict(iou_in=mr.splat_iou(R0, t0, Xd, LARGE["cam"], mask), iou_out=mr.splat_iou(R1, t1, Xd, LARGE["cam"], mask), lat_in=lat_in,
                lat_out=lat_out, along_in=along_in, along_out=along_out, rot_out=float(np.degrees(np.arccos(np.clip((np.trace(R1 @ R_TRUE.T) - 1) / 2, -1, 1)))))
