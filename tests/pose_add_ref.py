"""numpy restatement of fp_pose_add_errors (include/foundpose_amd.h, csrc/pose_add.hip) and of eval_add's protocol, written
from the contract, not from the kernel: the placement in the contract's operation order, a brute-force fmin minimum per query point, the root
after the minimum, and cumsum-ordered tile sums (np.cumsum is sequential; np.sum is pairwise and would not be the contract's order).  numpy's
elementwise fp64 +, -, *, / and sqrt are IEEE operations rounded one by one, so the device must agree with this file bit for bit."""

import math

import numpy as np

TILE = 256   # FP_POSE_ADD_TILE


def place(pose12, pts):
    """[12] = R row-major | t, pts [M, 3] -> [M, 3]: ((r0 x + r1 y) + r2 z) + t per row."""
    R, t = np.asarray(pose12, np.float64)[:9].reshape(3, 3), np.asarray(pose12, np.float64)[9:]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)


def _sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nn_sq(G, E, chunk=512):
    """Per row of G the smallest squared distance to a row of E: from +inf, a candidate wins only when strictly smaller, a NaN never."""
    out = np.empty(G.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, G.shape[0], chunk):
            s = _sq(G[c0:c0 + chunk, None, :] - E[None, :, :])
            out[c0:c0 + chunk] = np.fmin.reduce(s, axis=1, initial=np.inf)
    return out


def tiled_mean(vals):
    """Tiles of 256 consecutive values summed in ascending order, the tile sums in ascending order, / (double)M."""
    tiles = np.array([np.cumsum(vals[i:i + TILE])[-1] for i in range(0, len(vals), TILE)], np.float64)
    return np.cumsum(tiles)[-1] / np.float64(len(vals))


def pair_errors(pts, est12, gt12):
    """(add, adi) of one pair; pts [M, 3] its own points."""
    pts = np.asarray(pts, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        E, G = place(est12, pts), place(gt12, pts)
        a = np.sqrt(_sq(G - E))
        n = np.sqrt(nn_sq(G, E))
        return tiled_mean(a), tiled_mean(n)


def batch_errors(pts, est, gt, ranges):
    """fp_pose_add_errors: pts [V, 3], est / gt [H, 12], ranges [H, 2] = (pt_off, pt_cnt) -> err [H, 2]."""
    return np.array([pair_errors(pts[o:o + c], est[h], gt[h]) for h, (o, c) in enumerate(np.asarray(ranges))], np.float64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------- the protocol
def is_symmetric(info, obj_id, symmetric_ids=None):
    return bool(info.get("symmetries_discrete")) or bool(info.get("symmetries_continuous")) or (symmetric_ids is not None and obj_id in list(symmetric_ids))


def auc(d, auc_max):
    """VOCap of the YCB-Video toolbox over the errors d, as a fraction of auc_max; plain Python on purpose."""
    d = sorted(float(x) for x in d if not math.isnan(float(x))) + [math.nan] * sum(1 for x in d if math.isnan(float(x)))
    n = len(d)
    pts = [(x, (k + 1) / n) for k, x in enumerate(d) if x <= auc_max]
    if not pts:
        return 0.0
    mrec = [0.0] + [p[0] for p in pts] + [float(auc_max)]
    mpre = [0.0] + [p[1] for p in pts] + [pts[-1][1]]
    for i in range(1, len(mpre)):
        mpre[i] = max(mpre[i], mpre[i - 1])
    terms = [(mrec[i] - mrec[i - 1]) * mpre[i] for i in range(1, len(mrec)) if mrec[i] != mrec[i - 1]]
    return float(np.sum(np.array(terms, np.float64)) / float(auc_max)) if terms else 0.0


def match(err):
    """err [n_est, n_gt], estimates in rank order -> per GT the estimate it got (-1: none): each estimate takes the unmatched GT with the
    lowest error, ties to the lower GT, valid or not."""
    err = np.asarray(err, np.float64)
    got = [-1] * err.shape[1]
    for e in range(err.shape[0]):
        best = None
        for g in range(err.shape[1]):
            if got[g] >= 0:
                continue
            v = math.inf if math.isnan(err[e, g]) else err[e, g]
            if best is None or v < best[0]:
                best = (v, g)
        if best is not None:
            got[best[1]] = e
    return got


def summarize(tables, recall_factor=0.1, auc_max=100.0):
    """eval_add's details=True tables -> {"mean", "all", "per_object"} of (recall_add_s, auc_add, auc_adi, auc_add_s)."""
    err, sym, diam = tables["err"], tables["symmetric"], tables["diameters"]
    inst = {}
    for t in tables["targets"]:
        lid, n_est, valid = t["obj_id"], t["n_est"], list(t["valid"])
        n_gt = len(valid)
        e = np.asarray(err[t["pair_off"]:t["pair_off"] + n_est * n_gt]).reshape(n_est, n_gt, 2)
        got = match(e[:, :, 1 if sym[lid] else 0])
        for g in range(n_gt):
            if valid[g]:
                a, s = (math.inf, math.inf) if got[g] < 0 else (float(e[got[g], g, 0]), float(e[got[g], g, 1]))
                inst.setdefault(lid, []).append((a, s, s if sym[lid] else a, diam[lid]))

    def sc(rows):
        return {"recall_add_s": sum(1 for r in rows if r[2] < recall_factor * r[3]) / len(rows),
                "auc_add": auc([r[0] for r in rows], auc_max), "auc_adi": auc([r[1] for r in rows], auc_max),
                "auc_add_s": auc([r[2] for r in rows], auc_max)}
    per = {lid: sc(rows) for lid, rows in sorted(inst.items())}
    mean = {k: float(np.mean([per[lid][k] for lid in per])) for k in ("recall_add_s", "auc_add", "auc_adi", "auc_add_s")}
    return {"mean": mean, "all": sc([r for lid in sorted(inst) for r in inst[lid]]), "per_object": per}
