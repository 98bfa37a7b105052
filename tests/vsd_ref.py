"""numpy restatement of fp_vsd_counts (csrc/vsd.hip) in numpy's own operation order: bop_toolkit_lib's
misc.depth_im_to_dist_im_fast, visibility._estimate_visib_mask in `bop19` mode and pose_error.vsd with the `step` cost,
as published (the toolkit is not installed here)."""
import numpy as np


def dist_im(depth: np.ndarray, K: np.ndarray) -> np.ndarray:
    """misc.depth_im_to_dist_im_fast: fp32 depth -> fp64 distance from the optical centre."""
    h, w = depth.shape
    xs = (np.arange(w) - K[0, 2]) / np.float64(K[0, 0])
    ys = (np.arange(h) - K[1, 2]) / np.float64(K[1, 1])
    Xs = np.multiply(xs[None, :], depth)
    Ys = np.multiply(ys[:, None], depth)
    return np.sqrt(Xs ** 2 + Ys ** 2 + depth.astype(np.float64) ** 2)


def visib_mask(d_test: np.ndarray, d_model: np.ndarray, delta: float) -> np.ndarray:
    """visibility._estimate_visib_mask, bop19 mode (delta a Python float: numpy compares the fp32 difference in fp32)."""
    d_diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    return np.logical_and(np.logical_or(d_diff <= float(delta), d_test == 0), d_model > 0)


def vsd_counts(depth_test, depth_est, depth_gt, K, delta, diameter, taus) -> np.ndarray:
    """-> int64 [2 + T]: |union|, |intersection|, per tau the intersection pixels with dist >= tau."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    dist_test = dist_im(np.asarray(depth_test, np.float32), K)
    dist_gt = dist_im(np.asarray(depth_gt, np.float32), K)
    dist_est = dist_im(np.asarray(depth_est, np.float32), K)
    visib_gt = visib_mask(dist_test, dist_gt, delta)
    visib_est = np.logical_or(visib_mask(dist_test, dist_est, delta), np.logical_and(visib_gt, dist_est > 0))
    inter = np.logical_and(visib_gt, visib_est)
    union = np.logical_or(visib_gt, visib_est)
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    dists /= diameter
    return np.array([union.sum(), inter.sum()] + [(dists >= tau).sum() for tau in taus], np.int64)


def vsd(depth_test, depth_est, depth_gt, K, delta, diameter, taus) -> np.ndarray:
    """pose_error.vsd from the counts: (sum(costs) + visib_comp_count) / float(visib_union_count), 1 for an empty union."""
    c = vsd_counts(depth_test, depth_est, depth_gt, K, delta, diameter, taus)
    if c[0] == 0:
        return np.ones(len(taus))
    return np.array([(c[2 + t] + (c[0] - c[1])) / float(c[0]) for t in range(len(taus))])
