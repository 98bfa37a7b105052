"""numpy restatement of utils/eval_errors.py mssd / mspd (with bop_toolkit_lib.misc.transform_pts_Rt / project_pts), written
elementwise in the operation order csrc/pose_eval.hip documents, so that exact inputs give bit-equal results; plus the
reference's own (BLAS) form, which is what the tolerances of the comparisons cover."""
import numpy as np


def _affine(r, t, p):
    return ((r[0] * p[:, 0] + r[1] * p[:, 1]) + r[2] * p[:, 2]) + t


def transform(R, t, pts):
    t = np.asarray(t, np.float64).reshape(3)
    return np.stack([_affine(R[i], t[i], pts) for i in range(3)], 1)


def project(P, pts):
    with np.errstate(divide="ignore", invalid="ignore"):
        w = _affine(P[2, :3], P[2, 3], pts)
        return np.stack([_affine(P[0, :3], P[0, 3], pts) / w, _affine(P[1, :3], P[1, 3], pts) / w], 1)


def compose(R_gt, t_gt, syms):
    """(R_gt S_R, R_gt S_t + t_gt) of every symmetry, as eval_util.pose_errors_batch composes them."""
    SR = np.stack([s["R"] for s in syms])
    St = np.stack([np.asarray(s["t"], np.float64).reshape(3, 1) for s in syms])
    return np.matmul(R_gt, SR), np.matmul(R_gt, St) + np.asarray(t_gt, np.float64).reshape(3, 1)


def errors(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """-> (mssd, mssd vertex, mssd sym, mspd, mspd vertex, mspd sym) with the reference's selection rules:
    np.max / np.argmax per symmetry, Python's min() for the value and np.argmin for the symmetry."""
    R_gs, t_gs = compose(R_gt, t_gt, syms)
    t_est = np.asarray(t_est, np.float64).reshape(3, 1)
    pe = transform(R_est, t_est, pts)
    qe = project(K.dot(np.hstack((R_est, t_est))), pts)
    out = []
    for metric in ("mssd", "mspd"):
        es, ind = [], []
        for s in range(len(syms)):
            if metric == "mssd":
                d = transform(R_gs[s], t_gs[s], pts) - pe
                e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            else:
                d = qe - project(K.dot(np.hstack((R_gs[s], t_gs[s]))), pts)
                e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            es.append(e.max())
            ind.append(int(e.argmax()))
        k = int(np.argmin(np.array(es)))
        out += [min(es), ind[k], k]
    return tuple(out)


def rows(R_est, t_est, R_gt, t_gt, K, syms):
    """The kernel's input rows of one hypothesis: est [12], p_est [12], gt_sym [S, 12], p_gt [S, 12]."""
    t_est = np.asarray(t_est, np.float64).reshape(3, 1)
    R_gs, t_gs = compose(R_gt, t_gt, syms)
    est = np.concatenate([R_est.reshape(9), t_est.reshape(3)])
    p_est = K.dot(np.hstack((R_est, t_est))).reshape(12)
    gt = np.concatenate([R_gs.reshape(-1, 9), t_gs.reshape(-1, 3)], 1)
    p_gt = np.matmul(K, np.concatenate([R_gs, t_gs], 2)).reshape(-1, 12)
    return est, p_est, gt, p_gt
