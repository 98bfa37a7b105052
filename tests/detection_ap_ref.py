"""The BOP 6D detection score restated in numpy fp64 with plain loops: the greedy matching of one estimate group for
one threshold, and the average precision of one object for one column.  It restates the PUBLISHED behaviour of bop_toolkit's detection
scores (eval_calc_scores in detection mode, score.calc_pose_detection_scores); the toolkit is not installed, so nothing here is pinned
against its code.  csrc/detection_ap.hip must equal these functions bit for bit."""

import numpy as np

REC_THR = np.linspace(0, 1, 101)   # the recall thresholds of the score, as fp64 rounds them


def match_group(err, th, valid):
    """err [E, G] fp64, the estimates in rank order; th the threshold; valid [G].  -> (flag [E] int8, matched_gt [E] int32): every estimate
    takes the free GT with the lowest error strictly below th (ties to the lower index; a NaN never matches), valid or not; flag 1 for a
    valid GT, 2 for an invalid one, 0 without a match."""
    err = np.asarray(err, np.float64)
    E, G = err.shape
    taken = [False] * G
    flag, matched = np.zeros(E, np.int8), np.full(E, -1, np.int32)
    for e in range(E):
        best = -1
        for g in range(G):
            if taken[g] or not err[e, g] < th:
                continue
            if best < 0 or err[e, g] < err[e, best]:
                best = g
        if best >= 0:
            taken[best] = True
            matched[e] = best
            flag[e] = 1 if valid[best] else 2
    return flag, matched


def match_batch(est_off, gt_off, pair_off, err, gt_valid, group_tab, ths):
    """fp_detection_match's tables (numpy) -> (flag int8 [N_est, 2 T], matched_gt int32 [N_est, 2 T])."""
    ths = np.asarray(ths, np.float64)
    T = ths.shape[2]
    n_est = int(est_off[-1]) if len(est_off) else 0
    flag, matched = np.zeros((n_est, 2 * T), np.int8), np.full((n_est, 2 * T), -1, np.int32)
    for g in range(len(est_off) - 1):
        e0, e1, g0, g1, p0 = est_off[g], est_off[g + 1], gt_off[g], gt_off[g + 1], pair_off[g]
        E, G = e1 - e0, g1 - g0
        block = np.asarray(err[p0:p0 + E * G], np.float64).reshape(E, G, 2)
        for typ in range(2):
            for k in range(T):
                f, m = match_group(block[:, :, typ], ths[group_tab[g], typ, k], np.asarray(gt_valid[g0:g1]) > 0)
                flag[e0:e1, typ * T + k], matched[e0:e1, typ * T + k] = f, m
    return flag, matched


def average_precision(flags, n_valid, rec_thr=REC_THR):
    """flags: one object's estimates in global rank order for one column (1 true positive, 0 false positive, 2 ignored).
    -> (ap, q [R], (tp, fp, ignored)).  n_valid <= 0: ap = -1 and q = 0."""
    rec_thr = np.asarray(rec_thr, np.float64)
    R = len(rec_thr)
    kept = [int(f) for f in flags if int(f) in (0, 1)]
    totals = (sum(kept), len(kept) - sum(kept), len(flags) - len(kept))
    q = np.zeros(R, np.float64)
    if n_valid <= 0:
        return -1.0, q, totals
    p, r = [], []
    tp = fp = 0
    for f in kept:
        tp += f
        fp += 1 - f
        p.append(np.float64(tp) / np.float64(tp + fp))
        r.append(np.float64(tp) / np.float64(n_valid))
    for k in range(len(p) - 2, -1, -1):          # the envelope: p~_k = max_{j >= k} p_j
        p[k] = max(p[k], p[k + 1])
    for i in range(R):
        for k in range(len(r)):                  # searchsorted(r, rec_thr[i], side="left")
            if r[k] >= rec_thr[i]:
                q[i] = p[k]
                break
    s = q[0]
    for i in range(1, R):
        s = s + q[i]
    return float(s / np.float64(R)), q, totals


def ap_batch(obj_off, order, flag, n_valid, rec_thr=REC_THR):
    """fp_detection_ap's tables (numpy) -> (ap [O, C], q [O, C, R], totals int32 [O, C, 3])."""
    flag = np.asarray(flag)
    O, C, R = len(obj_off) - 1, flag.shape[1], len(rec_thr)
    ap, q, totals = np.zeros((O, C)), np.zeros((O, C, R)), np.zeros((O, C, 3), np.int32)
    for o in range(O):
        rows = np.asarray(order[obj_off[o]:obj_off[o + 1]], np.int64)
        for c in range(C):
            ap[o, c], q[o, c], totals[o, c] = average_precision(flag[rows, c] if len(rows) else [], int(n_valid[o]), rec_thr)
    return ap, q, totals
