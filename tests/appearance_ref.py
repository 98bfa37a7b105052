"""The yardstick of the appearance score: numpy restatements of the contracts of fp_proposal_patch_cover and
fp_proposal_appearance (include/foundpose_amd.h).  Coverage is in integers; similarities are in fp64, and `replay` restates the steps
behind the similarities -- best match, mean, status, combined score -- in fp32 from a given similarity matrix, so a device result can be
replayed from the device's own similarities bit for bit."""
import numpy as np


def crop_window(box, size):
    """(w', h', ox, oy) of fp_proposal_crops' window for a box (x1, y1, x2, y2)."""
    x1, y1, x2, y2 = (int(v) for v in box)
    w, h = x2 - x1, y2 - y1
    L = max(w, h)
    wo, ho = max(1, (2 * w * size + L) // (2 * L)), max(1, (2 * h * size + L) // (2 * L))
    return wo, ho, (size - wo) // 2, (size - ho) // 2


def box_ok(box, H, W, image_index=0, n_img=1):
    x1, y1, x2, y2 = (int(v) for v in box)
    return 0 <= image_index < n_img and x1 >= 0 and y1 >= 0 and x2 <= W and y2 <= H and x2 > x1 and y2 > y1


def patch_cover(mask, box, size, ps, image_index=0, n_img=1):
    """mask [H, W] (0 / non-zero) -> int32 [(size / ps)^2]: the covered pixels of every patch cell, row-major."""
    assert size % ps == 0
    g = size // ps
    out = np.zeros(g * g, np.int32)
    H, W = mask.shape
    if not box_ok(box, H, W, image_index, n_img):
        return out
    x1, y1, x2, y2 = (int(v) for v in box)
    w, h = x2 - x1, y2 - y1
    wo, ho, ox, oy = crop_window(box, size)
    for Y in range(oy, oy + ho):
        sy = y1 + ((2 * (Y - oy) + 1) * h) // (2 * ho)
        for X in range(ox, ox + wo):
            sx = x1 + ((2 * (X - ox) + 1) * w) // (2 * wo)
            if mask[sy, sx]:
                out[(Y // ps) * g + X // ps] += 1
    return out


def template_rows(obj_off, num_bank, best_obj, best_template):
    """-> the bank row of every proposal, -1 where there is none; obj_off clamped into [0, num_bank] and made non-decreasing."""
    off = [min(max(int(obj_off[0]), 0), num_bank)]
    for v in obj_off[1:]:
        off.append(min(max(int(v), off[-1]), num_bank))
    rows = []
    for o, t in zip(best_obj, best_template):
        o, t = int(o), int(t)
        rows.append(off[o] + t if 0 <= o < len(off) - 1 and 0 <= t < off[o + 1] - off[o] else -1)
    return rows


def similarities_f64(q, bank, rows):
    """q [P, Np, D], bank [N, Np, D] -> fp64 sim [P, Np (query), Np (template)]; zeros for a proposal of no row."""
    P, Np, _ = q.shape
    out = np.zeros((P, Np, Np), np.float64)
    for p, r in enumerate(rows):
        if r >= 0:
            out[p] = q[p].astype(np.float64) @ bank[r].astype(np.float64).T
    return out


def replay(sim, q_cover, bank_cover, rows, best_score, min_cover):
    """Steps 4 to 7 of the contract in fp32 from sim [P, Np, Np] (any float type: it is rounded to fp32 first).
    -> (best_sim f32 [P, Np], best_patch int32 [P, Np], appearance f32 [P], n_valid int32 [P], status int32 [P], score f32 [P])."""
    sim = np.asarray(sim).astype(np.float32)
    P, Np = q_cover.shape
    best_sim, best_patch = np.zeros((P, Np), np.float32), np.full((P, Np), -1, np.int32)
    appearance, n_valid, status = np.zeros(P, np.float32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, r in enumerate(rows):
        if r < 0:
            status[p] = 2
            continue
        qv = q_cover[p] >= min_cover
        tv = bank_cover[r] >= min_cover
        n_valid[p] = int(qv.sum())
        status[p] = 1 if n_valid[p] == 0 else (0 if tv.any() else 3)
        if status[p] != 0:
            continue
        total = None
        for j in range(Np):
            if not qv[j]:
                continue
            best, arg = np.float32(-np.inf), -1
            for i in range(Np):
                if tv[i] and sim[p, j, i] > best:   # false for a NaN and at equality
                    best, arg = sim[p, j, i], i
            best_sim[p, j], best_patch[p, j] = best, arg
            with np.errstate(invalid="ignore"):
                total = best if total is None else np.float32(total + best)
        with np.errstate(invalid="ignore"):
            appearance[p] = np.float32(total / np.float32(n_valid[p]))
    with np.errstate(invalid="ignore"):
        score = ((np.asarray(best_score, np.float32) + appearance) * np.float32(0.5)).astype(np.float32)
    return best_sim, best_patch, appearance, n_valid, status, score


def replay_from_best(best_sim, q_cover, bank_cover, rows, best_score, min_cover):
    """Steps 5 to 7 from a given best_sim [P, Np] (the device's own): -> (appearance, n_valid, status, score) as `replay` gives them."""
    best_sim = np.asarray(best_sim, np.float32)
    P, Np = q_cover.shape
    appearance, n_valid, status = np.zeros(P, np.float32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, r in enumerate(rows):
        if r < 0:
            status[p] = 2
            continue
        qv = q_cover[p] >= min_cover
        n_valid[p] = int(qv.sum())
        status[p] = 1 if n_valid[p] == 0 else (0 if (bank_cover[r] >= min_cover).any() else 3)
        if status[p] != 0:
            continue
        total = None
        for j in np.nonzero(qv)[0]:
            with np.errstate(invalid="ignore"):
                total = best_sim[p, j] if total is None else np.float32(total + best_sim[p, j])
        with np.errstate(invalid="ignore"):
            appearance[p] = np.float32(total / np.float32(n_valid[p]))
    with np.errstate(invalid="ignore"):
        score = ((np.asarray(best_score, np.float32) + appearance) * np.float32(0.5)).astype(np.float32)
    return appearance, n_valid, status, score
