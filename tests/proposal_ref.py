"""numpy fp64 restatement of the proposal-labelling contracts (include/foundpose_amd.h: fp_mask_boxes, fp_proposal_crops, fp_proposal_scores,
fp_proposal_rank, fp_box_iou) and of detect_util.label_proposals' selection rules.  Plain loops: this file is the
yardstick, not an implementation."""

import numpy as np

DECISIONS = ("candidate", "small", "empty", "no_object", "low_score", "group_limit")


# ---------------------------------------------------------------------------------------------------- boxes
def mask_boxes(masks):
    """masks [P, H, W] -> (boxes int32 [P, 4] = (x1, y1, x2, y2), x2 / y2 exclusive; area int32 [P]); an empty mask gives zeros."""
    masks = np.asarray(masks) != 0
    boxes, area = np.zeros((len(masks), 4), np.int32), np.zeros(len(masks), np.int32)
    for p, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        area[p] = ys.size
        if ys.size:
            boxes[p] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes, area


# ---------------------------------------------------------------------------------------------------- crops
def crop_window(box, S):
    """-> (w', h', ox, oy) of the box's window in the S x S crop."""
    w, h = int(box[2]) - int(box[0]), int(box[3]) - int(box[1])
    L = max(w, h)
    wo, ho = max(1, (2 * w * S + L) // (2 * L)), max(1, (2 * h * S + L) // (2 * L))
    return wo, ho, (S - wo) // 2, (S - ho) // 2


def axis_weights(n_in, n_out):
    """The antialiased-bilinear taps of one axis: [(lo, weights fp64 [hi - lo], summing to 1)] per output index."""
    scale = n_in / n_out
    sup = max(scale, 1.0)
    out = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - sup + 0.5)), min(n_in, int(c + sup + 0.5))
        raw = np.array([max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)], np.float64)
        out.append((lo, raw / raw.sum()))
    return out


def resample(x, n_out_h, n_out_w):
    """x fp64 [h, w, C] -> [n_out_h, n_out_w, C], separable."""
    h, w, _ = x.shape
    wx, wy = axis_weights(w, n_out_w), axis_weights(h, n_out_h)
    tmp = np.stack([np.tensordot(wt, x[:, lo:lo + len(wt)], axes=(0, 1)) for lo, wt in wx], 1)       # [h, n_out_w, C]
    return np.stack([np.tensordot(wt, tmp[lo:lo + len(wt)], axes=(0, 0)) for lo, wt in wy], 0)      # [n_out_h, n_out_w, C]


def proposal_crop(image, mask, box, S):
    """image [H, W, 3], mask [H, W], box (x1, y1, x2, y2) -> (crop fp64 [3, S, S], status)."""
    H, W = mask.shape
    x1, y1, x2, y2 = (int(v) for v in box)
    out = np.zeros((3, S, S), np.float64)
    if not (0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H):
        return out, 2
    wo, ho, ox, oy = crop_window(box, S)
    src = np.asarray(image, np.float64)[y1:y2, x1:x2] * (np.asarray(mask)[y1:y2, x1:x2, None] != 0)
    out[:, oy:oy + ho, ox:ox + wo] = resample(src, ho, wo).transpose(2, 0, 1)
    return out, 0


def max_taps(n_in, n_out):
    return max(len(wt) for _, wt in axis_weights(n_in, n_out))


# ---------------------------------------------------------------------------------------------------- scores
def similarities64(desc_n, bank_n):
    return np.asarray(desc_n, np.float64) @ np.asarray(bank_n, np.float64).T


def proposal_scores(sims, obj_off, k):
    """sims: fp32 [P, N] similarities of every proposal with every bank row (the bits the device chain produced); obj_off [O + 1].
    -> (scores f32 [P, O], best_obj int32 [P], best_score f32 [P], best_template int32 [P]) with the fp32 adds of the contract."""
    sims = np.asarray(sims, np.float32)
    P, O = sims.shape[0], len(obj_off) - 1
    scores = np.full((P, O), -np.inf, np.float32)
    best_obj, best_tpl = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    best_score = np.full(P, -np.inf, np.float32)
    for p in range(P):
        for o in range(O):
            row = sims[p, obj_off[o]:obj_off[o + 1]]
            m = min(k, row.size)
            if m == 0:
                continue
            top = sorted(range(row.size), key=lambda t: (-row[t], t))[:m]   # value descending, equal values by the lower template id
            s = np.float32(row[top[0]])
            for t in top[1:]:
                s = np.float32(s + row[t])
            s = np.float32(s / np.float32(m))
            scores[p, o] = s
            if s > best_score[p]:
                best_obj[p], best_score[p], best_tpl[p] = o, s, top[0]
    return scores, best_obj, best_score, best_tpl


# ---------------------------------------------------------------------------------------------------- overlaps and suppression
def box_iou(boxes, pairs):
    """-> (overlap f64 [M], status int32 [M])."""
    boxes = np.asarray(boxes, np.int64)
    ov, st = np.zeros(len(pairs), np.float64), np.full(len(pairs), 2, np.int32)
    for q, (i, j) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        if not (0 <= i < len(boxes) and 0 <= j < len(boxes)):
            continue
        a, b = boxes[i], boxes[j]
        area_a = max(a[2] - a[0], 0) * max(a[3] - a[1], 0)
        area_b = max(b[2] - b[0], 0) * max(b[3] - b[1], 0)
        inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0) if area_a > 0 and area_b > 0 else 0
        union = area_a + area_b - inter
        if union > 0:
            ov[q], st[q] = np.float64(inter) / np.float64(union), 0
    return ov, st


def decide(best_obj, best_score, area, crop_status, num_obj, min_area, min_score, max_group=256):
    """fp_proposal_rank's decisions and layout: -> (decision names [P], order: the proposal at each place, group_off [O + 1])."""
    P = len(best_obj)
    names = []
    for p in range(P):
        if area[p] < min_area:
            names.append("small")
        elif crop_status[p] != 0:
            names.append("empty")
        elif not 0 <= best_obj[p] < num_obj:
            names.append("no_object")
        elif not np.float32(best_score[p]) >= np.float32(min_score):
            names.append("low_score")
        else:
            names.append("candidate")
    order, group_off = [], [0]
    for o in range(num_obj):
        members = sorted((p for p in range(P) if names[p] == "candidate" and best_obj[p] == o), key=lambda p: (-best_score[p], p))
        for p in members[max_group:]:
            names[p] = "group_limit"
        order.extend(members[:max_group])
        group_off.append(len(order))
    return names, order, group_off


def group_pairs(group_off):
    """The pairs (a, b), a < b, of every group, a-major -> (pairs [M, 2], pair_off [O + 1])."""
    pairs, pair_off = [], [0]
    for g0, g1 in zip(group_off[:-1], group_off[1:]):
        pairs.extend((a, b) for a in range(g0, g1) for b in range(a + 1, g1))
        pair_off.append(len(pairs))
    return np.asarray(pairs, np.int32).reshape(-1, 2), pair_off


def nms_greedy(boxes_ranked, group_off, thresh):
    """Greedy suppression per group over places in rank order: -> (keep [N] bool, suppressed_by [N], -1 for a kept place).  Two places
    conflict at overlap >= thresh."""
    n = group_off[-1]
    keep, by = np.ones(n, bool), np.full(n, -1, np.int64)
    for g0, g1 in zip(group_off[:-1], group_off[1:]):
        for a in range(g0, g1):
            if not keep[a]:
                continue
            for b in range(a + 1, g1):
                ov, st = box_iou(boxes_ranked, [(a, b)])
                if keep[b] and st[0] == 0 and ov[0] >= thresh:
                    keep[b], by[b] = False, a
    return keep, by


def select(best_obj, best_score, area, crop_status, boxes, num_obj, min_area, min_score, nms_thresh, max_per_image, max_group=256):
    """label_proposals' selection: -> (decision names [P] with "kept" / "suppressed" / "max_per_image" filled in, suppressed_by [P] (a
    proposal index or -1), kept proposals in score order)."""
    names, order, group_off = decide(best_obj, best_score, area, crop_status, num_obj, min_area, min_score, max_group)
    keep, by = nms_greedy(np.asarray(boxes)[order] if order else np.zeros((0, 4), np.int64), group_off, nms_thresh)
    suppressed_by = [-1] * len(best_obj)
    survivors = []
    for place, p in enumerate(order):
        if keep[place]:
            survivors.append(p)
        else:
            names[p], suppressed_by[p] = "suppressed", order[by[place]]
    survivors.sort(key=lambda p: (-best_score[p], p))
    for p in survivors[:max_per_image]:
        names[p] = "kept"
    for p in survivors[max_per_image:]:
        names[p] = "max_per_image"
    return names, suppressed_by, survivors[:max_per_image]
