"""numpy fp64 restatement of the result-picture contract: every kernel of csrc/vis.hip and the
assembly of the per-detection tile in foundpose_amd/vis_util.py.  Written from the contract, not from the kernels; images
are uint8 HWC, one detection at a time."""
import numpy as np


def pca_colorize(fmap, H, W):
    """fmap [gh, gw, C] -> uint8 [H, W, 3]: channels 0..2, ONE (lo, hi) for the three, trunc(255 (x - lo) / (hi - lo)), nearest upsampling."""
    x = np.asarray(fmap, np.float64)[:, :, :3]
    gh, gw = x.shape[:2]
    lo, hi = x.min(), x.max()
    v = np.zeros_like(x) if hi == lo else np.trunc(255.0 * ((x - lo) / (hi - lo)))   # the quotient first: exactly 1 at hi
    ys = (np.arange(H) * gh) // H
    xs = (np.arange(W) * gw) // W
    return v[ys][:, xs].astype(np.uint8)


def mask_tint(img, mask):
    out = np.asarray(img, np.uint8).copy()
    on = np.asarray(mask) != 0
    out[on] = ((out[on].astype(np.int64) + 255) >> 1).astype(np.uint8)
    return out


def edge(mask):
    """Set pixels with an unset 4-neighbour inside the image."""
    m = np.asarray(mask) != 0
    unset = ~m
    e = np.zeros_like(m)
    e[:, 1:] |= unset[:, :-1]
    e[:, :-1] |= unset[:, 1:]
    e[1:, :] |= unset[:-1, :]
    e[:-1, :] |= unset[1:, :]
    return e & m


def dilate(e, iterations=1):
    e = np.asarray(e, bool)
    H, W = e.shape
    for _ in range(iterations):
        p = np.zeros((H + 2, W + 2), bool)
        p[1:-1, 1:-1] = e
        e = np.zeros((H, W), bool)
        for dy in range(3):
            for dx in range(3):
                e |= p[dy:dy + H, dx:dx + W]
    return e


def contour(img, mask, colour, dilate_iterations=1):
    out = np.asarray(img, np.uint8).copy()
    out[dilate(edge(mask), dilate_iterations)] = np.asarray(colour, np.uint8)
    return out


def resize_area(src, oh, ow):
    """Footprint-area-weighted mean, rounded to nearest; downscaling only."""
    src = np.asarray(src, np.float64)
    h, w = src.shape[:2]
    if oh > h or ow > w:
        raise ValueError("downscaling only")

    def weights(n, on):
        m = np.zeros((on, n))
        for o in range(on):
            a, b = o * n / on, (o + 1) * n / on
            for s in range(int(np.floor(a)), min(n, int(np.ceil(b)))):
                m[o, s] = max(0.0, min(b, s + 1) - max(a, s))
        return m / m.sum(1, keepdims=True)
    wy, wx = weights(h, oh), weights(w, ow)
    out = np.tensordot(wx, np.tensordot(wy, src, axes=(1, 0)), axes=(1, 1)).transpose(1, 0, 2)   # rows first, then columns
    return np.floor(out + 0.5).astype(np.uint8)


def segment_distance(px, py, seg):
    x0, y0, x1, y1 = (float(v) for v in seg)
    dx, dy = x1 - x0, y1 - y0
    l2 = dx * dx + dy * dy
    t = np.zeros_like(px) if l2 == 0 else np.clip(((px - x0) * dx + (py - y0) * dy) / l2, 0.0, 1.0)
    return np.hypot(px - (x0 + t * dx), py - (y0 + t * dy))


def segment_coverage(d, lw):
    return np.clip(0.5 + lw / 2.0 - d, 0.0, 1.0)


def disc_coverage(d, r):
    return np.clip(0.5 + r - d, 0.0, 1.0)


def draw_matches(tile, segs, colour=(230, 230, 230), alpha=1.0, lw=1.0, radius=2.5):
    """segs [N, 4] (x0, y0, x1, y1), in the given order: segment, disc at (x0, y0), disc at (x1, y1); rounded once at the end."""
    out = np.asarray(tile, np.float64).copy()
    H, W = out.shape[:2]
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    col = np.asarray(colour, np.float64)
    for s in np.asarray(segs, np.float64).reshape(-1, 4):
        for cov in (segment_coverage(segment_distance(px, py, s), lw),
                    disc_coverage(np.hypot(px - s[0], py - s[1]), radius), disc_coverage(np.hypot(px - s[2], py - s[3]), radius)):
            a = (alpha * cov)[..., None]
            out = out * (1.0 - a) + col * a
    return np.rint(out).astype(np.uint8)


def scene_composite(img, depth, colours):
    """depth [K, H, W] (0 = background) -> (out, ids): nearest positive layer per pixel, ties to the lowest k."""
    d = np.asarray(depth, np.float64)
    z = np.where(d > 0, d, np.inf)
    ids = np.argmin(z, axis=0).astype(np.int32)           # first minimum = lowest k
    ids[~np.isfinite(z.min(axis=0))] = -1
    out = np.asarray(img, np.uint8).copy()
    on = ids >= 0
    out[on] = ((out[on].astype(np.int64) + np.asarray(colours, np.int64)[ids[on]]) >> 1).astype(np.uint8)
    return out, ids


# ---------------------------------------------------------------------------------------------------- tile assembly
def select_matches(conf, left, right, top_n, W, H):
    """The top_n correspondences by conf (stable, descending, ties to the lower index), those whose right point lies in
    [0, W) x [0, H) kept, least confident first -> segments [n, 4] with the right point shifted by (W, 0).  A NaN
    confidence (0 / 0 in the matcher) ranks below every number."""
    conf = np.asarray(conf, np.float64)
    conf = np.where(np.isnan(conf), -np.inf, conf)
    order = sorted(range(len(conf)), key=lambda i: (-conf[i], i))[:top_n]
    left, right = np.asarray(left, np.float64), np.asarray(right, np.float64)
    keep = [i for i in order if 0 <= right[i, 0] < W and 0 <= right[i, 1] < H]
    keep = keep[::-1]
    return np.array([[left[i, 0], left[i, 1], right[i, 0] + W, right[i, 1]] for i in keep], np.float64).reshape(-1, 4)


def strip_size(n, Ht, Wt, W):
    """Row 2: n templates side by side, area-resized to 2W wide (vis_util.py:428-446) -> (height, width)."""
    return int(Ht * 2 * W / (n * Wt)), 2 * W


def darken(img):
    return ((np.asarray(img, np.int64) * 9) // 10).astype(np.uint8)


def tile(row1_left, row1_right, templates, row3_left, row3_right, segs):
    """uint8 [H + h2 + H, 2W, 3]."""
    H, W = row1_left.shape[:2]
    strip = np.concatenate(list(templates), axis=1)
    h2, w2 = strip_size(len(templates), templates[0].shape[0], templates[0].shape[1], W)
    row3 = draw_matches(np.concatenate([row3_left, row3_right], axis=1), segs)
    return np.concatenate([np.concatenate([row1_left, row1_right], axis=1), resize_area(strip, h2, w2), row3], axis=0)
