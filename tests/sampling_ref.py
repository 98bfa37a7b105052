"""Plain restatement of the query-feature hand-off (numpy, no GPU): what sits between the ViT's feature map and the matcher.

* sample_bilinear: the rounding sequence of sample_bilinear_kernel (csrc/match.hip) and ln_sample_kernel (csrc/vit.hip), which is the one of
  torch's CPU grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False) in fp32:
      sx = 2 / img_w;  ux = sx * px;  u1 = (ux - 1) + 1 (two roundings);  ix = fma(u1, W / 2, -0.5);
      w = ix - floor(ix), e = 1 - w (and n, s in y);  weights s*e, s*w, n*e, n*w, each rounded;
      acc = v_nw * w_nw, then fma over ne, sw, se;  a tap outside the map contributes 0.
  fma32 is an exact fp32 fused multiply-add built from fp64 operations (Python before 3.13 has no math.fma).
* pca_project: out[i, j] = fp32(chain(x_i, c_j) - chain(mean, c_j)), chain = the k-ascending fmaf chain of oracle.clib.dot_rows (the
  F32_EPI_SUB_VEC / F32_EPI_STORE epilogues of csrc/f32_tile.hip behind fp_pca_project).
* row norms: oracle.clib.sqnorm and oracle.match.l2_normalize_rows already state x / max(sqrt(chain), eps); nothing is restated here.
* the case tables (fixed seeds) shared by tests/test_sampling_cpu.py (the restatement against torch, the tables bite) and
  tests/test_gpu_sampling.py (the kernels against the restatement).

Non-finite point coordinates are out of scope: grid_sample's result for a NaN or infinite coordinate depends on the float -> int
conversion of the platform, and no caller produces one (query points are grid-cell centres inside a mask)."""

from collections import namedtuple

import numpy as np

from oracle import clib

F32 = np.float32
U24 = 2.0 ** -24


def gamma(n):
    """n u / (1 - n u), u = 2^-24: the constant of the standard forward bound of n chained fp32 roundings."""
    return n * U24 / (1.0 - n * U24)


# ------------------------------------------------------------------------------------------------ exact fp32 fma
def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, elementwise.  The product of two fp32 numbers is exact in fp64 (48 bits); the fp64 sum p + c is
    rounded TO ODD (TwoSum gives its exact error: when the sum is inexact and its last bit even, step to the neighbour on the error's side),
    and a round-to-odd fp64 value rounds to fp32 like the exact one (53 >= 24 + 2 bits).  float64(a) * float64(b) + float64(c) rounded to
    nearest twice is NOT this: it differs whenever the fp64 sum lands on an fp32 tie it did not start from.  Finite operands only."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                       # exact: s + err == p + c
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F32)


# ------------------------------------------------------------------------------------------------ bilinear sampling
Taps = namedtuple("Taps", "x0 y0 valid wx wy ux uy")
"""Per point: x0, y0 int64 (the north-west tap; x1 = x0 + 1, y1 = y0 + 1), valid bool [P, 4] in the order nw, ne, sw, se, the fractional
weights wx = ix - x0 and wy = iy - y0, and ux, uy = (2 / size) * p before the round trip through -1, +1."""

WRONG = ("no_round_trip", "swap_image", "swap_map", "x1_le_w", "tap_order", "align_corners")
"""Deliberately wrong variants of sample_bilinear (tests/test_sampling_cpu.py: the point table must tell each from torch)."""


def _axis(p, size, n, wrong):
    """One coordinate: pixel position p [P] fp32 in an image of `size` pixels, on a map of n cells -> (index coordinate, u before the round trip)."""
    s = F32(2.0) / F32(size)
    u = (s * p).astype(F32)
    u1 = u if wrong == "no_round_trip" else ((u - F32(1.0)).astype(F32) + F32(1.0)).astype(F32)
    if wrong == "align_corners":
        return (u1 * (F32(n - 1) / F32(2.0))).astype(F32), u
    return fma32(u1, F32(n) / F32(2.0), F32(-0.5)), u


def sample_bilinear(fmap_bchw, points, point_img, image_size, wrong=None):
    """fmap [B, C, H, W] fp32, points [P, 2] (x, y) in image coordinates, point_img [P] or None (image 0), image_size (width, height)
    -> (out [P, C] fp32, Taps).  wrong: None, or one of WRONG."""
    assert wrong is None or wrong in WRONG
    f = np.asarray(fmap_bchw, dtype=F32)
    pts = np.asarray(points, dtype=F32).reshape(-1, 2)
    B, C, H, W = f.shape
    img_w, img_h = int(image_size[0]), int(image_size[1])
    if wrong == "swap_image":
        img_w, img_h = img_h, img_w
    nx, ny = (H, W) if wrong == "swap_map" else (W, H)
    img = np.zeros(pts.shape[0], np.int64) if point_img is None else np.asarray(point_img).astype(np.int64)
    ix, ux = _axis(pts[:, 0], img_w, nx, wrong)
    iy, uy = _axis(pts[:, 1], img_h, ny, wrong)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    w = (ix - fx).astype(F32)
    e = (F32(1.0) - w).astype(F32)
    n = (iy - fy).astype(F32)
    s = (F32(1.0) - n).astype(F32)
    hi_x, hi_y = (W + 1, H + 1) if wrong == "x1_le_w" else (W, H)
    vx0, vx1 = (x0 >= 0) & (x0 < W), (x1 >= 0) & (x1 < hi_x)
    vy0, vy1 = (y0 >= 0) & (y0 < H), (y1 >= 0) & (y1 < hi_y)

    def tap(vx, vy, x, y):           # [P, C]: the map's value where the tap is valid, +0 elsewhere (an index past the map is clamped, then dropped)
        ok = vx & vy
        v = f[img, :, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return np.where(ok[:, None], v, F32(0.0)).astype(F32), ok

    v_nw, k_nw = tap(vx0, vy0, x0, y0)
    v_ne, k_ne = tap(vx1, vy0, x1, y0)
    v_sw, k_sw = tap(vx0, vy1, x0, y1)
    v_se, k_se = tap(vx1, vy1, x1, y1)
    w_nw, w_ne, w_sw, w_se = ((s * e).astype(F32)[:, None], (s * w).astype(F32)[:, None], (n * e).astype(F32)[:, None], (n * w).astype(F32)[:, None])
    acc = (v_nw * w_nw).astype(F32)
    rest = [(v_ne, w_ne), (v_sw, w_sw), (v_se, w_se)]
    if wrong == "tap_order":
        rest = [rest[1], rest[0], rest[2]]
    for v, wt in rest:
        acc = fma32(v, wt, acc)
    return acc, Taps(x0, y0, np.stack([k_nw, k_ne, k_sw, k_se], 1), w, n, ux, uy)


# ------------------------------------------------------------------------------------------------ PCA projection
def chain_matrix(x, c):
    """[n, D] x [d, D] -> [n, d] fp32: out[i, j] = the k-ascending fmaf chain over x[i, k] * c[j, k], started at +0."""
    x, c = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c, dtype=F32)
    out = np.empty((x.shape[0], c.shape[0]), F32)
    for j in range(c.shape[0]):
        out[:, j] = clib.dot_rows(x, c[j])
    return out


def pca_project(x, components, mean):
    """sklearn's PCA.transform without whitening as the device computes it: chain(x_i, c_j) - chain(mean, c_j), the difference rounded once;
    mean None: the chain alone."""
    y = chain_matrix(x, components)
    if mean is None:
        return y
    mp = chain_matrix(np.asarray(mean, dtype=F32).reshape(1, -1), components)
    return (y - mp).astype(F32)


# ------------------------------------------------------------------------------------------------ case tables
SAMPLE_MAPS = [            # (B, C, H, W, img_w, img_h)
    (1, 48, 37, 37, 518, 518),     # the shape of tests/golden/points_sample_pca.npz
    (3, 65, 12, 20, 280, 168),     # non-square map and image, one pass of the 64 lanes plus one channel, three images
    (2, 130, 16, 16, 224, 224),    # two lane passes plus two channels
    (1, 1, 1, 1, 14, 14),          # one cell: every point has taps outside
    (2, 384, 74, 74, 518, 518),    # the stride-7 grid at the production channel count
]
NUM_POINTS = 401               # not a multiple of the 4 points a block takes
CLASSES = "abcdefg"
MIN_PER_CLASS = 8
MIN_ROUND_TRIP = 20


def sample_map(i):
    """Map i of SAMPLE_MAPS: standard-normal fp32 [B, C, H, W] from a fixed seed."""
    B, C, H, W, _, _ = SAMPLE_MAPS[i]
    return np.random.default_rng(7100 + i).standard_normal((B, C, H, W)).astype(F32)


def sample_points(i):
    """The NUM_POINTS points of map i -> (points [P, 2] fp32, point_img [P] int32 or None where B == 1, label [P] of CLASSES)."""
    B, C, H, W, img_w, img_h = SAMPLE_MAPS[i]
    return make_points(B, H, W, img_w, img_h, 7200 + i)


def make_points(B, H, W, img_w, img_h, seed):
    """NUM_POINTS points of every class for B maps of H x W cells over images of img_w x img_h pixels -> (points, point_img, label) as
    sample_points returns them.  A coordinate is made from the index coordinate it should land on: p = (i + 0.5) * cell.  The labels say how
    a point was MADE; what it is (x0, y0, validity) is read off the restatement by classify()."""
    rng = np.random.default_rng(seed)
    cx, cy = img_w / W, img_h / H

    def px(ixc):
        return (np.asarray(ixc, np.float64) + 0.5) * cx

    def py(iyc):
        return (np.asarray(iyc, np.float64) + 0.5) * cy

    def inner_x(k):      # both taps valid where the map has two cells; on a one-cell map: anywhere between the two outer cell centres
        return px(rng.uniform(0.05, W - 1.05, k)) if W > 1 else px(rng.uniform(-0.95, 0.95, k))

    def inner_y(k):
        return py(rng.uniform(0.05, H - 1.05, k)) if H > 1 else py(rng.uniform(-0.95, 0.95, k))

    lo, hi_x, hi_y = (-0.95, -0.05), (W - 0.95, W - 0.05), (H - 0.95, H - 0.05)
    parts = []

    def add(label, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        parts.append((label, np.stack([x.ravel(), y.ravel()], 1)))

    k = 80                                                                           # (a) cell centres (2 / img_w is not a power of two: on
                                                                                     #     some maps only one centre in five lands on weight 0)
    add("a", px(rng.integers(0, W, k)), py(rng.integers(0, H, k)))
    k = 10                                                                           # (b) x0 == -1, y0 == -1, both
    add("b", px(rng.uniform(*lo, k)), inner_y(k))
    add("b", inner_x(k), py(rng.uniform(*lo, k)))
    add("b", px(rng.uniform(*lo, k)), py(rng.uniform(*lo, k)))
    add("c", px(rng.uniform(*hi_x, k)), inner_y(k))                                  # (c) x1 == W, y1 == H, both
    add("c", inner_x(k), py(rng.uniform(*hi_y, k)))
    add("c", px(rng.uniform(*hi_x, k)), py(rng.uniform(*hi_y, k)))
    k = 5                                                                            # (d) more than one cell beyond each of the four sides
    across_x, across_y = px(rng.uniform(-3.0, W + 2.0, 2 * k)), py(rng.uniform(-3.0, H + 2.0, 2 * k))
    add("d", px(rng.uniform(-4.0, -2.2, k)), across_y[:k])
    add("d", px(rng.uniform(W + 1.2, W + 3.0, k)), across_y[k:])
    add("d", across_x[:k], py(rng.uniform(-4.0, -2.2, k)))
    add("d", across_x[k:], py(rng.uniform(H + 1.2, H + 3.0, k)))
    ex, ey = [0.0, float(img_w), img_w / 2.0, 0.5], [0.0, float(img_h), img_h / 2.0, 0.5]     # (e) exact values, every pairing
    gx, gy = np.meshgrid(ex, ey, indexing="ij")
    add("e", gx, gy)
    add("e", [float(img_h)], [float(img_w)])
    far = 1.0e6                                                                      # (f) far points
    add("f", [far, far, -far, -far], [far, -far, far, -far])
    add("f", [far, -far], inner_y(2))
    add("f", inner_x(2), [far, -far])
    used = sum(p.shape[0] for _, p in parts)                                         # (g) random interior points
    add("g", inner_x(NUM_POINTS - used), inner_y(NUM_POINTS - used))
    label = np.concatenate([np.full(p.shape[0], l) for l, p in parts])
    pts = np.concatenate([p for _, p in parts]).astype(F32)
    order = rng.permutation(NUM_POINTS)                                              # the classes spread over the blocks
    assert pts.shape == (NUM_POINTS, 2)
    img = rng.integers(0, B, NUM_POINTS).astype(np.int32) if B > 1 else None
    return pts[order], img, label[order]


def classify(taps, H, W):
    """What the points ARE, from the restatement's own x0, y0 -> dict of bool [P] masks:
    a: both fractional weights exactly 0;  bx / by: x0 == -1 with x1 valid / the same in y;  cx / cy: x1 == W with x0 valid / the same in y;
    d_left, d_right, d_up, d_down: all four taps outside AND more than one cell beyond that side;  all_out: all four taps outside;
    round_trip: (u - 1) + 1 != u in x or in y."""
    x0, y0 = taps.x0, taps.y0
    rt = lambda u: ((u - F32(1.0)).astype(F32) + F32(1.0)).astype(F32) != u       # noqa: E731
    all_out = ~taps.valid.any(1)
    return {
        "a": (taps.wx == 0) & (taps.wy == 0),
        "bx": (x0 == -1) & (W >= 1), "by": (y0 == -1) & (H >= 1),
        "cx": (x0 == W - 1), "cy": (y0 == H - 1),
        "all_out": all_out,
        "d_left": all_out & (x0 < -2), "d_right": all_out & (x0 > W), "d_up": all_out & (y0 < -2), "d_down": all_out & (y0 > H),
        "round_trip": rt(taps.ux) | rt(taps.uy),
    }


PCA_SHAPES = [             # (n, D, d)
    (1, 48, 16),           # smallest
    (133, 36, 100),        # ragged rows and columns, a K tail of 4 behind one 32-wide step
    (64, 1024, 65),        # the <= 64-row wave cut; one live column in the second tile column
    (129, 1024, 256),      # two column tiles, one live row in the second row tile
    (517, 384, 256),       # a 518 crop's disc of patches
    (260, 768, 256),       # three row tiles
]
PCA_CASES = [(s, True) for s in PCA_SHAPES] + [((133, 36, 100), False)]      # (shape, with a mean); the last one: mean=None


def pca_case(shape, with_mean):
    """-> (x [n, D], components [d, D], mean [D] or None), fp32.  Standard-normal components and spread; the mean is 10 x the spread on five
    channels (0.1 x elsewhere) and x is drawn AROUND it, so x C^T carries mean C^T (about 10 sqrt(5) in magnitude, against sqrt(D) for what is
    left) and the subtraction cancels it."""
    n, D, d = shape
    rng = np.random.default_rng(7300 + n + D + d)
    comps = rng.standard_normal((d, D)).astype(F32)
    x = rng.standard_normal((n, D)).astype(F32)
    if not with_mean:
        return x, comps, None
    mean = (0.1 * rng.standard_normal(D)).astype(F32)
    big = rng.choice(D, 5, replace=False)
    mean[big] = (10.0 * np.where(rng.random(5) < 0.5, -1.0, 1.0) * (1.0 + 0.1 * rng.random(5))).astype(F32)
    return (x + mean).astype(F32), comps, mean


SQNORM_SHAPES = [(1, 4), (257, 36), (255, 1024), (1000, 256)]
NORMALIZE_SHAPES = [(1, 1), (5, 63), (6, 64), (7, 65), (9, 1000), (4, 2048)]
EPS = 1e-8
SPECIAL_ROWS = ("one", "zero", "tiny", "huge")
FLT_MAX = float(np.finfo(F32).max)


def sqnorm_case(shape):
    return np.random.default_rng(7400 + shape[0] + shape[1]).standard_normal(shape).astype(F32)


def normalize_case(shape):
    """-> (x [n, d] fp32, {special name: row}).  Rows 0 .. min(n, 4) - 1 are, in the order of SPECIAL_ROWS (a one-row case keeps the first):
    one:  a single non-zero element (-3.75, in the last column), expected -1 there;
    zero: all zero, expected zeros;
    tiny: elements of magnitude 1e-12, norm below eps = 1e-8, expected x / eps;
    huge: elements of magnitude 1e18 where d of their squares overflow fp32 (d >= 341), else 3e19, whose square overflows alone: the chain is
          +inf, expected x / inf = 0.
    The rows behind them are standard normal."""
    n, d = shape
    rng = np.random.default_rng(7500 + n + d)
    x = rng.standard_normal(shape).astype(F32)
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    rows = {}
    for r, name in enumerate(SPECIAL_ROWS[:min(n, 4)]):
        rows[name] = r
        if name == "one":
            x[r] = 0.0
            x[r, d - 1] = -3.75
        elif name == "zero":
            x[r] = 0.0
        elif name == "tiny":
            x[r] = (sign * 1e-12 * (1.0 + rng.random(d))).astype(F32)
        else:
            mag = 1e18 if d * 1e36 > FLT_MAX else 3e19
            x[r] = (sign * mag).astype(F32)
    return x, rows
