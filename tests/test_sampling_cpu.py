"""tests/sampling_ref.py against torch's own arithmetic (CPU only): the restatement the GPU tests of the query-feature hand-off compare the
kernels with must itself be the reference's operation -- grid_sample(bilinear, zeros, align_corners=False) bit for bit, sklearn's
PCA.transform and x / max(|x|, eps) within the forward bounds of their fp64 forms -- and the shared point table must hold the classes of
points at which a sampling kernel goes wrong, and tell six deliberately wrong samplers from torch."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import clib
from oracle import match as om
from tests import sampling_ref as sr
from tests.helpers import load_golden

F32 = np.float32
U = sr.U24
MAPS = list(range(len(sr.SAMPLE_MAPS)))
MAP_IDS = ["x".join(str(v) for v in m) for m in sr.SAMPLE_MAPS]
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _torch_sample(fmap_bchw, pts, img, image_size, dtype):
    """torch's CPU grid_sample per image: uv = (2 / size) * p - 1 in `dtype`, the grid laid out [1, N, 1, 2] -> [P, C]."""
    f = torch.from_numpy(np.asarray(fmap_bchw)).to(dtype)
    p = torch.from_numpy(np.asarray(pts)).to(dtype)
    size = torch.tensor([image_size[0], image_size[1]], dtype=dtype)
    uv = (2.0 / size) * p - 1.0
    img = np.zeros(p.shape[0], np.int64) if img is None else np.asarray(img).astype(np.int64)
    out = torch.zeros(p.shape[0], f.shape[1], dtype=dtype)
    for b in range(f.shape[0]):
        sel = torch.from_numpy(np.nonzero(img == b)[0])
        if sel.numel():
            s = F.grid_sample(f[b:b + 1], uv[sel].reshape(1, -1, 1, 2), mode="bilinear", padding_mode="zeros", align_corners=False)
            out[sel] = s[0, :, :, 0].T
    return out.numpy()


def _case(i):
    """Map i, its points, the restatement and torch's fp32 result on them: computed once, read by every test, never written."""
    if i not in _CACHE:
        fmap = sr.sample_map(i)
        pts, img, label = sr.sample_points(i)
        size = sr.SAMPLE_MAPS[i][4:]
        out, taps = sr.sample_bilinear(fmap, pts, img, size)
        _CACHE[i] = dict(fmap=fmap, pts=pts, img=img, label=label, size=size, out=out, taps=taps, torch32=_torch_sample(fmap, pts, img, size, torch.float32))
    return _CACHE[i]


# ------------------------------------------------------------------------------------------------ the exact fma
def _fma_exact(a, b, c):
    """fp32(a * b + c) by rational arithmetic: the nearer of the two fp32 neighbours of the exact value, ties to the even one."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    r = F32(float(exact))                      # within an ulp or so of the answer: walk to the neighbours that bracket the exact value
    while Fraction(float(r)) > exact:
        r = np.nextafter(r, F32(-np.inf))
    hi = np.nextafter(r, F32(np.inf))          # r <= exact < hi
    d_lo, d_hi = exact - Fraction(float(r)), Fraction(float(hi)) - exact
    if d_lo != d_hi:
        return r if d_lo < d_hi else hi
    return r if (int(r.view(np.uint32)) & 1) == 0 else hi


def test_fma32_is_one_rounding():
    """3000 random triples plus triples built so that fp64(a * b + c) is an fp32 tie the exact sum is not (where rounding twice goes wrong):
    a * b = 1 + 2^-24 exactly (24929 * 673 = 2^24 + 1), the midpoint of two fp32 neighbours, and c = +-2^-60 decides the side."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal(3000).astype(F32)
    b = rng.standard_normal(3000).astype(F32)
    c = (rng.standard_normal(3000) * 10.0 ** rng.integers(-8, 2, 3000)).astype(F32)
    c[::7] = -(a[::7] * b[::7]).astype(F32)               # cancellation: the fma returns the product's own rounding error
    ta = np.array([24929.0, 24929.0, -24929.0, 24929.0 * 3.0], F32)              # 24929 * 673 = 2^24 + 1
    tb = np.array([673.0 * 2.0 ** -24] * 4, F32)
    tc = np.array([2.0 ** -60, -2.0 ** -60, -2.0 ** -60, 2.0 ** -58], F32)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = sr.fma32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(_bits(got), _bits(want))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert not np.array_equal(_bits(twice), _bits(want)), "the triples no longer tell one rounding from two"


# ------------------------------------------------------------------------------------------------ sampling: equality with torch
@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_restatement_equals_torch_grid_sample_bit_for_bit(i):
    c = _case(i)
    assert c["out"].dtype == F32 and c["out"].shape == (sr.NUM_POINTS, sr.SAMPLE_MAPS[i][1])
    bad = np.nonzero((_bits(c["out"]) != _bits(c["torch32"])).any(1))[0]
    assert bad.size == 0, f"{bad.size} points differ from torch, the first: {c['pts'][bad[0]]} (class {c['label'][bad[0]]})"


def test_restatement_equals_the_reference_fixture_bit_for_bit():
    g = load_golden("points_sample_pca")
    fmap = g["fmap"][None]
    for pts, want in ((g["filtered_disc"], g["sampled_grid"]), (g["offgrid_points"], g["sampled_offgrid"])):
        got, _ = sr.sample_bilinear(fmap, pts, None, (518, 518))
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_points_with_no_tap_on_the_map_give_plus_zero(i):
    c = _case(i)
    out_rows = ~c["taps"].valid.any(1)
    assert int(out_rows.sum()) >= sr.MIN_PER_CLASS
    assert not _bits(c["out"][out_rows]).any(), "a row with all four taps outside is not +0.0 in every channel"


# ------------------------------------------------------------------------------------------------ sampling: distance from fp64
def _fp64_bound(c, i):
    """What |fp32 restatement - fp64 grid_sample| of a point may be, [P] fp64, u = 2^-24.

    Coordinates.  sx = 2 / img_w and ux = sx * px carry one rounding each: |d ux| <= 2 u |ux| (1 + u).  ux - 1 and the + 1 behind it round once
    each: u |ux - 1| and u |u1|.  ix = fma(u1, W / 2, -0.5) rounds once: u |ix|.  So
        dx = (W / 2) u (2 |ux| + |ux - 1| + |u1|) (1 + 2 u) + u |ix|,   and dy alike.
    The sampled value is a continuous, piecewise bilinear function of (ix, iy) over the map padded with zeros -- also across a cell border, where
    fp32 and fp64 may pick different taps -- whose slope along x is at most Gx, the largest difference of two horizontal neighbours of the
    PADDED map (a border value against the 0 beside it included), and Gy along y.  A shifted coordinate moves it by at most Gx dx + Gy dy.
    Weights and sum.  w = ix - floor(ix) is exact; e = 1 - w rounds once (<= u, e <= 1); a product of two such factors carries
    |d(s e)| <= 3 u (1 + u).  The sum is one multiplication and three fmas: a relative error of at most gamma_4 on every term.  With M the
    largest magnitude of the map and weights that sum to one: 4 * 3 u M + gamma_4 M <= 17 u M.
    The fp64 side's own roundings are 2^-29 of these."""
    B, C, H, W, img_w, img_h = sr.SAMPLE_MAPS[i]
    f = c["fmap"].astype(np.float64)
    pad = np.pad(f, ((0, 0), (0, 0), (1, 1), (1, 1)))
    gx, gy, m = np.abs(np.diff(pad, axis=3)).max(), np.abs(np.diff(pad, axis=2)).max(), np.abs(f).max()

    def shift(u, n, idx):
        u = u.astype(np.float64)
        return (n / 2.0) * U * (3 * np.abs(u) + np.abs(u - 1.0)) * (1 + 2 * U) + U * (np.abs(idx) + 1.0)      # (|u1| <= |ux| (1 + 2 u); |ix| <= |x0| + 1)

    t = c["taps"]
    dx, dy = shift(t.ux, W, t.x0.astype(np.float64)), shift(t.uy, H, t.y0.astype(np.float64))
    return gx * dx + gy * dy + 17 * U * m, (gx, gy, m)


@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_restatement_is_within_the_fp32_bound_of_fp64_grid_sample(i):
    """A second witness that does not depend on torch's fp32 rounding order.  Measured (largest distance over the points with a tap on the map
    / its bound there), maps in the order of sampling_ref.SAMPLE_MAPS: 1.100e-05 / 1.065e-04, 4.721e-06 / 4.735e-05, 7.868e-06 / 5.047e-05,
    7.887e-08 / 1.103e-06, 2.980e-05 / 2.147e-04; the largest err / bound of a point is 0.14, 0.12, 0.16, 0.07, 0.15."""
    c = _case(i)
    ref = _torch_sample(c["fmap"], c["pts"], c["img"], c["size"], torch.float64)
    bound, (gx, gy, m) = _fp64_bound(c, i)
    err = np.abs(c["out"].astype(np.float64) - ref).max(1)
    near = c["taps"].valid.any(1)
    worst = int(np.argmax(np.where(near, err / bound, 0.0)))
    print(f"sampling/fp64 map {sr.SAMPLE_MAPS[i]}: max |fp32 - fp64| = {err[near].max():.3e}, bound there {bound[np.argmax(np.where(near, err, 0))]:.3e}, "
          f"max err / bound = {err[worst] / bound[worst]:.4f} (Gx {gx:.2f}, Gy {gy:.2f}, M {m:.2f})")
    assert bool((err <= bound).all()), f"point {c['pts'][worst]} is {err[worst] / bound[worst]:.3f} x its bound away from the fp64 sample"
    assert err[near].max() > 0.0        # (fp32 really is a different computation: the bound is not met by comparing fp64 with itself)


# ------------------------------------------------------------------------------------------------ sampling: the table holds its classes
@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_point_table_holds_every_class(i):
    B, C, H, W, img_w, img_h = sr.SAMPLE_MAPS[i]
    c = _case(i)
    pts, label, taps = c["pts"], c["label"], c["taps"]
    assert pts.shape == (sr.NUM_POINTS, 2) and pts.dtype == F32 and sr.NUM_POINTS % 4 != 0 and bool(np.isfinite(pts).all())
    assert (c["img"] is None) == (B == 1)
    if B > 1:
        assert c["img"].dtype == np.int32 and set(np.unique(c["img"])) == set(range(B))
    k = sr.classify(taps, H, W)
    need = sr.MIN_PER_CLASS
    count = {name: int(mask.sum()) for name, mask in k.items()}
    print(f"sampling/classes map {sr.SAMPLE_MAPS[i]}: {count}, made as {dict(zip(*np.unique(label, return_counts=True)))}")
    for cls in sr.CLASSES:
        assert int((label == cls).sum()) >= need, f"class ({cls}): fewer than {need} points made"
    assert int((k["a"] & (label == "a")).sum()) >= need                                     # (a) cell centres land on weights exactly 0 and 1
    for axis in ("x", "y"):                                                                 # (b), (c): one side, the other side, the corner
        assert count["b" + axis] >= need and count["c" + axis] >= need
    assert int((k["bx"] & k["by"]).sum()) >= need and int((k["cx"] & k["cy"]).sum()) >= need
    if H > 1 and W > 1:      # an edge that is not a corner: the other axis has both taps on the map
        inner_x, inner_y = (taps.x0 >= 0) & (taps.x0 < W - 1), (taps.y0 >= 0) & (taps.y0 < H - 1)
        for m_, inner in ((k["bx"], inner_y), (k["by"], inner_x), (k["cx"], inner_y), (k["cy"], inner_x)):
            assert int((m_ & inner).sum()) >= need
    else:
        assert not bool(taps.valid.all(1).any()), "a one-cell map: every point has a tap outside"
    assert int((k["bx"] & k["by"] & (taps.valid.sum(1) == 1)).sum()) >= need                # a corner: three taps outside
    assert count["all_out"] >= need and min(count["d_left"], count["d_right"], count["d_up"], count["d_down"]) >= 2     # (d)
    assert count["d_left"] + count["d_right"] + count["d_up"] + count["d_down"] >= need
    exact = {(0.0, 0.0), (float(img_w), float(img_h)), (img_w / 2.0, img_h / 2.0), (0.5, 0.5), (0.0, float(img_h)), (float(img_w), 0.0)}   # (e)
    have = {(float(x), float(y)) for x, y in pts[label == "e"]}
    assert exact <= have
    far = np.abs(pts[label == "f"])                                                         # (f)
    assert bool((far.max(1) == 1.0e6).all()) and int((far.min(1) == 1.0e6).sum()) >= 4
    assert bool(taps.valid[label == "g"].all()) or min(H, W) == 1                           # (g) interior: all four taps on the map
    assert count["round_trip"] >= sr.MIN_ROUND_TRIP, "too few points notice a coordinate chain without the round trip through -1, +1"


# ------------------------------------------------------------------------------------------------ sampling: the table discriminates
def _applies(i, wrong):
    B, C, H, W, img_w, img_h = sr.SAMPLE_MAPS[i]
    if H * W == 1:
        return False                              # the one-cell map is the trivial one: a single value, nothing to order or to swap
    if wrong == "swap_image":
        return img_w != img_h
    if wrong == "swap_map":
        return H != W
    return True


WRONG_CASES = [(i, w) for w in sr.WRONG for i in MAPS if _applies(i, w)]


@pytest.mark.parametrize("i,wrong", WRONG_CASES, ids=[f"{w}-{MAP_IDS[i]}" for i, w in WRONG_CASES])
def test_point_table_tells_a_wrong_sampler_from_torch(i, wrong):
    """u1 = ux; img_w and img_h swapped; W and H swapped; x1 <= W for x1 < W; the fma chain over nw, sw, ne, se; align_corners=True."""
    c = _case(i)
    got, _ = sr.sample_bilinear(c["fmap"], c["pts"], c["img"], c["size"], wrong=wrong)
    differ = (_bits(got) != _bits(c["torch32"])).any(1)
    print(f"sampling/wrong {wrong} map {sr.SAMPLE_MAPS[i]}: {int(differ.sum())} of {sr.NUM_POINTS} points differ from torch")
    assert bool(differ.any()), f"the point table cannot tell '{wrong}' from torch on map {sr.SAMPLE_MAPS[i]}"


def test_wrong_variants_cover_the_non_square_map():
    assert {w for i, w in WRONG_CASES if sr.SAMPLE_MAPS[i][2] != sr.SAMPLE_MAPS[i][3]} == set(sr.WRONG)
    assert len({i for i, w in WRONG_CASES}) == len(MAPS) - 1


# ------------------------------------------------------------------------------------------------ PCA
@pytest.mark.parametrize("shape,with_mean", sr.PCA_CASES, ids=[f"{'x'.join(map(str, s))}-{'mean' if m else 'nomean'}" for s, m in sr.PCA_CASES])
def test_pca_restatement_within_the_forward_bound_of_fp64(shape, with_mean):
    """|out - (X - mu) C^T| <= gamma_{D+1} (sum |x_k c_k| + sum |mu_k c_k|) + u |result|: two chains of D fmas (gamma_D each, the +1 covers the
    bound's own fp64 evaluation) and the one rounding of the difference."""
    n, D, d = shape
    x, comps, mean = sr.pca_case(shape, with_mean)
    assert x.shape == (n, D) and comps.shape == (d, D) and (mean is None) == (not with_mean)
    got = sr.pca_project(x, comps, mean)
    assert got.dtype == F32 and got.shape == (n, d)
    x64, c64 = x.astype(np.float64), comps.astype(np.float64)
    m64 = np.zeros(D) if mean is None else mean.astype(np.float64)
    ref = (x64 - m64) @ c64.T
    bound = sr.gamma(D + 1) * (np.abs(x64) @ np.abs(c64).T + np.abs(m64) @ np.abs(c64).T) + U * np.abs(ref)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"pca/fp64 {shape} mean {with_mean}: max err / bound = {ratio:.4f}")
    assert ratio <= 1.0
    if with_mean:       # the case cancels: what is subtracted is of the size of what is left (a forgotten or doubled mean is far outside the bound)
        sub = float(np.abs(m64 @ c64.T).mean())
        assert sub > 0.5 * float(np.abs(ref).mean()) and sub > 100.0 * float(bound.max())
        assert np.array_equal(got, (sr.chain_matrix(x, comps) - sr.chain_matrix(mean[None], comps)).astype(F32))


def test_pca_chain_is_the_k_ascending_fmaf_chain():
    """chain_matrix against fma32 applied k by k (both operand orders of the product: the chain does not depend on it)."""
    x, comps, _ = sr.pca_case((133, 36, 100), False)
    acc = np.zeros((133, 100), F32)
    for k in range(36):
        acc = sr.fma32(x[:, k:k + 1], comps[None, :, k], acc)
    assert np.array_equal(_bits(sr.chain_matrix(x, comps)), _bits(acc))


# ------------------------------------------------------------------------------------------------ row norms
@pytest.mark.parametrize("shape", sr.SQNORM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sqnorm_oracle_within_the_forward_bound_of_fp64(shape):
    x = sr.sqnorm_case(shape)
    got = clib.sqnorm(x)
    ref = (x.astype(np.float64) ** 2).sum(1)
    assert got.dtype == F32 and got.shape == (shape[0],)
    assert bool((np.abs(got - ref) <= sr.gamma(shape[1]) * ref).all())          # d fmas of non-negative terms


@pytest.mark.parametrize("shape", sr.NORMALIZE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_normalize_oracle_bound_and_special_rows(shape):
    """Ordinary rows: x / (sqrt(S (1 + t)) (1 + d1)) (1 + d2) with |t| <= gamma_d (the chain), |d1|, |d2| <= u (square root and division, both
    correctly rounded): within (gamma_d / 2 + 2 u) (1 + gamma_d) of x / |x|; asserted with gamma_d + 3 u.  Special rows: exact."""
    n, d = shape
    x, rows = sr.normalize_case(shape)
    assert sorted(rows.values()) == list(range(min(n, 4))) and list(rows) == list(sr.SPECIAL_ROWS[:min(n, 4)])
    with np.errstate(over="ignore", invalid="raise", divide="raise"):
        got = om.l2_normalize_rows(x, sr.EPS)
    assert got.dtype == F32 and got.shape == x.shape and bool(np.isfinite(got).all())
    eps32 = F32(sr.EPS)
    want_one = np.zeros(d, F32)
    want_one[d - 1] = -1.0
    assert np.array_equal(got[rows["one"]], want_one)
    if "zero" in rows:
        assert not got[rows["zero"]].any()
    if "tiny" in rows:
        r = rows["tiny"]
        assert float(np.sqrt((x[r].astype(np.float64) ** 2).sum())) < sr.EPS and bool((x[r] != 0).all())
        assert np.array_equal(got[r], (x[r] / eps32).astype(F32))
    if "huge" in rows:
        r = rows["huge"]
        with np.errstate(over="ignore"):
            assert np.isinf(clib.sqnorm(x[r:r + 1])[0]) and bool(np.isfinite(x[r]).all())
        assert not got[r].any()                                                 # x / max(sqrt(inf), eps) = x / inf = 0
    plain = np.arange(n) >= len(rows)
    if plain.any():
        x64 = x[plain].astype(np.float64)
        ref = x64 / np.maximum(np.sqrt((x64 ** 2).sum(1, keepdims=True)), sr.EPS)
        assert bool((np.abs(got[plain] - ref) <= (sr.gamma(d) + 3 * U) * np.abs(ref)).all())
