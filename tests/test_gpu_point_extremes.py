"""GPU: fp_pts_diameter and fp_directed_hausdorff (csrc/point_extremes.hip) against their numpy restatement (tests/models_info_ref.py) bit for
bit, at the sizes where the kernels take another path -- one point, a wave, the workgroup's 256 threads, the query block and LDS tile of 1 024,
more than two of each; exact cases on an integer lattice; one larger set against scipy; and the refusals."""

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import models_info_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)
STRIDES = (1, 3, 7)
K_MAX = 70


def _rot(rng):
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _tf(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _dev_diameter(pts):
    d, pair = ops.pts_diameter(torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda())
    return float(d.cpu()[0]), tuple(int(x) for x in pair.cpu())


def _dev_hausdorff(pts, tfs, stride=1):
    h, arg = ops.directed_hausdorff(torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda(),
                                    torch.from_numpy(np.ascontiguousarray(tfs, np.float64).reshape(-1, 12)).cuda(), stride)
    return h.cpu().numpy(), arg.cpu().numpy()


@pytest.fixture(scope="module")
def clouds():
    """Per size a blob and 70 rigid transforms near and far from the identity; the restatement's values per (size, stride), computed once."""
    rng = np.random.default_rng(26)
    out = {}
    for V in SIZES:
        pts = rng.normal(size=(V, 3)) * 40.0 + np.array([13.0, -7.0, 21.0])
        tfs = []
        for k in range(K_MAX):
            R = _rot(rng)
            if k % 2:   # a small turn: the nearest neighbour of most points is their own counterpart
                a = rng.normal(size=3) * 0.02
                R = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            tfs.append(_tf(R, rng.normal(size=3) * (2.0 if k % 2 else 30.0)))
        tfs = np.stack(tfs)
        want = {}
        for s in STRIDES:
            h, arg = ref.batch_hausdorff(pts, tfs, s)
            h.setflags(write=False), arg.setflags(write=False)
            want[s] = (h, arg)
        out[V] = {"pts": pts, "tfs": tfs, "want": want, "diameter": ref.diameter(pts)}
    return out


# ---------------------------------------------------------------------------------------------------------------- diameter
def test_diameter_equals_the_restatement_bit_for_bit(clouds):
    for V in SIZES:
        d, pair = _dev_diameter(clouds[V]["pts"])
        wd, wpair = clouds[V]["diameter"]
        print(V, "device", d, pair, "restatement", wd, wpair)
        assert _bits(d) == _bits(wd) and pair == wpair, f"V = {V}"
        assert pair[0] < pair[1] or V == 1
    assert _dev_diameter(clouds[1]["pts"]) == (0.0, (0, 0))


def _lattice(n=7, spacing=16.0, shift=(48.0, 16.0, 80.0)):
    g = (np.arange(n, dtype=np.float64) - (n - 1) / 2) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(shift)   # centre = shift


def test_diameter_ties_go_to_the_lowest_pair_and_a_nan_never_wins():
    pts = _lattice()                         # the four body diagonals tie; (0, 342) is the lowest pair
    d, pair = _dev_diameter(pts)
    assert pair == (0, 342) and d == float(np.sqrt(np.float64(3 * 96.0 * 96.0)))
    assert (d, pair) == ref.diameter(pts)
    big = np.tile(pts, (4, 1))               # 1 372 points in two tiles: every pair's copies tie across tile pairs
    assert _dev_diameter(big) == ref.diameter(big) and _dev_diameter(big)[1] == (0, 342)
    bad = pts.copy()
    bad[0] = np.nan
    bad[200, 1] = np.nan
    d, pair = _dev_diameter(bad)
    assert (d, pair) == ref.diameter(bad) and np.isfinite(d) and 0 not in pair and 200 not in pair
    same = np.tile(np.array([[1.0, 2.0, 3.0]]), (300, 1))
    assert _dev_diameter(same) == (0.0, (0, 0)) == ref.diameter(same)


def test_a_larger_set_agrees_with_pdist():
    from scipy.spatial.distance import pdist
    pts = np.random.default_rng(3).normal(size=(5000, 3)) * 50.0
    d, pair = _dev_diameter(pts)
    want = pdist(pts).max()
    print("device", d, pair, "pdist", want)
    assert abs(d - want) <= 1e-9 * want
    assert abs(np.linalg.norm(pts[pair[0]] - pts[pair[1]]) - want) <= 1e-9 * want


# ---------------------------------------------------------------------------------------------------------------- Hausdorff
def test_hausdorff_batches_equal_the_restatement_bit_for_bit(clouds):
    for V in SIZES:
        c = clouds[V]
        for s in STRIDES:                    # 3 and 7 exceed V = 1 and V = 2: the one query is vertex 0
            wh, warg = c["want"][s]
            for K in sorted({1, 3, len(wh)}):
                h, arg = _dev_hausdorff(c["pts"], c["tfs"][:K], s)
                assert np.array_equal(_bits(h), _bits(wh[:K])) and np.array_equal(arg, warg[:K]), f"V = {V}, stride {s}, K = {K}"
                assert np.all(arg % s == 0) and np.all(arg < V)
            if V == 2049 and s == 3:
                print("V 2049 stride 3: device", h[:4].tolist(), arg[:4].tolist(), "restatement", wh[:4].tolist(), warg[:4].tolist())


def test_the_reversed_batch_and_each_candidate_alone_give_the_same_bits(clouds):
    for V in SIZES:
        c = clouds[V]
        for s in STRIDES:
            wh, warg = c["want"][s]
            K = len(wh)
            h, arg = _dev_hausdorff(c["pts"], c["tfs"][:K][::-1].copy(), s)
            assert np.array_equal(_bits(h), _bits(wh[::-1])) and np.array_equal(arg, warg[::-1]), f"V = {V}, stride {s} reversed"
            for k in (0, 1, 2, K - 1):
                h, arg = _dev_hausdorff(c["pts"], c["tfs"][k:k + 1], s)
                assert _bits(h)[0] == _bits(wh)[k] and arg[0] == warg[k], f"V = {V}, stride {s}, candidate {k} alone"


def test_a_query_subset_gives_a_lower_bound(clouds):
    for V in SIZES:
        h1 = clouds[V]["want"][1][0]
        for s in STRIDES[1:]:
            assert np.all(clouds[V]["want"][s][0][:len(h1)] <= h1)
            h, _ = _dev_hausdorff(clouds[V]["pts"], clouds[V]["tfs"], s)
            full, _ = _dev_hausdorff(clouds[V]["pts"], clouds[V]["tfs"], 1)
            assert np.all(h <= full), f"V = {V}, stride {s}"


# ---- exact cases: an integer lattice of spacing 16, signed-permutation rotations and integer translations, so every operation is exact
R_PERM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])          # a signed permutation, det +1
HALF_TURN_Z = np.diag([-1.0, -1.0, 1.0])


def test_a_lattice_symmetry_gives_zero_and_a_short_translation_its_length():
    pts = _lattice()
    c = np.array([48.0, 16.0, 80.0])
    tfs = np.stack([_tf(R_PERM, c - R_PERM @ c), _tf(np.eye(3), [3.0, -4.0, 0.0]), _tf(HALF_TURN_Z, c - HALF_TURN_Z @ c)])
    for s in (1, 2):
        h, arg = _dev_hausdorff(pts, tfs, s)
        assert h.tolist() == [0.0, 5.0, 0.0] and arg.tolist() == [0, 0, 0]      # every query ties: the lowest
        assert np.array_equal(_bits(h), _bits(ref.batch_hausdorff(pts, tfs, s)[0]))


def test_one_outlier_gives_its_distance_and_its_index():
    c = np.array([48.0, 16.0, 80.0])
    pts = np.insert(_lattice(), 100, c + np.array([148.0, 0.0, 0.0]), axis=0)    # 100 beyond the lattice face at +48
    tf = _tf(HALF_TURN_Z, c - HALF_TURN_Z @ c)                                 # the lattice onto itself; the outlier to c - (148, 0, 0)
    h, arg = _dev_hausdorff(pts, tf[None], 1)
    assert h.tolist() == [100.0] and arg.tolist() == [100]
    h, arg = _dev_hausdorff(pts, tf[None], 100)                                # queries 0, 100, 200, 300
    assert h.tolist() == [100.0] and arg.tolist() == [100]
    h, arg = _dev_hausdorff(pts, tf[None], 3)                                  # the outlier is not queried
    assert h.tolist() == [0.0] and arg.tolist() == [0]
    nan_tf = tf.copy()
    nan_tf[9] = np.nan                                                         # a NaN query has no nearest neighbour: +inf, as the restatement
    h, arg = _dev_hausdorff(pts, nan_tf[None], 1)
    wh, warg = ref.batch_hausdorff(pts, nan_tf[None], 1)
    assert np.array_equal(_bits(h), _bits(wh)) and np.array_equal(arg, warg) and np.isinf(h[0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_ops_refuse_bad_arguments_before_any_launch():
    pts = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    tfs = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    for bad in (pts.cpu(), pts.float(), pts[:, :2], pts[:0], pts.reshape(-1), "pts"):
        with pytest.raises(ValueError):
            ops.pts_diameter(bad)
        with pytest.raises(ValueError):
            ops.directed_hausdorff(bad, tfs)
    for bad in (tfs.cpu(), tfs.float(), tfs[:, :9], tfs[:0], tfs.reshape(-1), None):
        with pytest.raises(ValueError):
            ops.directed_hausdorff(pts, bad)
    for stride in (0, -1, 1.5, True, None, 2**31):
        with pytest.raises(ValueError):
            ops.directed_hausdorff(pts, tfs, stride)
    with pytest.raises(ValueError, match="device tensor"):
        ops.directed_hausdorff(pts.cpu(), tfs)


def test_the_library_validates_too_and_writes_nothing():
    pts = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    tfs = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    null = _lib.vp(0)

    def fresh(nbytes):
        return (torch.full((4,), -7.0, dtype=torch.float64, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda"),
                torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda"))

    def untouched(d, i, scratch):
        torch.cuda.synchronize()
        return bool((d == -7.0).all()) and bool((i == -7).all()) and bool((scratch == 0x5A).all())

    for V, nbytes, nulls in ((0, None, ()), (-1, None, ()), (_lib.PTS_DIAMETER_MAX_V + 1, None, ()), (10, 8, ()), (10, None, (0,)), (10, None, (2,)),
                             (10, None, (4,)), (10, None, (5,))):
        d, pair, scratch = fresh(64)
        args = [_lib.ptr(pts), V, _lib.ptr(scratch), scratch.numel() if nbytes is None else nbytes, _lib.ptr(d), _lib.ptr(pair), _lib.stream()]
        for n in nulls:
            args[n] = null
        with pytest.raises(_lib.FoundPoseNativeError, match="fp_pts_diameter"):
            _lib.call("fp_pts_diameter", *args)
        assert untouched(d, pair, scratch)
    for V, stride, K, nbytes, nulls in ((0, 1, 2, None, ()), (10, 0, 2, None, ()), (10, -3, 2, None, ()), (10, 1, 0, None, ()), (10, 1, 65536, None, ()),
                                        (10, 1, 2, 16, ()), (10, 1, 2, None, (0,)), (10, 1, 2, None, (3,)), (10, 1, 2, None, (5,)),
                                        (10, 1, 2, None, (7,)), (10, 1, 2, None, (8,))):
        h, arg, scratch = fresh(64)
        args = [_lib.ptr(pts), V, stride, _lib.ptr(tfs), K, _lib.ptr(scratch), scratch.numel() if nbytes is None else nbytes, _lib.ptr(h), _lib.ptr(arg),
                _lib.stream()]
        for n in nulls:
            args[n] = null
        with pytest.raises(_lib.FoundPoseNativeError, match="fp_directed_hausdorff"):
            _lib.call("fp_directed_hausdorff", *args)
        assert untouched(h, arg, scratch)
    assert _lib.pts_diameter_scratch_bytes(1) == 16 and _lib.pts_diameter_scratch_bytes(2049) == 16 * 6
    assert _lib.pts_hausdorff_scratch_bytes(2049, 1, 70) == 16 * 70 * 3 and _lib.pts_hausdorff_scratch_bytes(2049, 7, 3) == 16 * 3
