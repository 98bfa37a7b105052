"""GPU: fp_pose_add_errors (csrc/pose_add.hip) against its numpy restatement (tests/pose_add_ref.py) bit for bit, at the sizes where the kernel
takes another path -- one point, the sum tile of 256, the LDS tile and the query block of 1024, more than two of each -- in one ragged batch,
pair by pair and in the reversed batch; exact cases on an integer lattice; one larger pair against scipy's k-d tree; and the refusals."""

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import pose_add_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)


def _rot(rng):
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()])


def _device(pts, est, gt, ranges):
    return ops.pose_add_errors(torch.from_numpy(pts).cuda(), torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda(), ranges).cpu().numpy()


@pytest.fixture(scope="module")
def ragged():
    """One pair per size, each with its own blob, a GT pose and an estimate a few mm and degrees off; the restatement's errors, computed once."""
    rng = np.random.default_rng(11)
    pts, est, gt, ranges = [], [], [], []
    off = 0
    for M in SIZES:
        pts.append(rng.normal(size=(M, 3)) * 40.0)
        Rg, tg = _rot(rng), np.array([rng.uniform(-100, 100), rng.uniform(-100, 100), rng.uniform(600, 1200)])
        a = rng.normal(size=3) * 0.05
        dR = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])   # not a rotation exactly: the kernel does not care
        est.append(_pose(dR @ Rg, tg + rng.normal(size=3) * 4.0))
        gt.append(_pose(Rg, tg))
        ranges.append((off, M))
        off += M
    d = {"pts": np.concatenate(pts), "est": np.stack(est), "gt": np.stack(gt), "ranges": np.array(ranges, np.int64)}
    d["want"] = ref.batch_errors(d["pts"], d["est"], d["gt"], d["ranges"])
    d["want"].setflags(write=False)
    return d


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_ragged_batch_equals_the_restatement_bit_for_bit(ragged):
    got = _device(ragged["pts"], ragged["est"], ragged["gt"], ragged["ranges"])
    print("device", got.tolist(), "restatement", ragged["want"].tolist())
    assert np.all(np.isfinite(got)) and np.all(got[:, 1] <= got[:, 0]) and np.all(got[:, 1] > 0)
    assert np.array_equal(_bits(got), _bits(ragged["want"]))


def test_each_pair_alone_and_the_reversed_batch_give_the_same_bits(ragged):
    want = _bits(ragged["want"])
    for h in range(len(SIZES)):
        alone = _device(ragged["pts"], ragged["est"][h:h + 1], ragged["gt"][h:h + 1], ragged["ranges"][h:h + 1])
        assert np.array_equal(_bits(alone), want[h:h + 1]), f"pair {h} (M = {SIZES[h]}) alone"
    rev = _device(ragged["pts"], ragged["est"][::-1].copy(), ragged["gt"][::-1].copy(), ragged["ranges"][::-1].copy())
    assert np.array_equal(_bits(rev), want[::-1])
    # a pair's points need not start at its object's first point: a sub-range is a pair like any other
    o, c = int(ragged["ranges"][-1][0]) + 3, 1500
    sub = _device(ragged["pts"], ragged["est"][-1:], ragged["gt"][-1:], [(o, c)])
    assert np.array_equal(_bits(sub), _bits(np.array([ref.pair_errors(ragged["pts"][o:o + c], ragged["est"][-1], ragged["gt"][-1])])))


# ---- exact cases: an integer lattice, signed-permutation rotations and integer translations, so every operation is exact
def _lattice():
    g = np.arange(-3, 4, dtype=np.float64) * 16.0
    z = np.arange(0, 7, dtype=np.float64) * 16.0
    return np.stack(np.meshgrid(g, g, z, indexing="ij"), -1).reshape(-1, 3)   # 343 points, symmetric under a half turn about z


R_PERM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])          # a signed permutation, det +1
T_INT = np.array([40.0, -24.0, 800.0])


def test_identical_poses_give_zero():
    pts = _lattice()
    got = _device(pts, _pose(R_PERM, T_INT)[None], _pose(R_PERM, T_INT)[None], [(0, len(pts))])
    assert got.tolist() == [[0.0, 0.0]]


def test_a_short_translation_gives_its_length_for_both():
    pts = _lattice()
    shift = np.array([3.0, -4.0, 0.0])            # |shift| = 5 < 8, half the spacing: every point's nearest neighbour is its own counterpart
    want = float(np.sqrt((shift[0] * shift[0] + shift[1] * shift[1]) + shift[2] * shift[2]))
    got = _device(pts, _pose(R_PERM, T_INT + shift)[None], _pose(R_PERM, T_INT)[None], [(0, len(pts))])
    assert got.tolist() == [[want, want]] and want == 5.0


def test_a_half_turn_of_a_symmetric_lattice_gives_adi_zero_and_add_positive():
    pts = _lattice()
    half_turn = np.diag([-1.0, -1.0, 1.0])
    got = _device(pts, _pose(R_PERM @ half_turn, T_INT)[None], _pose(R_PERM, T_INT)[None], [(0, len(pts))])
    assert got[0, 1] == 0.0 and got[0, 0] > 0
    assert np.array_equal(_bits(got), _bits(np.array([ref.pair_errors(pts, _pose(R_PERM @ half_turn, T_INT), _pose(R_PERM, T_INT))])))


def test_a_larger_pair_agrees_with_the_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    M = 20000
    pts = rng.normal(size=(M, 3)) * 50.0
    Rg, tg = _rot(rng), np.array([10.0, 20.0, 900.0])
    est, gt = _pose(_rot(rng), tg + np.array([2.0, -1.0, 3.0])), _pose(Rg, tg)
    got = _device(pts, est[None], gt[None], [(0, M)])[0]
    E, G = ref.place(est, pts), ref.place(gt, pts)
    d, _ = cKDTree(E).query(G, k=1)
    add = np.linalg.norm(G - E, axis=1).mean()
    print("device", got.tolist(), "k-d tree adi", d.mean(), "numpy add", add)
    assert abs(got[1] - d.mean()) <= 1e-9 * d.mean()
    assert abs(got[0] - add) <= 1e-9 * add


# ---- refusals
def test_bad_tables_are_refused_before_any_launch():
    pts = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    pose = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    for ranges in ([(0, 10), (0, 0)],               # pt_cnt = 0
                   [(0, 10), (5, 6)],               # past V
                   [(0, 10), (-1, 2)],
                   [(0, 10), (0, 2**31)],           # does not fit int32
                   [(0, 10)],                       # one row for two pairs
                   torch.tensor([(0, 10), (0, 10)], device="cuda"),    # a device table
                   np.array([(0.0, 10.0), (0.0, 10.0)])):
        with pytest.raises(ValueError):
            ops.pose_add_errors(pts, pose, pose, ranges)
    with pytest.raises(ValueError):
        ops.pose_add_errors(pts, pose[:0], pose[:0], np.zeros((0, 2), np.int64))     # H = 0
    for bad in ((pts.cpu(), pose, pose), (pts, pose.cpu(), pose), (pts, pose, pose.cpu())):
        with pytest.raises(ValueError, match="device tensor"):
            ops.pose_add_errors(*bad, [(0, 10), (0, 10)])


def test_the_library_validates_too_and_writes_nothing():
    """The C entry point behind ops checks the table itself: a bad one is FP_ERR_INVALID with err and scratch as they were."""
    pts = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    pose = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    for table, nbytes in (([(0, 10), (0, 0)], None), ([(0, 10), (5, 6)], None), ([(0, 10), (-1, 2)], None), ([(0, 10), (0, 10)], 8)):
        r = np.array(table, np.int32)
        err = torch.full((2, 2), -7.0, dtype=torch.float64, device="cuda")
        scratch = torch.full((_lib.pose_add_scratch_bytes(2, 10),), 0x5A, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.FoundPoseNativeError, match="fp_pose_add_errors"):
            _lib.call("fp_pose_add_errors", _lib.ptr(pts), 10, _lib.ptr(pose), _lib.ptr(pose), r.ctypes.data_as(_lib.vp), 2, _lib.ptr(scratch),
                      scratch.numel() if nbytes is None else nbytes, _lib.ptr(err), _lib.stream())
        torch.cuda.synchronize()
        assert bool((err == -7.0).all()) and bool((scratch == 0x5A).all())
    assert _lib.pose_add_scratch_bytes(2, 10) == 32 * 8 + 16 * 2 and _lib.pose_add_scratch_bytes(9, 257) == 32 * 16 + 16 * 9 * 2
