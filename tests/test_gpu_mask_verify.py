"""fp_pose_verify_mask (pnp_util.verify_poses_mask) against its numpy restatement (tests/mask_verify_ref.py) on the smallest batch that
reaches every path: the blob fixture of tests/pose_verify_ref.py -- 2 detections of 2 objects x 3 slots, 600 and 602 sampled points (one
object sampled with stride 2: more than two rounds of the 256-thread point loop), a 48 x 64 image -- with each detection's mask the
silhouette of a dense splat of its planted pose, G = 16; slots: the planted pose, a pose shifted sideways by rho / 2, a pose moved along
the ray to 0.7 x its distance, success false, a planted pose partly outside the image, C.z <= rho + 1; A = I and a rotated A.  The
fixture is far from every decision boundary (min_margin, asserted on the CPU too), every output is an integer count or the fp64 quotient
of two of them, so counts, status and score must be EQUAL, bit for bit; and the same bits alone, in the batch and in the reversed batch.

Measured on an MI355X (G = 16, seed 6): the planted poses' IoU is 0.9008 (881 / 978) and, partly outside the image, 0.8953 (667 / 745);
the shifted pose 0.4159, the scaled one 0.4522 -- the restatement's figures, which the GPU's equal."""

import numpy as np
import pytest
import torch

from tests import mask_verify_ref as mv
from tests import pose_verify_ref as pv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return mv.gpu_fixture()


@pytest.fixture(scope="module")
def ref(fix):
    out = mv.run_ref_on(fix)
    assert out["min_margin"] > 1e-6
    return out


@pytest.fixture(scope="module")
def bank(fix):
    return pv.make_bank(fix)


def _run(fix, bank, pairs=None, masks=None, solve=None, det_obj=None, grid=None, min_pixels=16):
    """The fixture's pairs through the GPU path.  pairs: [[pair, ...], ...], one row per detection of the launch, every row's pairs of one
    fixture detection (default: the fixture as it is).  masks: the fixture's [2, H, W] replaced.  -> dict of numpy arrays, pairs flattened
    in launch order."""
    from foundpose_amd import pnp_util
    n = fix["n_slots"]
    pairs = [list(range(d * n, (d + 1) * n)) for d in range(2)] if pairs is None else pairs
    dets = [row[0] // n for row in pairs]
    sel = np.array(pairs)
    dev = "cuda"
    poses = {"success": torch.from_numpy(fix["success"][sel]).to(dev), "R": torch.from_numpy(fix["R"][sel]).to(dev), "t": torch.from_numpy(fix["t"][sel]).to(dev)}
    m = fix["masks"] if masks is None else masks
    out = pnp_util.verify_poses_mask(
        poses, bank, [fix["det_obj"][d] for d in dets] if det_obj is None else det_obj, [fix["solve"][d] for d in dets] if solve is None else solve,
        [fix["frames"][d] for d in dets], torch.from_numpy(np.ascontiguousarray(m[dets])).to(dev), max_points=fix["max_points"],
        grid=fix["grid"] if grid is None else grid, min_pixels=min_pixels)
    torch.cuda.synchronize()
    assert out["counts"].dtype == torch.int32 and out["status"].dtype == torch.int32 and out["score"].dtype == torch.float64
    return {k: v.reshape(sel.size, *v.shape[2:]).cpu().numpy() for k, v in out.items()}


def _assert_equal(out, want):
    assert np.array_equal(out["counts"], want["counts"])
    assert np.array_equal(out["status"], want["status"])
    assert np.array_equal(out["score"].view(np.int64), want["score"].view(np.int64))   # the same division of the same integers


def test_matches_the_restatement(fix, ref, bank):
    out = _run(fix, bank)
    print("counts (n_both, n_model_only, n_mask_only, n_cells) per pair, GPU:", out["counts"].tolist(), "restatement:", ref["counts"].tolist())
    print("score GPU:", out["score"].tolist(), "restatement:", ref["score"].tolist(), "status GPU:", out["status"].tolist())
    # an ordering, on the restatement first: the planted pose beats the shifted and the scaled one
    assert ref["score"][0] > ref["score"][1] and ref["score"][0] > ref["score"][2]
    _assert_equal(out, ref)
    assert out["score"][0] > out["score"][1] and out["score"][0] > out["score"][2]
    few = _run(fix, bank, min_pixels=2000)   # status 1: the counts are reported, the score is 0
    assert few["status"].tolist() == [1, 1, 1, 2, 1, 2] and not few["score"].any() and np.array_equal(few["counts"], ref["counts"])
    _assert_equal(few, mv.run_ref_on(fix, min_pixels=2000))


def test_the_largest_grid_matches_the_restatement():
    """G = 128, the upper bound the host accepts: 512 words of bitmap, cells a third of a pixel wide -- most pixels' cells hold no point of
    a 600-point sample (the IoU falls to about 0.1: DESIGN.md section 18, limit 3), and every pixel's cell index is far from the clamp's
    reach.  Another seed, whose min_margin at this grid is 2.6e-6."""
    big = mv.gpu_fixture(seed=7, grid=128)
    want = mv.run_ref_on(big)
    assert want["min_margin"] > 1e-6
    out = _run(big, pv.make_bank(big))
    print("G = 128 counts, GPU:", out["counts"].tolist(), "restatement:", want["counts"].tolist())
    _assert_equal(out, want)


def test_alone_in_the_batch_and_reversed_are_the_same_bits(fix, bank):
    n = fix["n_slots"]
    both = _run(fix, bank)
    rev = _run(fix, bank, pairs=[list(range(2 * n - 1, n - 1, -1)), list(range(n - 1, -1, -1))])
    for k, v in both.items():
        assert np.array_equal(v, rev[k][::-1]), k
    for p in range(2 * n):
        alone = _run(fix, bank, pairs=[[p]])
        for k, v in alone.items():
            assert np.array_equal(v[0], both[k][p]), (p, k)


def test_an_empty_and_a_full_mask(fix, ref, bank):
    for value in (0, 1, 255):
        masks = np.full_like(fix["masks"], value)
        want = mv.run_ref_on(fix, masks=masks)
        out = _run(fix, bank, masks=masks)
        _assert_equal(out, want)
        assert np.array_equal(out["counts"][:, 3], ref["counts"][:, 3])   # the bitmap does not depend on the mask
        scored = want["status"] == 0
        if value == 0:
            assert not out["counts"][:, [0, 2]].any() and not out["score"].any() and scored.sum() == 4
        else:   # every model pixel is in the mask; what remains of the 48 x 64 image is mask only
            assert not out["counts"][:, 1].any() and np.array_equal(out["counts"][scored][:, [0, 2]].sum(1), np.full(4, 48 * 64))


def test_bad_arguments_raise_before_anything_is_launched(fix, bank, monkeypatch):
    from foundpose_amd import crop_util, pnp_util
    launched = []
    real = pnp_util.call
    monkeypatch.setattr(pnp_util, "call", lambda *a: (launched.append(a[0]), real(*a))[1])
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="outside the bank's"):
            _run(fix, bank, det_obj=bad)
    crop = fix["solve"][1]
    Ts = crop.T_world_from_eye.copy()
    Ts[:3, 3] += (0.5, 0.0, 0.0)
    moved = crop_util.PinholePlaneCameraModel(crop.width, crop.height, crop.f, crop.c, Ts)
    with pytest.raises(ValueError, match="mask verification needs cameras that share their centre"):
        _run(fix, bank, solve=[fix["solve"][0], moved])
    for bad in (7, 129, 16.0):
        with pytest.raises(ValueError, match="grid"):
            _run(fix, bank, grid=bad)
    with pytest.raises(ValueError, match="min_pixels"):
        _run(fix, bank, min_pixels=0)
    dev = "cuda"
    poses = {"success": torch.from_numpy(fix["success"].reshape(2, 3)).to(dev), "R": torch.from_numpy(fix["R"].reshape(2, 3, 3, 3)).to(dev),
             "t": torch.from_numpy(fix["t"].reshape(2, 3, 3)).to(dev)}
    m = torch.from_numpy(fix["masks"])
    for bad, msg in ((m, "on the device"), (m.to(dev).float(), "uint8"), (m.to(dev)[0], "uint8"), (m.to(dev)[:1], "for 2 detections")):
        with pytest.raises(ValueError, match=msg):
            pnp_util.verify_poses_mask(poses, bank, fix["det_obj"], fix["solve"], fix["frames"], bad)
    for shape in ((0, 3), (2, 0)):   # no detection / no slot: empty tensors
        B, n = shape
        empty = {"success": torch.zeros(B, n, dtype=torch.bool, device=dev), "R": torch.zeros(B, n, 3, 3, dtype=torch.float64, device=dev),
                 "t": torch.zeros(B, n, 3, dtype=torch.float64, device=dev)}
        out = pnp_util.verify_poses_mask(empty, bank, fix["det_obj"][:B], fix["solve"][:B], fix["frames"][:B], m.to(dev)[:B])
        assert tuple(out["counts"].shape) == (B, n, 4) and tuple(out["score"].shape) == (B, n) and tuple(out["status"].shape) == (B, n)
    assert launched == []
    _run(fix, bank, grid=8)
    assert launched == ["fp_pose_verify_mask"]


def test_the_c_entry_refuses_a_bad_grid_and_a_ragged_batch(fix, ref, bank):
    from foundpose_amd import _lib
    from foundpose_amd._lib import call, ptr, stream
    n, dev = fix["n_slots"], "cuda"
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    vp = bank.verify_points(fix["max_points"])
    ok, R, tt = t(fix["success"], torch.int32), t(fix["R"].reshape(6, 9), torch.float64), t(fix["t"], torch.float64)
    cam, A = t([mv.camera_tuple(c) for c in fix["frames"]], torch.float64), t(fix["A"].reshape(2, 9), torch.float64)
    rng, cen, rad = t([vp.ranges[o] for o in fix["det_obj"]], torch.int32), t(vp.centers, torch.float64), t(vp.radii, torch.float64)
    masks = t(fix["masks"], torch.uint8)
    area = masks.ne(0).flatten(1).sum(1, dtype=torch.int32)
    counts = torch.full((6, 4), 9, dtype=torch.int32, device=dev)
    score = torch.full((6,), 9.0, dtype=torch.float64, device=dev)
    status = torch.full((6,), 9, dtype=torch.int32, device=dev)
    args = lambda pairs, grid: (ptr(ok), ptr(R), ptr(tt), ptr(cam), ptr(A), ptr(rng), ptr(cen), ptr(rad), ptr(vp.points), int(vp.points.shape[0]),
                                ptr(masks), ptr(area), 48, 64, pairs, n, grid, 16, ptr(counts), ptr(score), ptr(status), stream())
    call("fp_pose_verify_mask", *args(6, fix["grid"]))
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), ref["counts"]) and np.array_equal(status.cpu().numpy(), ref["status"])
    assert np.array_equal(score.cpu().numpy().view(np.int64), ref["score"].view(np.int64))
    for a, msg in (((6, 7), "grid"), ((6, 129), "grid"), ((5, 16), "multiple of n_slots")):
        with pytest.raises(_lib.FoundPoseNativeError, match=msg):
            call("fp_pose_verify_mask", *args(*a))
