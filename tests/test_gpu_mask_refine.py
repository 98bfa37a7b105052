"""GPU: the silhouette refinement (csrc/mask_refine.hip: refine_util.mask_contours, refine_util.refine_mask)
against the numpy restatement tests/mask_refine_ref.py on the fixtures of tests/mask_refine_steps.py, whose margins
tests/test_mask_refine_cpu.py asserts: N = 70 (three chunks, the last ragged) and N = one more than the contour pass's LDS tile,
K' = 5 (skipped), 6, 33 and 70."""

import numpy as np
import pytest
import torch

from foundpose_amd import ops, refine_util
from tests import lm_ref, lm_steps
from tests import mask_refine_ref as mr
from tests import mask_refine_steps as ms
from tests.test_gpu_mask_distance import SIZES, _contents

pytestmark = pytest.mark.gpu


def _cuda(a, dt=None):
    return torch.as_tensor(np.array(a), dtype=dt).cuda()      # a copy: some fixtures are read-only


def _run(dets, iters=30, normal_eq=False):
    """dets: list of dict(X, R, t, cam, mask, delta, K_max, has_pose=True), one image size and delta -> refine_mask's dict (cpu numpy).
    Each detection's contour rows are made with its own cap."""
    X = np.concatenate([d["X"] for d in dets]).astype(np.float32)
    n = np.array([len(d["X"]) for d in dets])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    masks = _cuda(np.stack([d["mask"] for d in dets]))
    rows, kb, at = [], [], 0
    for i, d in enumerate(dets):
        r, _, e = refine_util.mask_contours(masks[i:i + 1], d["K_max"])
        rows.append(r)
        kb.append((at, at + int(e[0])))
        at += int(e[0])
    kb = np.array(kb).reshape(-1, 2)
    assert len({d["delta"] for d in dets}) == 1
    out = refine_util.refine_mask(
        ops.mask_distance(masks), torch.cat(rows), _cuda(kb[:, 0], torch.int32), _cuda(kb[:, 1], torch.int32), [d["cam"] for d in dets],
        _cuda(np.stack([d["R"] for d in dets]), torch.float64), _cuda(np.stack([d["t"] for d in dets]), torch.float64), _cuda(rb, torch.int32),
        _cuda(rb + n, torch.int32), _cuda(X), _cuda(np.array([d.get("has_pose", True) for d in dets])), dets[0]["delta"], iters=iters,
        return_normal_equations=normal_eq)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(d, iters):
    return mr.refine(d["R"], d["t"], np.asarray(d["X"], np.float32).astype(np.float64), d["cam"], d["mask"], d["delta"], iters, d["K_max"], d.get("has_pose", True))


def _pose_gap(Ra, ta, Rb, tb):
    c = (np.trace(np.asarray(Ra) @ np.asarray(Rb).T) - 1.0) / 2.0
    s = np.linalg.norm(np.asarray(Ra) - np.asarray(Rb)) / np.sqrt(2.0)      # |dR|_F / sqrt 2: the angle for small turns, without arccos near 1
    return (s if c > 0.999 else float(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(np.asarray(ta) - np.asarray(tb)))


def _same_bits(a, b, i, j):
    return all(np.array_equal(a[k][i], b[k][j], equal_nan=True) for k in ("R", "t", "cost_in", "cost_out", "num_points", "iters_used", "status"))


# ---------------------------------------------------------------------------------------------------- contour rows
@pytest.mark.parametrize("H,W", SIZES)
def test_contour_rows_equal_the_restatement(H, W):
    masks = np.stack([m for _, m in _contents(H, W)])
    for cap in (16, 100000):
        rows, begin, end = refine_util.mask_contours(_cuda(masks), cap)
        assert rows.dtype == torch.int32 and begin.dtype == torch.int32 and end.dtype == torch.int32 and rows.is_cuda
        rows, begin, end = rows.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy()
        at = 0
        for i, m in enumerate(masks):
            ref = mr.contour_rows(m, cap)
            assert begin[i] == at and end[i] == at + len(ref) and np.array_equal(rows[begin[i]:end[i]], ref), (cap, i)
            at += len(ref)
        assert at == len(rows)
    if H * W > 1000:
        assert max(len(mr.contour_pixels(m)) for m in masks) > 16       # the cap of 16 subsamples here


def test_contour_rows_of_the_planted_masks():
    for size, cap in (("small", 6), ("small", 33), ("small", 70), ("large", 1024)):
        m = ms.planted_mask(size)
        rows, begin, end = refine_util.mask_contours(_cuda(m[None]), cap)
        assert np.array_equal(rows.cpu().numpy(), mr.contour_rows(m, cap)) and (int(begin[0]), int(end[0])) == (0, min(cap, len(mr.contour_pixels(m))))


# ---------------------------------------------------------------------------------------------------- the system and the steps
def test_normal_equations_and_cost_at_the_input_pose():
    """1e-9 of the largest entry per block: the bar of tests/test_gpu_depth_refine.py, for its reason -- both sides compute in fp64 from
    the same integers and differ in summation order only."""
    dets = [ms.fixture(n).det for n in ms.IDS]
    out = _run(dets, iters=0, normal_eq=True)
    for i, name in enumerate(ms.IDS):
        fx = ms.fixture(name)
        d = fx.det
        ref = mr.normal_equations(d["R"], d["t"], np.asarray(d["X"], np.float32).astype(np.float64), d["cam"], fx.d2, fx.q, d["delta"])
        got = out["normal_eq"][i]
        for blk in (slice(0, 21), slice(21, 27)):
            assert np.abs(got[blk] - ref[blk]).max() <= 1e-9 * np.abs(ref[blk]).max(), (name, blk)
        assert abs(got[27] - ref[27]) <= 1e-9 * ref[27] and abs(out["cost_in"][i] - ref[27]) <= 1e-9 * ref[27]
        assert out["cost_in"][i] == out["cost_out"][i] == got[27] and out["status"][i] == 1 and out["iters_used"][i] == 0
        assert out["num_points"][i] == len(d["X"])
        assert np.array_equal(out["R"][i], d["R"]) and np.array_equal(out["t"][i], d["t"])


def test_the_accept_reject_sequence_over_the_pinned_prefix():
    """The four fixtures as one batch at iters = 1 .. K: after k iterations the kernel stands where the restatement stands, and has moved
    exactly where the restatement accepted."""
    fxs = [ms.fixture(n) for n in ms.IDS]
    pre = [ms.prefix(fx) for fx in fxs]
    Ks = [min(p[0], lm_steps.K_MAX) for p in pre]
    prev = _run([fx.det for fx in fxs], iters=0)
    got = ["" for _ in fxs]
    for k in range(1, max(Ks) + 1):
        out = _run([fx.det for fx in fxs], iters=k)
        for i, fx in enumerate(fxs):
            if k > Ks[i]:
                continue
            rec = pre[i][1]["trace"][k - 1]
            moved = not (np.array_equal(out["R"][i], prev["R"][i]) and np.array_equal(out["t"][i], prev["t"][i]))
            assert moved == (out["cost_out"][i] < prev["cost_out"][i])
            got[i] += "a" if moved else "r"
            dr_, dt_ = _pose_gap(out["R"][i], out["t"][i], rec["R"], rec["t"])
            assert dr_ < lm_steps.POSE_RAD and dt_ < lm_steps.POSE_MM, (fx, k, dr_, dt_)
            assert out["iters_used"][i] == k and out["status"][i] == (0 if "acc" in [r["kind"] for r in pre[i][1]["trace"][:k]] else 1), (fx, k)
            assert out["cost_out"][i] <= out["cost_in"][i]
        prev = out
    for i, fx in enumerate(fxs):
        assert got[i] == lm_ref.decisions(pre[i][1]["trace"][:Ks[i]]), fx
    assert any("r" in g for g in got)


def test_alone_in_the_batch_and_in_the_reversed_batch_the_same_bits():
    five = dict(ms.fixture("n70_k6").det, K_max=5)           # K' = 5: skipped
    dets = [ms.fixture(n).det for n in ms.IDS] + [five]
    batch = _run(dets, iters=12, normal_eq=True)
    rev = _run(dets[::-1], iters=12, normal_eq=True)
    for i, d in enumerate(dets):
        alone = _run([d], iters=12, normal_eq=True)
        assert _same_bits(alone, batch, 0, i) and _same_bits(rev, batch, len(dets) - 1 - i, i), i
        assert np.array_equal(alone["normal_eq"][0], batch["normal_eq"][i]) and np.array_equal(rev["normal_eq"][len(dets) - 1 - i], batch["normal_eq"][i])
    assert batch["status"].tolist() == [0, 0, 0, 0, 2]
    assert np.array_equal(batch["R"][4], five["R"]) and np.array_equal(batch["t"][4], five["t"]) and batch["iters_used"][4] == 0


# ---------------------------------------------------------------------------------------------------- edge cases
def test_edge_cases():
    base = ms.fixture("n70_k70").det
    H, W = base["mask"].shape
    # the object partly outside the image: planted 26 px to the right, its mask cut off by the border
    t_out = np.array(ms.SMALL["t"]) + np.array([26.0 * 400.0 / 120.0, 0.0, 0.0])
    cut = mr.splat_mask(ms.R_TRUE, t_out, ms.dense_points(), base["cam"], H, W)
    assert cut[:, W - 1].any() and 0 < cut.sum() < ms.planted_mask("small").sum()
    outside = dict(base, mask=cut, R=base["R"], t=base["t"] + (t_out - np.array(ms.SMALL["t"])))
    cases = {"nopose": dict(base, has_pose=False), "empty": dict(base, mask=np.zeros((H, W), np.uint8)), "ones": dict(base, mask=np.ones((H, W), np.uint8)),
             "outside": outside, "behind": dict(base, t=-np.asarray(base["t"])), "fine": base}
    names = list(cases)
    out = _run([cases[n] for n in names], iters=10)
    refs = {n: _ref(cases[n], 10) for n in names}
    want = {"nopose": 2, "empty": 2, "ones": 2, "behind": 2, "fine": 0, "outside": 0}
    for i, n in enumerate(names):
        assert out["status"][i] == refs[n]["status"] == want[n], n
        assert out["cost_out"][i] <= out["cost_in"][i] or np.isnan(out["cost_in"][i]), n
        if want[n]:
            assert np.array_equal(out["R"][i], cases[n]["R"]) and np.array_equal(out["t"][i], cases[n]["t"]) and out["iters_used"][i] == 0, n
    assert out["cost_in"][names.index("behind")] == np.inf == refs["behind"]["cost_in"] and out["num_points"][names.index("behind")] == 0
    assert out["cost_in"][0] == out["cost_in"][1] == out["cost_in"][2] == 0.0
    i = names.index("outside")
    assert 6 <= out["num_points"][i] == refs["outside"]["num_points"] < len(base["X"])        # the part of the model outside the image is ignored
    assert abs(out["cost_in"][i] - refs["outside"]["cost_in"]) <= 1e-9 * refs["outside"]["cost_in"] and out["cost_out"][i] < out["cost_in"][i]
    zero = _run([base], iters=0)
    assert zero["status"][0] == 1 and zero["cost_in"][0] == zero["cost_out"][0] > 0 and np.array_equal(zero["R"][0], base["R"]) and np.array_equal(zero["t"][0], base["t"])


def test_what_is_refused():
    d = ms.fixture("n70_k6").det
    masks = _cuda(d["mask"][None])
    rows, b, e = refine_util.mask_contours(masks, 6)
    args = lambda **kw: dict(dict(d2=ops.mask_distance(masks), contour=rows, contour_begin=b, contour_end=e, cameras=[d["cam"]], R=_cuda(d["R"][None]),
                                  t=_cuda(d["t"][None]), row_begin=_cuda([0], torch.int32), row_end=_cuda([70], torch.int32), vertices=_cuda(d["X"]),
                                  has_pose=_cuda([True]), huber_px=4.0, iters=3), **kw)
    assert refine_util.refine_mask(**args())["status"].tolist() == [0]
    for kw in (dict(huber_px=0.0), dict(huber_px=float("nan")), dict(iters=-1), dict(iters=1001), dict(d2=masks), dict(cameras=[d["cam"]] * 2)):
        with pytest.raises(ValueError):
            refine_util.refine_mask(**args(**kw))
    from foundpose_amd._lib import FoundPoseNativeError
    with pytest.raises(FoundPoseNativeError, match="contour rows"):     # a contour range outside the rows is reported, never read
        refine_util.refine_mask(**args(contour_end=_cuda([7], torch.int32), max_contour=7))
    with pytest.raises(FoundPoseNativeError, match="bank rows"):
        refine_util.refine_mask(**args(row_end=_cuda([71], torch.int32), max_points=71))
    with pytest.raises(ValueError):
        refine_util.mask_contours(masks, 0)


# ---------------------------------------------------------------------------------------------------- recovery
def test_recovery_from_the_sideways_start():
    """One of the four starts of tests/test_mask_refine_cpu.py on the device, at 144 x 192 with 4 000 points and the contour cap 1024:
    the same three ordering conditions."""
    X, mask, _, _ = ms.recovery_problem()
    _, R0, t0, _ = ms.recovery_starts()[0]
    out = _run([dict(X=X, R=R0, t=t0, cam=ms.LARGE["cam"], mask=mask, delta=8.0, K_max=1024)], iters=30)
    assert out["status"][0] == 0 and out["cost_out"][0] < out["cost_in"][0]
    s = ms.recovery_scores(R0, t0, out["R"][0], out["t"][0])
    print(f"sideways on the device: cost {out['cost_in'][0]:.4f} -> {out['cost_out'][0]:.4f}, IoU {s['iou_in']:.3f} -> {s['iou_out']:.3f}, "
          f"lateral {s['lat_in']:.2f} -> {s['lat_out']:.2f} mm")
    assert s["iou_out"] > s["iou_in"] and s["lat_out"] < s["lat_in"]
