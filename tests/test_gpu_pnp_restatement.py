"""fp_pnp_ransac / fp_pnp_ransac_keyed (pnp_util.solve_pnp_ransac_batch) hypothesis by hypothesis against the numpy restatement
(tests/pnp_ref.py); tests/test_pnp_cpu.py builds the same fixtures and asserts their conditions without a GPU (decided, identifiable,
fragile share <= 5 %).

  * sweeps: 2 048 pairs of one scene / 4 096 pairs of four points with one iteration each expose single hypotheses -- the sampler, P3P's
    branches, the fourth-point choice, the count and the mask of each one;
  * replay fixtures: 2 x 3 pairs with two cameras, counts 0, 5, 6, 40 and 57 (clamped), 300 hypotheses at confidence 0.99 and 0.5, with and
    without keys; a winner at h >= 256; k_max = N = 4096 with 4 096 hypotheses -- success, quality and the inlier masks EQUAL to the
    restatement's, the winning hypothesis the predicted one, the refined pose within 1e-6 rad / 1e-3 mm;
  * lm_iters = 0 and every refusal of the C entries, on sentinel-filled outputs.

A raw hypothesis is held to max(1e-6 px, 1000 * delta_h), delta_h being the restatement's own gap between Grunert's formulas and the
polished solution (pnp_ref's docstring); the observed maximum of device error / delta_h is printed by every test that measures it."""

import numpy as np
import pytest
import torch

from tests import pnp_ref as pr

pytestmark = pytest.mark.gpu


def _run(fix, conf=0.99, pair_keys=None, cams=None, refine_lm=True):
    """A fixture through the GPU path -> dict of numpy arrays, pairs flattened."""
    from foundpose_amd import pnp_util
    B, n, K = fix["B"], fix["n_slots"], fix["K"]
    keys = None if pair_keys is None else torch.as_tensor(np.asarray(pair_keys, np.int64).reshape(B, n))
    out = pnp_util.solve_pnp_ransac_batch(
        torch.from_numpy(fix["coord_2d"]).reshape(B, n, K, 2).cuda(), torch.from_numpy(fix["coord_3d"]).reshape(B, n, K, 3).cuda(),
        torch.from_numpy(fix["counts"]).reshape(B, n).cuda(), fix["cams"] if cams is None else cams, fix["iters"], fix["thresh"], conf, refine_lm,
        seed=fix["seed"], return_ransac_pose=True, min_corresp=fix["min_corresp"], pair_keys=keys)
    torch.cuda.synchronize()
    return {k: v.reshape(B * n, *v.shape[2:]).cpu().numpy() for k, v in out.items()}


def _check(bad, fig, what):
    print(f"{what}: device against the predicted winner at most {fig['hyp_px']:.3e} px, max device error / max(1e-9 px, delta_h) = {fig['hyp_ratio']:.3g} "
          f"(1000 allowed), every other visited hypothesis >= {fig['min_gap_ratio']:.3g} times farther; refined pose {fig['rad']:.3e} rad / {fig['mm']:.3e} mm")
    assert not bad, f"{len(bad)} mismatches, the first: {bad[:5]}"


# ------------------------------------------------------------------------------------------------------------------------------ sweeps
def test_hypothesis_sweep():
    fix = pr.sweep_fixture()
    hyps = pr.sweep_hypotheses(fix)
    bad, fig = pr.compare_sweep(_run(fix, pair_keys=fix["pair_keys"]), hyps, fix)
    print(f"hypothesis sweep: {fig['fragile']} of {len(hyps)} hypotheses fragile (the device solved {fig['fragile_solved']} of them, {fig['fragile_unsolved']} "
          f"not), {fig['open']} with the fourth inlier inside the band; {fig['checked']} checked, {fig['models']} of them models; device against the "
          f"exact path at most {fig['hyp_px']:.3e} px, max device error / max(1e-9 px, delta_h) = {fig['hyp_ratio']:.3g} (1000 allowed)")
    assert fig["fragile"] + fig["open"] <= 0.05 * len(hyps)
    assert not bad, f"{len(bad)} mismatches, the first: {bad[:5]}"


def test_four_point_sweep():
    fix = pr.four_point_fixture()
    hyps = pr.four_point_hypotheses(fix)
    bad, fig = pr.compare_four_point(_run(fix), hyps, fix)
    P = len(hyps)
    print(f"four-point sweep: the device fails {fig['device_failed']} of {P} pairs ({fig['device_failed'] / P:.2e}), the restatement calls {fig['fragile']} "
          f"fragile ({fig['fragile'] / P:.2e}); non-fragile pairs re-project to at most {fig['worst_px']:.3e} px, device against the exact path at "
          f"most {fig['hyp_px']:.3e} px, max device error / max(1e-9 px, delta_h) = {fig['hyp_ratio']:.3g} (1000 allowed)")
    assert fig["fragile"] <= 0.05 * P
    assert not bad, f"{len(bad)} mismatches, the first: {bad[:5]}"


# ------------------------------------------------------------------------------------------------------------------- replay fixtures
@pytest.fixture(scope="module")
def replay_fix():
    return pr.replay_fixture()


@pytest.mark.parametrize("keyed", [False, True])
def test_replay_fixture_equals_the_restatement(replay_fix, keyed):
    fix, cache = replay_fix, {}
    keys = pr.REPLAY_KEYS if keyed else None
    for conf in (0.99, 0.5):
        ref = pr.run_ref_on(fix, conf, keys, cache=cache)
        assert pr.fixture_conditions(fix, ref) == []
        dev = _run(fix, conf, keys)
        _check(*pr.compare(dev, ref, fix["coord_2d"], fix["coord_3d"], fix["counts"], fix["cams"], fix["n_slots"]),
               f"replay fixture, keyed {keyed}, confidence {conf}")
        for p in np.nonzero(ref["success"])[0]:
            assert abs(np.linalg.det(dev["R"][p]) - 1.0) < 1e-12 and np.abs(dev["R"][p] @ dev["R"][p].T - np.eye(3)).max() < 1e-12
    # the camera is the detection's: with the two swapped every solved pair changes, and a restatement left on the old cameras notices
    swapped = _run(fix, 0.5, keys, cams=fix["cams"][::-1])
    for p in np.nonzero(ref["success"])[0]:
        assert not np.array_equal(swapped["ransac_pose"][p], dev["ransac_pose"][p])
    assert pr.compare(swapped, ref, fix["coord_2d"], fix["coord_3d"], fix["counts"], fix["cams"], fix["n_slots"])[0]


def test_late_winner():
    fix = pr.late_winner_fixture()
    ref = pr.run_ref_on(fix)
    assert pr.fixture_conditions(fix, ref, gap_factor=2.0) == [] and ref["best_h"][0] >= 256
    # (noise-free inliers: later all-inlier triples give the winner's pose to ~1e-5 px, so the winner is the nearest one, within its band,
    # but not 1e3 times nearer -- pnp_ref.late_winner_fixture)
    _check(*pr.compare(_run(fix), ref, fix["coord_2d"], fix["coord_3d"], fix["counts"], fix["cams"], 1, identify=False), "late winner")


def test_lds_limit():
    fix = pr.lds_fixture()
    ref = pr.run_ref_on(fix, pair_keys=pr.LDS_KEYS)
    assert pr.fixture_conditions(fix, ref) == []
    _check(*pr.compare(_run(fix, pair_keys=pr.LDS_KEYS), ref, fix["coord_2d"], fix["coord_3d"], fix["counts"], fix["cams"], 1), "LDS limit")


# ---------------------------------------------------------------------------------------------------------------------- the C entries
def _entry_args(fix, sentinel=False):
    dev = "cuda"
    P, K = fix["coord_2d"].shape[:2]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    ins = dict(c2=t(fix["coord_2d"], torch.float32), c3=t(fix["coord_3d"], torch.float32), cnt=t(fix["counts"], torch.int32),
               cam=t(fix["cams"], torch.float64))
    fill = (lambda shape, dt, v: torch.full(shape, v if sentinel else 0, dtype=dt, device=dev))
    outs = dict(success=fill((P,), torch.int32, 9), R=fill((P, 9), torch.float64, 7.5), t=fill((P, 3), torch.float64, -3.25),
                ninl=fill((P,), torch.int32, 77), mask=fill((P, K), torch.uint8, 5), rp=fill((P, 12), torch.float64, 1.5))
    return ins, outs


def test_without_lm_the_output_is_the_winning_hypothesis(replay_fix):
    from foundpose_amd._lib import call, ptr, stream
    fix = replay_fix
    ins, o = _entry_args(fix)
    call("fp_pnp_ransac", ptr(ins["c2"]), ptr(ins["c3"]), ptr(ins["cnt"]), ptr(ins["cam"]), 6, 3, fix["K"], fix["iters"], fix["thresh"], 0.99, 0, 6,
         fix["seed"], ptr(o["success"]), ptr(o["R"]), ptr(o["t"]), ptr(o["ninl"]), ptr(o["mask"]), ptr(o["rp"]), stream())
    torch.cuda.synchronize()
    assert o["success"].cpu().tolist() == [1, 0, 0, 1, 1, 0]
    for p in (0, 3, 4):
        assert torch.equal(o["R"][p], o["rp"][p, :9]) and torch.equal(o["t"][p], o["rp"][p, 9:])
    # and the refinement does move it
    full = _run(fix)
    for p in (0, 3, 4):
        assert np.array_equal(full["ransac_pose"][p], o["rp"][p].cpu().numpy()) and not np.array_equal(full["R"][p].reshape(9), full["ransac_pose"][p][:9])


def test_bad_arguments_raise_before_anything_is_written(replay_fix):
    from foundpose_amd import _lib
    from foundpose_amd._lib import call, ptr, stream
    fix = replay_fix
    ins, o = _entry_args(fix, sentinel=True)
    before = {k: v.clone() for k, v in o.items()}
    keys = torch.arange(6, dtype=torch.int64, device="cuda")
    good = dict(num_pairs=6, n_slots=3, k_max=fix["K"], iters=fix["iters"], thresh=fix["thresh"], conf=0.99, lm_iters=40, min_corresp=6)
    ptr_names = ("c2", "c3", "cnt", "cam", "success", "R", "t", "ninl", "mask")

    def go(entry="fp_pnp_ransac", null=None, key_ptr=None, **kw):
        a = dict(good, **kw)
        pp = {k: ptr(None if k == null else {**ins, **o}[k]) for k in ptr_names + ("rp",)}
        key_arg = () if entry == "fp_pnp_ransac" else (ptr(keys) if key_ptr is None else key_ptr,)
        call(entry, pp["c2"], pp["c3"], pp["cnt"], pp["cam"], *key_arg, a["num_pairs"], a["n_slots"], a["k_max"], a["iters"], a["thresh"], a["conf"],
             a["lm_iters"], a["min_corresp"], fix["seed"], pp["success"], pp["R"], pp["t"], pp["ninl"], pp["mask"], pp["rp"], stream())

    launch, entry_ = "pnp_ransac: ", "{entry}: "     # launch_pnp_ransac's refusals name the stage, the entry's own name the entry
    cases = [(dict(k_max=3), launch + r"k_max must be in \[4, 4096\] \(got 3\)"), (dict(k_max=4097), launch + r"k_max must be in \[4, 4096\] \(got 4097\)"),
             (dict(iters=0), launch + r"iterations must be in \[1, 4096\] \(got 0\)"), (dict(iters=4097), launch + r"iterations must be in \[1, 4096\] \(got 4097\)"),
             (dict(thresh=0.0), launch + "bad threshold / confidence"), (dict(thresh=-1.0), launch + "bad threshold / confidence"),
             (dict(conf=0.0), launch + "bad threshold / confidence"), (dict(conf=1.5), launch + "bad threshold / confidence"),
             (dict(min_corresp=3), launch + "bad lm_iters / n_slots / min_corresp"), (dict(lm_iters=-1), launch + "bad lm_iters / n_slots / min_corresp"),
             (dict(n_slots=0), entry_ + "num_pairs must be a multiple of n_slots"), (dict(num_pairs=5), entry_ + "num_pairs must be a multiple of n_slots"),
             (dict(num_pairs=-3), entry_ + "num_pairs must be a multiple of n_slots")]
    cases += [(dict(null=name), entry_ + "null pointer") for name in ptr_names]
    for entry in ("fp_pnp_ransac", "fp_pnp_ransac_keyed"):
        for kw, msg in cases:
            with pytest.raises(_lib.FoundPoseNativeError, match=r"\): " + msg.format(entry=entry) + "$"):
                go(entry, **kw)
    with pytest.raises(_lib.FoundPoseNativeError, match="fp_pnp_ransac_keyed: null pair_keys"):
        go("fp_pnp_ransac_keyed", key_ptr=ptr(None))
    for entry in ("fp_pnp_ransac", "fp_pnp_ransac_keyed"):      # nothing to do is not an error -- and still nothing is written
        go(entry, num_pairs=0)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert torch.equal(v, before[k]), k
    # the same buffers through an accepted call: all of them are written (the sentinels were in the way of nothing)
    go("fp_pnp_ransac_keyed")
    torch.cuda.synchronize()
    assert o["success"].cpu().tolist() == [1, 0, 0, 1, 1, 0] and int(o["mask"].max()) == 1 and not torch.equal(o["rp"], before["rp"])
