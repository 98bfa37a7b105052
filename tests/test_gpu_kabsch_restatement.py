"""fp_kabsch_ransac (pnp_util.solve_kabsch_ransac_batch) hypothesis by hypothesis against the numpy restatement (tests/kabsch_ref.py), at
sizes where the kernel's loops stride and every wave holds data; tests/test_kabsch_cpu.py builds the same fixtures and asserts their
conditions without a GPU.

  * sweeps: 4 096 pairs of one scene (K = 48, eight model points exactly collinear) and 2 048 pairs of a scene with 8 valid
    correspondences among 256, one iteration each, expose single hypotheses -- the sampler and its limit of 1 + 64 draws, the gate, the
    exactly degenerate triangle, the count and the mask of each one;
  * the replay at K = 700 (counts 700, 300, 257 | 64, 757 clamped, 700 with 70 % outliers; 1 024 hypotheses; confidence 0.99 and 0.5;
    with and without keys): better hypotheses beyond the shrunken budget, ties a whole millimetre apart, budgets that shrink in steps;
  * a winner at h >= 256; k_max = N = 4096 with 4 096 hypotheses (120 KB of LDS, every lane in both block reductions);
  * the lift on exact rounding ties, the image border, NaN pixels and depths of 0, -1, NaN and +inf, against a hand-written list;
  * the refit on six inliers, a coplanar model, the identity, half-turns and coordinates of 5 m;
  * every refusal of the C entry, on sentinel-filled outputs.

success, num_valid, quality and the masks must be EQUAL to the restatement's, the winning hypothesis within 1e-9 rad / 1e-6 mm, the refit
within 1e-6 rad / 1e-3 mm, R a rotation to 1e-12 (kabsch_ref.compare); every test prints its observed maxima."""

import numpy as np
import pytest
import torch

from tests import kabsch_ref as kr

pytestmark = pytest.mark.gpu


def _run(fix, conf=0.99, refit=True, pair_keys=None):
    """A fixture through the GPU path -> dict of numpy arrays, pairs flattened."""
    from foundpose_amd import pnp_util
    B, n, K = len(fix["solve"]), fix["n_slots"], fix["K"]
    keys = None if pair_keys is None else torch.as_tensor(np.asarray(pair_keys, np.int64).reshape(B, n))
    out = pnp_util.solve_kabsch_ransac_batch(
        torch.from_numpy(fix["coord_2d"]).reshape(B, n, K, 2).cuda(), torch.from_numpy(fix["coord_3d"]).reshape(B, n, K, 3).cuda(),
        torch.from_numpy(fix["counts"]).reshape(B, n).cuda(), fix["solve"], fix["frames"], torch.from_numpy(fix["depth"]).cuda(), fix["image_index"],
        fix["tau"], fix["iters"], conf, refit, fix["seed"], return_ransac_pose=True, pair_keys=keys)
    torch.cuda.synchronize()
    return {k: v.reshape(B * n, *v.shape[2:]).cpu().numpy() for k, v in out.items()}


def _check(dev, ref, what, refit=True):
    bad, fig = kr.compare(dev, ref, refit)
    print(f"{what}: min_margin {ref['min_margin']:.3e}; {kr.figures(fig)}")
    assert not bad, f"{len(bad)} mismatches, the first: {bad[:5]}"
    return fig


# ------------------------------------------------------------------------------------------------------------------------------ sweeps
def test_hypothesis_sweep():
    fix = kr.sweep_fixture()
    ref = kr.run_ref_on(fix, False, fix["pair_keys"], cache={})
    assert kr.sweep_conditions(fix, ref) == []
    print(f"hypothesis sweep, {len(ref['success'])} hypotheses by what decided them: {kr.sweep_classes(ref)}")
    _check(_run(fix, refit=False, pair_keys=fix["pair_keys"]), ref, "hypothesis sweep", refit=False)


def test_sparse_validity_sweep():
    fix = kr.sparse_fixture()
    ref = kr.run_ref_on(fix, False, fix["pair_keys"], cache={})
    assert kr.sparse_conditions(fix, ref) == []
    print(f"sparse-validity sweep, {len(ref['success'])} hypotheses: {kr.sparse_classes(ref)}")
    _check(_run(fix, refit=False, pair_keys=fix["pair_keys"]), ref, "sparse-validity sweep", refit=False)


# --------------------------------------------------------------------------------------------------------------------------- the replay
@pytest.fixture(scope="module")
def stride():
    fix = kr.stride_fixture()
    return fix, kr.stride_refs(fix)


def test_the_stride_fixture_meets_its_conditions(stride):
    fix, refs = stride
    assert kr.stride_conditions(fix, refs) == []
    facts = kr.stride_facts(fix, refs)
    print("replay at sizes that stride, (confidence, keyed, pair, ...): better hypotheses beyond the budget", facts["beyond"], "; ties whole mm away",
          [(c, k, p, h, round(d, 2)) for c, k, p, h, d in facts["ties"]], "; budgets shrinking in >= 3 steps", facts["shrinks"])


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("conf", kr.STRIDE_CONFS)
def test_replay_at_sizes_that_stride(stride, conf, keyed):
    fix, refs = stride
    keys = kr.STRIDE_KEYS if keyed else None
    dev = _run(fix, conf, pair_keys=keys)
    _check(dev, refs[(conf, keyed)], f"replay at sizes that stride, confidence {conf}, keyed {keyed}")
    # the comparison notices: a restatement left on the other confidence, or on the other keys, disagrees with the device
    other_conf = kr.STRIDE_CONFS[1 - kr.STRIDE_CONFS.index(conf)]
    assert kr.compare(dev, refs[(other_conf, keyed)])[0]
    assert kr.compare(dev, refs[(conf, not keyed)])[0]


def test_late_winner():
    fix = kr.late_winner_fixture()
    ref = kr.run_ref_on(fix)
    assert kr.late_conditions(fix, ref) == []
    print(f"late winner: best_h = {ref['best_h'][0]} (lane {ref['best_h'][0] % 256}), {ref['quality'][0]} inliers of {ref['num_valid'][0]}")
    _check(_run(fix), ref, "late winner")


def test_the_limits():
    fix = kr.limit_fixture()
    ref = kr.run_ref_on(fix)
    assert kr.limit_conditions(fix, ref) == []
    _check(_run(fix), ref, "k_max = N = 4096, 4 096 hypotheses")


# ----------------------------------------------------------------------------------------------------------------------- the lift's edges
def test_lift_edges_exact():
    fix = kr.edge_fixture()
    ref = kr.run_ref_on(fix)
    assert kr.edge_conditions(fix, ref) == []
    dev = _run(fix)
    # the hand-written list first: which pixel was read shows in the mask (kabsch_ref.edge_fixture)
    assert int(dev["num_valid"][0]) == sum(kr.EDGE_VALID) == 21
    assert dev["inliers"][0].astype(int).tolist() == kr.EDGE_INLIER
    assert dev["success"][0] and dev["quality"][0] == sum(kr.EDGE_INLIER) == 20
    _check(dev, ref, "lift edges")


# ------------------------------------------------------------------------------------------------------------------ the refit's conditioning
def test_refit_conditioning():
    fix = kr.conditioning_fixture()
    ref = kr.run_ref_on(fix)
    assert kr.conditioning_conditions(fix, ref) == []
    dev = _run(fix)
    for p, name in enumerate(kr.COND_NAMES):
        R = dev["R"][p]
        print(f"  {name}: eig_gap {ref['eig_gap'][p]:.3f}, {ref['quality'][p]} inliers, refit {kr.rotation_angle(R, ref['R'][p]):.3e} rad / "
              f"{np.abs(dev['t'][p] - ref['t'][p]).max():.3e} mm, |det R - 1| {abs(np.linalg.det(R) - 1.0):.3e}, |R R^T - I| {np.abs(R @ R.T - np.eye(3)).max():.3e}")
    _check(dev, ref, "refit conditioning")


# ------------------------------------------------------------------------------------------------------------------------- the C entry
def test_bad_arguments_raise_before_anything_is_written():
    from foundpose_amd import _lib
    from foundpose_amd._lib import call, ptr, stream
    fix = kr.gpu_fixture()
    n, K, dev = fix["n_slots"], fix["K"], "cuda"
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    ins = dict(c2=t(fix["coord_2d"], torch.float32), c3=t(fix["coord_3d"], torch.float32), cnt=t(fix["counts"], torch.int32),
               cam=t([kr.camera_tuple(c) for c in fix["solve"]], torch.float64), fcam=t([kr.camera_tuple(c) for c in fix["frames"]], torch.float64),
               A=t(fix["A"].reshape(2, 9), torch.float64), iid=t(fix["image_index"], torch.int32), tau=t(fix["tau"], torch.float64),
               depth=t(fix["depth"], torch.float32))
    fill = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)
    o = dict(success=fill((6,), torch.int32, 9), R=fill((6, 9), torch.float64, 7.5), t=fill((6, 3), torch.float64, -3.25), ninl=fill((6,), torch.int32, 77),
             nval=fill((6,), torch.int32, 55), mask=fill((6, K), torch.uint8, 5), rp=fill((6, 12), torch.float64, 1.5))
    before = {k: v.clone() for k, v in o.items()}
    keys = torch.arange(6, dtype=torch.int64, device=dev)
    good = dict(num_images=2, H=48, W=64, num_pairs=6, n_slots=n, k_max=K, iters=fix["iters"], conf=0.99, min_corresp=6)
    required = ("c2", "c3", "cnt", "cam", "fcam", "A", "iid", "tau", "depth", "success", "R", "t", "ninl", "nval", "mask")

    def go(null=None, **kw):
        a = dict(good, **kw)
        pp = {k: ptr(None if k == null else v) for k, v in {**ins, **o, "keys": keys}.items()}
        call("fp_kabsch_ransac", pp["c2"], pp["c3"], pp["cnt"], pp["cam"], pp["fcam"], pp["A"], pp["iid"], pp["tau"], pp["depth"], a["num_images"], a["H"],
             a["W"], pp["keys"], a["num_pairs"], a["n_slots"], a["k_max"], a["iters"], a["conf"], 1, a["min_corresp"], fix["seed"], pp["success"], pp["R"],
             pp["t"], pp["ninl"], pp["nval"], pp["mask"], pp["rp"], stream())

    launch, entry = "kabsch_ransac: ", "fp_kabsch_ransac: "    # launch_kabsch_ransac's refusals name the stage, the entry's own name the entry
    multiple = entry + "num_pairs must be a multiple of n_slots"
    cases = [(dict(k_max=2), launch + r"k_max must be in \[3, 4096\] \(got 2\)"), (dict(k_max=4097), launch + r"k_max must be in \[3, 4096\] \(got 4097\)"),
             (dict(iters=0), launch + r"iterations must be in \[1, 4096\] \(got 0\)"), (dict(iters=4097), launch + r"iterations must be in \[1, 4096\] \(got 4097\)"),
             (dict(conf=0.0), launch + "bad confidence"), (dict(conf=1.5), launch + "bad confidence"), (dict(conf=float("nan")), launch + "bad confidence"),
             (dict(min_corresp=2), launch + "bad n_slots / min_corresp"),
             (dict(n_slots=0), multiple), (dict(num_pairs=5), multiple), (dict(num_pairs=-3), multiple),
             (dict(num_images=0), launch + r"0 depth images of 64 x 48"), (dict(H=0), launch + r"2 depth images of 64 x 0"),
             (dict(W=0), launch + r"2 depth images of 0 x 48")]
    cases += [(dict(null=name), entry + "null pointer") for name in required]
    for kw, msg in cases:
        with pytest.raises(_lib.FoundPoseNativeError, match=r"\): " + msg + "$"):
            go(**kw)
    go(num_pairs=0)      # nothing to do is not an error -- and still nothing is written
    torch.cuda.synchronize()
    for k, v in o.items():
        assert torch.equal(v, before[k]), k
    # the same buffers through an accepted call, without the two optional pointers first: all of them are written
    go(null="keys")
    torch.cuda.synchronize()
    assert o["success"].cpu().tolist() == [1, 0, 0, 1, 0, 1] and int(o["mask"].max()) == 1 and not torch.equal(o["rp"], before["rp"])
    for k, v in o.items():
        assert not (v == before[k]).any(), k     # no element kept its sentinel
    first = {k: v.clone() for k, v in o.items()}
    for k, v in o.items():
        v.copy_(before[k])
    go(null="rp")        # out_ransac_pose is optional: it stays as it was, the rest is what the first call wrote
    torch.cuda.synchronize()
    assert torch.equal(o["rp"], before["rp"])
    for k in ("success", "R", "t", "ninl", "nval", "mask"):
        assert torch.equal(o[k], first[k]), k
