"""GPU: csrc/refine_terms.hpp's Levenberg-Marquardt state machine step by step, through its five entry points (refine_util.refine_depth,
refine_featuremetric, refine_rgbd, ops.tsdf_track without and with colours), against the one restated loop tests/lm_ref.py.

Every fixture of tests/lm_steps.py (70 points: three chunks, the last one ragged; the far starts of feat:edge7 / edge0 leave 58 / 56 valid) is run as K + 1 separate calls with iters = 0 .. K, K
inside the fixture's pinned prefix -- the iterations the restatement itself decides on a clear margin (tests/test_lm_steps_cpu.py checks
that, and that each fault of the accept / reject / stop rules would change what is asserted here).  Per call: iters_used and status
exactly; after a rejected step or a failed factorisation pose and cost bit-identical to the call before; after an accepted step a lower
cost; the pose within 1e-6 (|dR|_F) / 1e-3 mm of the restatement's after the same step; cost_in within 1e-9 relative (the two feature
solvers: 1e-4, their dot products are fp32 -- the bars of the tests at the input pose).  Exact constructions: a normal matrix with a zero
diagonal entry at every lambda (the lambda ceiling), steps the z-bad rule refuses although they lower the cost, and a batch whose four
problems go inactive at different launches.

Measured on an MI355X, the largest distance of a pose from the restatement's over a sweep, |dR|_F / mm:
  depth      edge0 3.0e-14 / 1.5e-11   edge5 1.4e-14 / 7.7e-12   edge2 6.8e-14 / 1.8e-11
  feat       edge7 1.2e-08 / 1.4e-06   edge0 1.7e-08 / 2.0e-06   zbad1 8.3e-10 / 6.2e-08   zbad0 3.4e-10 / 2.9e-08   field0 6.2e-09 / 5.3e-07
  rgbd       edge5_tau25 8.7e-10 / 1.2e-07   zbad1 8.3e-10 / 6.2e-08   edge5_tau15 2.5e-09 / 3.9e-07
  track      blob0 4.4e-14 / 5.8e-13   blob4 1.8e-13 / 2.3e-12
  track_rgb  blob3 4.6e-15 / 6.6e-14   blob4 1.1e-13 / 1.8e-12
(the restatement's own spread under the reversed point order: at most 7.1e-13 / 4.5e-11 mm; prefix lengths, K and seeds are listed in
tests/test_lm_steps_cpu.py); cost_in differs from the restatement's by at most 1e-15 relative (fp64 solvers) and 1.1e-8 (feature solvers).
The trackers' volumes are written by the CPU (tests/tsdf_ref.integrate, or by hand) and uploaded, so both sides read the same planes."""
import numpy as np
import pytest
import torch

from foundpose_amd import ops
from tests import lm_ref
from tests import lm_steps as ls
from tests import test_gpu_depth_refine as gd
from tests import test_gpu_featuremetric as gf
from tests import test_gpu_rgbd_refine as grg
from tests import test_gpu_tsdf_track as gt
from tests import test_gpu_tsdf_track_rgb as gtr

pytestmark = pytest.mark.gpu
COST_TOL = {"depth": 1e-9, "track": 1e-9, "track_rgb": 1e-9, "feat": 1e-4, "rgbd": 1e-4}
assert gd.CAM == ls.DCAM and (gd.H, gd.W) == (ls.DH, ls.DW) and gf.CAM == ls.FCAM and gf.W == grg.W == ls.FW


_DEVICE_VOLUMES = {}


def _device_volume(host):
    """The CPU's planes on the device (once per volume: the fixtures share theirs)."""
    if id(host) not in _DEVICE_VOLUMES:
        vol = ops.tsdf_new_volume(host["origin"], host["voxel_mm"], host["dims"])
        for k in ops.TSDF_PLANES:
            vol[k].copy_(torch.from_numpy(host[k]))
        _DEVICE_VOLUMES[id(host)] = vol
    return _DEVICE_VOLUMES[id(host)]


def _run(fxs, iters):
    """The fixtures (of one entry point; the trackers': of one volume) as one call -> [the outputs of problem b as a dict of numpy values]."""
    entry = fxs[0].entry
    if entry == "depth":
        out = gd._run(np.stack([f.D for f in fxs]), [dict(f.det, image=i) for i, f in enumerate(fxs)], iters=iters)
    elif entry == "feat":
        out = gf._run([f.M for f in fxs], [f.det for f in fxs], iters=iters)
    elif entry == "rgbd":
        out = grg._run([f.det for f in fxs], iters=iters)
    else:
        assert all(f.vol is fxs[0].vol for f in fxs)
        scene = dict(vol=_device_volume(fxs[0].vol), tau=fxs[0].tau)
        out = (gt if entry == "track" else gtr)._run(scene, [f.det for f in fxs], iters)
    return [{k: v[b] for k, v in out.items()} for b in range(len(fxs))]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def _restored(a, b):
    return np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and a["cost_out"] == b["cost_out"]


@pytest.mark.parametrize("fid", ls.IDS)
def test_every_step_of_the_pinned_prefix(fid):
    fx = ls.fixture(fid)
    ref = ls.pinned_prefix(fx)[1]
    trace, want = ref["trace"], lm_ref.decisions(ref["trace"])[:fx.K].replace("z", "r")
    outs = [_run([fx], k)[0] for k in range(fx.K + 1)]
    got, worst, capped = "", [0.0, 0.0], 0
    assert abs(outs[0]["cost_out"] - ref["cost_in"]) <= COST_TOL[fx.entry] * ref["cost_in"] and outs[0]["cost_out"] == outs[0]["cost_in"]
    assert np.array_equal(outs[0]["R"], fx.det["R"]) and np.array_equal(outs[0]["t"], fx.det["t"])
    for k, o in enumerate(outs):
        assert o["iters_used"] == k, (k, o["iters_used"])
        assert o["status"] == (0 if "a" in want[:k] else 1), (k, o["status"])
        assert abs(o["cost_in"] - ref["cost_in"]) <= COST_TOL[fx.entry] * ref["cost_in"] and o["cost_in"] == outs[0]["cost_in"], k
        assert o["num_points"] == ref["num_points"], k
        if k == 0:
            continue
        rec = trace[k - 1]
        if rec["kind"] == "acc":
            assert o["cost_out"] < outs[k - 1]["cost_out"], k
        else:
            assert _restored(o, outs[k - 1]), (k, rec["kind"])       # the pose of the call before, not the trial
        got += "a" if o["cost_out"] < outs[k - 1]["cost_out"] else ("r" if _restored(o, outs[k - 1]) else "?")
        dR, dt = float(np.linalg.norm(o["R"] - rec["R"])), float(np.linalg.norm(o["t"] - rec["t"]))
        worst = [max(worst[0], dR), max(worst[1], dt)]
        assert dR <= ls.POSE_RAD and dt <= ls.POSE_MM, (k, dR, dt)
        capped += k < fx.K and trace[k]["kind"] == "acc" and o["status"] == 0    # the cap fell in mid-descent: the next step is an accepted one
    print(f"{fx!r}: {got}, largest distance from the restatement {worst[0]:.2e} (|dR|_F) / {worst[1]:.2e} mm, cost_in {outs[0]['cost_in']!r} vs {ref['cost_in']!r}")
    assert got == want
    assert capped or "a" not in want[1:]


@pytest.mark.parametrize("fid", ls.ZBAD_IDS)
def test_zbad_rule_refuses_a_step_that_lowers_the_cost(fid):
    fx = ls.fixture(fid)
    trace = ls.pinned_prefix(fx)[1]["trace"]
    ks = [k for k in range(1, fx.K + 1) if trace[k - 1]["kind"] == "zbad" and trace[k - 1]["Et"] < trace[k - 1]["E"]][:3]
    assert ks
    for k in ks:
        before, after = _run([fx], k - 1)[0], _run([fx], k)[0]
        assert _restored(after, before) and (before["iters_used"], after["iters_used"]) == (k - 1, k), k


@pytest.mark.parametrize("entry", ls.ENTRIES)
def test_failed_factorisations_up_to_the_lambda_ceiling(entry):
    fx = ls.ceiling_fixture(entry)
    outs = {}
    for iters in ls.CEILING_ITERS:
        o, ref = _run([fx], iters)[0], fx.run(iters)
        outs[iters] = o
        print(f"{fx!r} iters {iters}: iters_used {o['iters_used']} (restatement {ref['iters_used']}), status {o['status']}, cost {o['cost_in']!r} vs {ref['cost_in']!r}")
        assert o["iters_used"] == ref["iters_used"] and o["status"] == ref["status"] == 1 and o["num_points"] == ref["num_points"]
        assert o["cost_in"] == o["cost_out"] and abs(o["cost_in"] - ref["cost_in"]) <= COST_TOL[entry] * ref["cost_in"]
        assert np.array_equal(o["R"], fx.det["R"]) and np.array_equal(o["t"], fx.det["t"])
    if entry == "depth":
        assert outs[30]["cost_in"] == 4.0
    # once two successive calls return the same iters_used < iters, every later call is bit-identical to them
    a, b, c = (outs[k] for k in ls.CEILING_ITERS[-3:])
    assert b["iters_used"] == c["iters_used"] < ls.CEILING_ITERS[-2] and _same(b, c) and _same(a, b)


@pytest.mark.parametrize("entry", ls.ENTRIES)
def test_mixed_batch_equals_every_problem_alone(entry):
    fxs = ls.mixed_batch(entry)
    for iters in ls.MIXED_ITERS:
        batch = _run(fxs, iters)
        alone = [_run([fx], iters)[0] for fx in fxs]
        print(f"{entry} iters {iters}: iters_used {[int(o['iters_used']) for o in batch]}, status {[int(o['status']) for o in batch]}")
        assert [int(o["status"]) for o in batch] == [1, 0, 2, 2]
        assert [int(o["iters_used"]) for o in batch] == [fx.run(iters)["iters_used"] for fx in fxs]
        for b, fx in enumerate(fxs):
            assert _same(batch[b], alone[b]), (iters, fx)
