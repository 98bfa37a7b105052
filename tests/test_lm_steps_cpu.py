"""CPU: the fixtures of tests/test_gpu_lm_steps.py (tests/lm_steps.py) satisfy, on the restatement alone, what that test relies on.

  * Every fixture's K lies inside its PINNED PREFIX (tests/lm_steps.py: decision margin, agreement of the restatement with itself under the
    reversed point order, no per-point branch within 1e-9 of flipping) and is min(prefix, 24).
  * Per entry point the prefix of at least one fixture holds at least three accepted steps and three COST rejections ("r": an admissible
    step with Et >= E; what the z-bad rule refuses, "z", does not count), a cost rejection right after an accepted step, two in a row
    and a cap that falls in mid-descent; and not every fixture starts with the same decision.
  * The z-bad fixtures hold refused steps that lower the cost, their deciding z at least 1e-3 mm below 1.
  * The ceiling fixtures fail every factorisation: iters_used follows the repeated `lam *= 10.0` exactly.
  * Each fault a kernel could have (a switch of tests/lm_ref.lm_loop) changes what the GPU test expects on at least one fixture.

Seeds 0 .. 7 were searched per entry point; the prefixes found (K in brackets where shorter than the prefix):
  depth      edge0 (6 deg / 25 mm, tau 25) 39 [24]  arrrrrrarararrarrararara   edge5 (10 / 40, tau 15) 40 [24]  rraraaarrrrrarrararararr
             edge2 (6 / 25, tau 25) 40 [24]  araraaarrrrrrrararrarara
  feat       edge7 (30 / 120, edge 6, noise 1) 28 [24]  aaaaarrrrrrrraaaaaaarrrr   edge0 (30 / 120, edge 6, noise 2) 18  aaaaaaaaarrrrrrrrr
             zbad1 (lift 6 mm) 18  zazzzzazazazzazazz   zbad0 (lift 12 mm) 21  azzzazazazzazazazazaz   field0 (10 / 40) 4  aaaa
  rgbd       edge5_tau25 (6 / 25) 30 [24]  aarrrrrarrarararararrara   zbad1 18  zazzzzazazazzazazz   edge5_tau15 (10 / 40) 26 [24]  aaaarrrrrrrrarararrarara
  track      blob0 (6 deg / 6 mm, 7.5 mm) 38 [24]  aarrarrrrrarararararrrar   blob4 (15 / 12, 5 mm) 40 [24]  raaaaaaaarrrrrrarrararar
  track_rgb  blob3 (6 / 6, 7.5 mm) 36 [24]  arrrraaaarrrrarrarrarara   blob4 (15 / 12, 5 mm) 40 [24]  raaaaaaaaaaaaaaaarrrrrrr
The feature term on a smooth map descends without a clear rejection from every start tried up to 10 degrees (field0 pins that plain
descent); its cost rejections come from far starts (30 degrees / 120 mm) on a map with an edge in feature space and noisy features,
on margins from 2.4e-4 (edge7) and 2.2e-3 (edge0) -- the GPU's cost differs from the restatement's by about 1e-8 relative -- and its
other refusals from the z-bad rule.  No trajectory found reaches the lambda ceiling by sixteen clear-margin rejections in a
row: the ceiling is pinned by the failed factorisations of the ceiling fixtures only.
"""

import functools

import numpy as np
import pytest

from tests import lm_ref
from tests import lm_steps as ls


def _string(trace):
    return lm_ref.decisions(trace)


@pytest.mark.parametrize("entry", ls.ENTRIES)
def test_prefix_is_long_enough_and_holds_what_the_gpu_test_needs(entry):
    """The content is asked of COST rejections ("r": admissible, Et >= E); what the z-bad rule refuses ("z") does not count towards it."""
    firsts, rich = set(), 0
    for fx in ls.fixtures(entry):
        n, ref, spread = ls.pinned_prefix(fx)
        s = _string(ref["trace"])
        rej = [r["margin"] for r in ref["trace"][:fx.K] if r["kind"] == "rej"]
        print(f"{fx!r}: prefix {n}, K {fx.K}, {s[:fx.K]}|{s[fx.K:n]}, {len(rej)} cost rejections on margins from {min(rej or [np.inf]):.1e}, "
              f"spread under the reversed order {spread[0]:.1e} (|dR|_F) / {spread[1]:.1e} mm")
        assert fx.K == min(n, ls.K_MAX) and fx.K >= 4
        assert spread[0] <= ls.POSE_RAD / 1000 and spread[1] <= ls.POSE_MM / 1000
        assert fx.run(fx.K)["iters_used"] == fx.K                       # the trajectory has not stopped before K
        p = s[:fx.K]
        firsts.add(p[0])
        mid = any(p[k] == "a" and "a" in p[:k] for k in range(1, fx.K))   # a cap at k leaves the next accepted step undone
        rich += p.count("a") >= 3 and p.count("r") >= 3 and "ar" in p and "rr" in p and mid
    assert rich >= 1 and len(firsts) > 1, (rich, firsts)


def test_zbad_fixtures_refuse_steps_that_lower_the_cost():
    assert {i.split(":")[0] for i in ls.ZBAD_IDS} == {"feat", "rgbd"}
    for fx in map(ls.fixture, ls.ZBAD_IDS):
        assert fx.run(0)["num_points"] == ls.NPTS                       # the start: every point in front of z = 1 and inside the map
        z = [r for r in ls.pinned_prefix(fx)[1]["trace"][:fx.K] if r["kind"] == "zbad"]
        print(f"{fx!r}: {len(z)} refused steps, {sum(r['Et'] < r['E'] for r in z)} of them lower the cost, 1 - z from {min(r['z_gap'] for r in z):.3g} mm")
        assert any(r["Et"] < r["E"] for r in z) and all(r["z_gap"] >= ls.Z_GAP for r in z)


@pytest.mark.parametrize("entry", ls.ENTRIES)
def test_ceiling_fixture_fails_every_factorisation(entry):
    fx = ls.ceiling_fixture(entry)
    lam, n = 1e-3, 0
    while True:          # the restated schedule: the count of failures after which lam > 1e12
        n += 1
        lam *= 10.0
        if lam > 1e12:
            break
    used = []
    for iters in ls.CEILING_ITERS:
        r = fx.run(iters)
        used.append(r["iters_used"])
        assert r["iters_used"] == min(iters, n) and r["status"] == 1 and r["cost_in"] == r["cost_out"] > 0 and r["num_points"] >= 6
        assert np.array_equal(r["R"], fx.det["R"]) and np.array_equal(r["t"], fx.det["t"])
        assert all(rec["kind"] == "chol" for rec in r["trace"]) and len(r["trace"]) == r["iters_used"]
    if entry == "depth":
        assert used == [0, 1, 5, 15, 16, 16, 16] and fx.run(30)["cost_in"] == 4.0


def test_mixed_batch_problems_stop_at_different_iterations():
    for entry in ls.ENTRIES:
        c, d, few, nopose = ls.mixed_batch(entry)
        assert [x.run(20)["status"] for x in (c, d, few, nopose)] == [1, 0, 2, 2]
        assert c.run(20)["iters_used"] == c.run(30)["iters_used"] < 20 and d.run(20)["iters_used"] == 20 and few.run(20)["num_points"] == 5


# ---------------------------------------------------------------------------------------------------------- the mutation table
MUTATIONS = {
    "reject x 100": dict(reject_factor=100.0),
    "no lambda / 10 on accept": dict(accept_divides=False),
    "failed Cholesky not counted": dict(count_failed_cholesky=False),
    "cap at it > iters": dict(cap_inclusive=True),
    "lambda ceiling at >=": dict(ceiling_inclusive=True),
    "trial pose kept on reject": dict(keep_trial_on_reject=True),
    "z-bad rule off": dict(admissible_rule=False),
    "status 0 without an accept": dict(status_needs_accept=False),
}


def _sweep_points():
    """[(fixture, iters)]: what the GPU test runs and compares -- the sweeps over 0 .. K and the ceiling fixtures at CEILING_ITERS."""
    return [(fx, k) for fx in map(ls.fixture, ls.IDS) for k in range(fx.K + 1)] + [(ls.ceiling_fixture(e), k) for e in ls.ENTRIES for k in ls.CEILING_ITERS]


@functools.lru_cache(maxsize=None)
def _expected(fx, k):
    return fx.run(k)


def _noticed(fx, k, lm):
    """Would the GPU test's assertions at `iters` = k fail on a kernel with this fault?  The exact outputs, the decision string, the pose
    beyond the bar -- or a pose that a rejected step did not restore bit for bit."""
    want, got = _expected(fx, k), fx.run(k, **lm)
    if (got["iters_used"], got["status"]) != (want["iters_used"], want["status"]):
        return True
    if _string(got["trace"]).replace("z", "r") != _string(want["trace"]).replace("z", "r"):
        return True
    if np.linalg.norm(got["R"] - want["R"]) > ls.POSE_RAD or np.linalg.norm(got["t"] - want["t"]) > ls.POSE_MM:
        return True
    if k and want["trace"] and len(want["trace"]) == k and want["trace"][-1]["kind"] != "acc":
        before = _expected(fx, k - 1)
        return not (np.array_equal(got["R"], before["R"]) and np.array_equal(got["t"], before["t"]) and got["cost_out"] == before["cost_out"])
    return False


@pytest.mark.parametrize("name", MUTATIONS)
def test_every_fault_changes_what_the_gpu_test_expects(name):
    """On some fixture -- and, since refine.hip and rgbd_refine.hip have SOLVE_STEP branches of their own, on a fixture of each of the two
    feature solvers as well."""
    for entries in (ls.ENTRIES, ("feat",), ("rgbd",)):
        hit = next(((fx, k) for fx, k in _sweep_points() if fx.entry in entries and _noticed(fx, k, MUTATIONS[name])), None)
        print(f"{name} among {entries}: first noticed by {hit[0]!r} at iters = {hit[1]}" if hit else f"{name} among {entries}: NOT noticed")
        assert hit is not None, entries
