"""The one numpy restatement of csrc/refine_terms.hpp's Levenberg-Marquardt state machine (TEST HELPER), with a trace.

lambda starts at 1e-3; a step is accepted when its cost is below the current one (and, for the two feature solvers, the trial pose is
admissible: none of its valid points has z <= 1 mm), then lambda / 10 (floor 1e-12); a rejected step or a failed Cholesky is one
iteration and lambda x 10; the loop stops at lambda > 1e12, at a relative decrease < 1e-10 or at `iters`.  The five restatements
(depth_refine_ref, featuremetric_ref, rgbd_refine_ref, tsdf_track_ref, tsdf_track_rgb_ref) call lm_loop with their own system.

The keyword switches after `z_gap` are the faults a wrong kernel could have (tests/test_lm_steps_cpu.py turns each on to show that the
step fixtures notice it); off, every floating-point statement is the one the five loops had.
"""

import numpy as np

DECISIONS = {"chol": "c", "acc": "a", "rej": "r", "zbad": "z"}


def rot_exp(w):
    """exp([w]x) (Rodrigues; series below 1e-8 rad) -- csrc/rot.hpp."""
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) + a * K + b * (K @ K)


def update(R, t, d):
    """R' = exp([w]x) R, t' = exp([w]x) t + v for d = (w, v)."""
    E = rot_exp(d[:3])
    return E @ R, E @ t + d[3:]


def lm_loop(system_at, R, t, E, Hm, g, iters, solve, admissible=None, z_gap=None, *, reject_factor=10.0, accept_divides=True,
            count_failed_cholesky=True, cap_inclusive=False, ceiling_inclusive=False, keep_trial_on_reject=False, admissible_rule=True,
            status_needs_accept=True):
    """From the system (E, Hm, g) at the input pose (R, t).  system_at(R, t) -> (E, H, g, extra); solve(H, g, lam) -> d or None;
    admissible(extra) -> bool (None: every pose is); z_gap(R, t) -> how far the deciding z of an inadmissible pose lies from 1.0.
    -> dict R, t, cost_out, iters_used, status, trace.  trace: one record per iteration -- kind "chol" | "acc" | "rej" | "zbad", lam (before
    the step), E, Et and trial = (Rt, tt) (None for "chol"), R, t (the pose after the step), margin = |Et - E| / E (inf for "chol"), z_gap (None unless "zbad")."""
    lam, it, accepted, trace = 1e-3, 0, False, []
    over = (lambda v: v >= 1e12) if ceiling_inclusive else (lambda v: v > 1e12)
    while (it <= iters) if cap_inclusive else (it < iters):
        d = solve(Hm, g, lam)
        if d is not None or count_failed_cholesky:
            it += 1
        if d is None:
            trace.append(dict(kind="chol", lam=lam, E=E, Et=None, trial=None, R=R, t=t, margin=np.inf, z_gap=None))
            lam *= reject_factor
            if over(lam):
                break
            continue
        Rt, tt = update(R, t, d)
        Et, Ht, gt, extra = system_at(Rt, tt)
        ok = admissible is None or not admissible_rule or bool(admissible(extra))
        rec = dict(lam=lam, E=E, Et=Et, trial=(Rt, tt), margin=abs(Et - E) / E, z_gap=None)
        if ok and Et < E:
            rel = (E - Et) / E
            R, t, E, Hm, g = Rt, tt, Et, Ht, gt
            if accept_divides:
                lam = max(lam / 10.0, 1e-12)
            accepted = True
            trace.append(dict(rec, kind="acc", R=R, t=t))
            if rel < 1e-10:
                break
        else:
            if keep_trial_on_reject:
                R, t = Rt, tt
            bad = admissible is not None and not admissible(extra)
            trace.append(dict(rec, kind="zbad" if bad else "rej", R=R, t=t, z_gap=z_gap(Rt, tt) if bad and z_gap is not None else None))
            lam *= reject_factor
            if over(lam):
                break
    return dict(R=R, t=t, cost_out=E, iters_used=it, status=0 if accepted or not status_needs_accept else 1, trace=trace)


def decisions(trace):
    """The trace as a string: one of c, a, r, z per iteration."""
    return "".join(DECISIONS[r["kind"]] for r in trace)
