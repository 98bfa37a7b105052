"""fp_pose_errors throughput (MSSD + MSPD of a batch of hypotheses) at three shapes, batches 1 and 32, on the device; and
the reference's numpy loop (utils/eval_errors.py: one transform_pts_Rt / project_pts pass per symmetry) at the same
shapes on the CPU, one hypothesis, labelled as a CPU number.

    python tools/bench_pose_eval.py [--iters 20] [--no-cpu]

Device time: HIP events around one call (the table upload and both kernels, pose_err_partial and pose_err_fold); the
per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.  FP64 share: VALU
instructions the partial kernel issues per (vertex, symmetry) pair (VALU_PER_PAIR, counted in its gfx950 ISA) x pairs /
time, over the FP64 vector issue rate 78.6 TFLOP/s / 2 (an FMA counts two FLOPs, the peak is one FMA per lane-cycle).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("lmo-like S=1 N=12k", 12_000, 1), ("lmo-like S=2 N=12k", 12_000, 2), ("tless-like S=630 N=30k", 30_000, 630),
          ("worst S=630 N=100k", 100_000, 630))
VALU_PER_PAIR = 827 / 8      # VALU instructions of one symmetry iteration of pose_err_partial (8 vertices per lane)
F64_PER_PAIR = 644 / 8       # ... of which fp64 arithmetic
FP64_ISSUE_PEAK = 78.6e12 / 2


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_case(rng, n, s):
    pts = rng.normal(0, 40, (n, 3))
    syms = [{"R": np.eye(3), "t": np.zeros((3, 1))}] + [{"R": _rot(rng), "t": rng.normal(0, 2, (3, 1))} for _ in range(s - 1)]
    R_gt, t_gt = _rot(rng), np.array([[5.0], [-3.0], [700.0]])
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    return dict(pts=pts, syms=syms, R_gt=R_gt, t_gt=t_gt, R_est=R_gt, t_est=t_gt + 3.0, K=K)


def cpu_reference(c):
    """utils/eval_errors.py mssd + mspd, with the toolkit's transform_pts_Rt / project_pts."""
    def tr(pts, R, t):
        return (R.dot(pts.T) + t.reshape((3, 1))).T

    def pr(pts, K, R, t):
        P = K.dot(np.hstack((R, t)))
        im = P.dot(np.hstack((pts, np.ones((pts.shape[0], 1)))).T)
        im /= im[2, :]
        return im[:2, :].T
    pe, qe, es, ps = tr(c["pts"], c["R_est"], c["t_est"]), pr(c["pts"], c["K"], c["R_est"], c["t_est"]), [], []
    for s in c["syms"]:
        R, t = c["R_gt"].dot(s["R"]), c["R_gt"].dot(s["t"]) + c["t_gt"]
        es.append(np.linalg.norm(tr(c["pts"], R, t) - pe, axis=1).max())
        ps.append(np.linalg.norm(qe - pr(c["pts"], c["K"], R, t), axis=1).max())
    return min(es), min(ps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from foundpose_amd import eval_util, ops
    assert torch.cuda.is_available(), "bench_pose_eval measures the MI355X"
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(0)}; FP64 vector peak 78.6 TFLOP/s (spec) -> {FP64_ISSUE_PEAK / 1e12:.1f} T lane-instructions/s")
    print(f"{'shape':<24}{'batch':>6}{'device us/call':>16}{'us/hyp':>10}{'hyp/s':>12}{'Gpairs/s':>10}{'VALU share':>12}{'CPU numpy s/hyp':>18}")
    for name, n, s in SHAPES:
        base = make_case(rng, n, s)
        cpu = None
        if not args.no_cpu:
            t0 = time.perf_counter()
            cpu_reference(base)
            cpu = time.perf_counter() - t0
        for batch in (1, 32):
            items = [dict(base, R_est=base["R_gt"] @ _rot(rng), t_est=base["t_gt"] + rng.normal(0, 5, (3, 1))) for _ in range(batch)]
            ev_args = _device_args(items, torch)
            for _ in range(3):
                ops.pose_errors(*ev_args)
            torch.cuda.synchronize()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = []
            for _ in range(args.iters):
                st.record()
                ops.pose_errors(*ev_args)
                en.record()
                en.synchronize()
                ts.append(st.elapsed_time(en) * 1e3)
            us = float(np.median(ts))
            pairs = batch * n * s
            share = VALU_PER_PAIR * pairs / (us * 1e-6) / FP64_ISSUE_PEAK
            cpu_s = f"{cpu:.4f}" if (cpu is not None and batch == 1) else ""
            print(f"{name:<24}{batch:>6}{us:>16.1f}{us / batch:>10.1f}{batch / (us * 1e-6):>12.0f}{pairs / (us * 1e-6) / 1e9:>10.1f}{share:>12.1%}{cpu_s:>18}")
            err, _ = eval_util.pose_errors_batch(items[:1])   # the evaluator's own path on the same hypothesis agrees
            assert np.array_equal(err, ops.pose_errors(*_device_args(items[:1], torch))[0].cpu().numpy())
    print(f"VALU share: {VALU_PER_PAIR:.1f} VALU instructions per (vertex, symmetry), {F64_PER_PAIR:.1f} of them fp64, over the fp64 issue peak;"
          " the device time includes the fold kernel and the table upload.")


def _device_args(items, torch):
    from tests import pose_eval_ref as ref   # the kernel's input rows, composed as the evaluator composes them
    rows = [ref.rows(it["R_est"], it["t_est"], it["R_gt"], it["t_gt"], it["K"], it["syms"]) for it in items]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    n, s = len(items[0]["pts"]), len(items[0]["syms"])
    ranges = np.array([(0, n, h * s, s) for h in range(len(items))])
    return (d(items[0]["pts"]), d(np.stack([r[0] for r in rows])), d(np.stack([r[1] for r in rows])), d(np.concatenate([r[2] for r in rows])),
            d(np.concatenate([r[3] for r in rows])), ranges)


if __name__ == "__main__":
    main()
