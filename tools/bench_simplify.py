"""fp_mesh_cell_keys and fp_mesh_cluster (csrc/simplify.hip) and the torch plumbing between and after them (foundpose_amd/simplify.py) on
the device: a mesh of the size reconstruct's benchmark emits, simplified to 20 000 vertices, beside the numpy restatement
(tests/simplify_ref.py) on a mesh small enough to run on this machine's CPU, scaled per input vertex.

    python tools/bench_simplify.py [--iters 10] [--no-cpu] [--res 600] [--target 20000] [--downstream] [--out profiles/simplify_bench.txt]

The input is synthetic.make_blob_mesh(res, res, radius=90): about res^2 vertices and 2 res^2 triangles.  Device time: HIP events around
one stage, the median of --iters runs after 2 warm-up runs, one process.  Stages: keys (fp_mesh_cell_keys), plumbing (torch.unique, the two
stable sorts, the two bincount + cumsum), cluster (fp_mesh_cluster), faces (the face rules: gather, sort, torch.unique over rows,
scatter_reduce).  The bisection on the cell size (32 rounds of keys + torch.unique, one read-back each) is timed separately, once warm.
--downstream also times what motivates a lighter mesh, on the input and on the output: ADD and ADD-S of 10 poses (fp_pose_add_errors over
all vertices, what eval_add runs per estimate) and models_info.calc_models_info(symmetries=True), wall clock."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters):
    import torch
    ts = []
    for it in range(iters + 2):
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        out = fn()
        en.record()
        en.synchronize()
        if it >= 2:
            ts.append(st.elapsed_time(en))
    return float(np.median(ts)), out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--res", type=int, default=600)
    ap.add_argument("--target", type=int, default=20000)
    ap.add_argument("--downstream", action="store_true")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "simplify_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import ops, simplify, synthetic
    assert torch.cuda.is_available(), "bench_simplify measures the MI355X"
    mesh = synthetic.make_blob_mesh(args.res, args.res, radius=90.0)
    V, F = len(mesh.vertices), len(mesh.faces)
    v64 = mesh.vertices.astype(np.float64)
    vmin, vmax = v64.min(0), v64.max(0)
    verts, cols, faces = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (mesh.vertices, mesh.colors, mesh.faces))
    lines = [f"# python tools/bench_simplify.py on one {torch.cuda.get_device_name(0)} (device: HIP events around a stage, median of {args.iters} after 2 "
             f"warm-up runs): make_blob_mesh({args.res}, {args.res}, radius=90), {V} vertices and {F} triangles, to at most {args.target} vertices"]
    count = simplify.cell_counter(verts, vmin, vmax)
    simplify.choose_cell_mm(vmin, vmax, args.target, count)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = simplify.choose_cell_mm(vmin, vmax, args.target, count)
    torch.cuda.synchronize()
    bis = time.perf_counter() - t0
    origin, dims = simplify.grid_for(vmin, vmax, c)
    lines.append(f"bisection {bis * 1e3:9.3f} ms wall   {simplify.BISECTION_ROUNDS} rounds of keys + torch.unique with one read-back each -> cells of {c!r} mm, "
                 f"grid {dims[0]} x {dims[1]} x {dims[2]}")
    ms_k, keys = _timed(lambda: ops.mesh_cell_keys(verts, origin, c, dims), args.iters)
    lines.append(f"keys      {ms_k:9.3f} ms   {V / ms_k / 1e6:8.2f} G vertices/s   {20.0 * V / ms_k / 1e6:7.2f} GB/s (12 B read, 8 B written per vertex)")
    ms_p, tb = _timed(lambda: ops.mesh_cluster_tables(keys, faces), args.iters)
    C = len(tb["cells"])
    lines.append(f"plumbing  {ms_p:9.3f} ms   torch.unique over {V} keys -> {C} cells; stable sorts of {V} and {3 * F} ranks; two bincount + cumsum")
    ms_c, out = _timed(lambda: ops.mesh_cluster(verts, cols, faces, tb, origin, c, dims), args.iters)
    gathered = 24.0 * V + 3 * F * (8 + 12 + 36) + 16.0 * V     # vertex records; per corner record its id, the face and three positions; the orders
    lines.append(f"cluster   {ms_c:9.3f} ms   {C / ms_c / 1e3:8.2f} M cells/s   {(V + 3 * F) / ms_c / 1e6:7.2f} G records/s   gathers {gathered / 1e6:.1f} MB "
                 f"({gathered / ms_c / 1e6:.1f} GB/s)   status counts {dict(zip(*(a.tolist() for a in np.unique(out['status'].cpu().numpy(), return_counts=True))))}")
    ms_f, f_out = _timed(lambda: simplify.output_faces(tb["rank"], faces), args.iters)
    lines.append(f"faces     {ms_f:9.3f} ms   {F} -> {len(f_out)} triangles (gather, row sort, torch.unique over rows, scatter_reduce)")
    total = ms_k + ms_p + ms_c + ms_f
    lines.append(f"sum       {total:9.3f} ms   keys {100 * ms_k / total:.1f} %, plumbing {100 * ms_p / total:.1f} %, cluster {100 * ms_c / total:.1f} %, "
                 f"faces {100 * ms_f / total:.1f} %")
    t0 = time.perf_counter()
    small, report = simplify.simplify_mesh(mesh, simplify.SimplifyOpts(target_vertices=args.target))
    lines.append(f"simplify_mesh, everything (uploads, bisection, read-backs, host compaction, normals, topology): {time.perf_counter() - t0:.3f} s wall -> "
                 f"{report['vertices_out']} vertices, {report['triangles_out']} triangles, rms quadric error {report['rms_quadric_error_mm']:.4f} mm, "
                 f"{report['topology']['boundary_edges']} boundary and {report['topology']['nonmanifold_edges']} non-manifold edges")
    if not args.no_cpu:
        from tests import simplify_ref as ref
        m = synthetic.make_blob_mesh(150, 150, radius=90.0)
        cs = ref.choose_cell(m.vertices, 1250)
        t0 = time.perf_counter()
        r = ref.simplify(m.vertices, m.colors, m.faces, cs)
        host = time.perf_counter() - t0
        per = host * 1e6 / len(m.vertices)
        lines.append(f"numpy restatement, {len(m.vertices)} vertices -> {len(r['vertices'])} on one CPU thread (keys, tables, sums, solve, faces): {host:.3f} s = "
                     f"{per:.1f} us per input vertex; at that rate the {V}-vertex mesh takes ~{per * V / 1e6:.0f} s, {per * V / 1e3 / total:.0f} x the device's "
                     f"{total:.2f} ms")
    if args.downstream:
        from foundpose_amd.models_info import calc_models_info
        from foundpose_amd.renderer import save_ply
        rng = np.random.default_rng(0)
        poses = np.concatenate([np.tile(np.eye(3).reshape(-1), (10, 1)), rng.normal(size=(10, 3))], 1)
        gt = np.concatenate([np.tile(np.eye(3).reshape(-1), (10, 1)), np.zeros((10, 3))], 1)
        est, gtd = torch.from_numpy(poses).cuda(), torch.from_numpy(gt).cuda()
        for name, m in (("input", mesh), ("output", small)):
            pts = torch.from_numpy(m.vertices.astype(np.float64)).cuda()
            ranges = np.tile(np.array([[0, len(pts)]], np.int64), (10, 1))
            ms_a, _ = _timed(lambda: ops.pose_add_errors(pts, est, gtd, ranges), args.iters)
            with tempfile.TemporaryDirectory() as d:
                save_ply(os.path.join(d, "obj_000001.ply"), m)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calc_models_info(d, symmetries=True)
                torch.cuda.synchronize()
                sym = time.perf_counter() - t0
            lines.append(f"downstream, {name} ({len(pts)} vertices): ADD and ADD-S of 10 poses {ms_a:9.3f} ms = {ms_a / 10:.3f} ms per pose; "
                         f"calc_models_info(symmetries=True) {sym:.2f} s wall")
            print(lines[-1], flush=True)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fobj:
        fobj.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
