"""Class-agnostic mask proposals from depth: fit the supporting planes, drop them, cut what stands on them into
connected components along depth discontinuities.  No weights: the table-top segmentation of RGB-D robotics, on the GPU
(csrc/depth_proposals.hip behind fp_depth_plane_fit, fp_depth_components, fp_component_table and fp_component_runs).

    python -m foundpose_amd.depth_proposals --dataset-dir <split> --output proposals.json [--opts opts.json] [--targets targets.json]
                                            [--report report.json]
        writes the proposals of every image of the split (or of the images the targets name) as CNOS-shaped records
        {scene_id, image_id, segmentation {size, counts}, bbox [x, y, w, h], score (area / (H W)), time}: what
        `python -m foundpose_amd.detect run --proposals` reads.  The report holds, per frame, the planes, their supports and the
        component counts.

opts.json is {"depth_proposal_opts": {...}} or the bare dict; unknown keys are an error."""

import argparse
import json
import os
import time
from dataclasses import asdict, dataclass, fields
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops
from .eval_bop19 import load_depth

MAX_BATCH = 32   # frames per call, at most
MAX_LEVELS = 3


@dataclass
class DepthProposalOpts:
    num_planes: int = 1                 # planes fitted one after the other, 0 .. 4
    plane_hypotheses: int = 256
    plane_stride: int = 4               # hypotheses are counted on every plane_stride-th row and column
    plane_thresh_mm: float = 10.0
    min_plane_share: float = 0.05       # a plane needs this share of the frame's valid pixels
    max_depth_mm: float = 0.0           # 0: no limit
    object_margin_mm: float = 15.0      # foreground stands higher than this over every accepted plane
    connect_mm: Union[float, List[float]] = 5.0   # up to three ascending values: one level each
    connect_slope: float = 4.0          # pixel footprints of depth allowed per pixel step
    min_pixels: int = 200
    max_area_share: float = 0.5
    max_proposals: int = 64             # per frame and level
    seed: int = 0

    def levels(self) -> List[float]:
        return [float(v) for v in (self.connect_mm if isinstance(self.connect_mm, (list, tuple)) else [self.connect_mm])]


def check_opts(opts: DepthProposalOpts) -> DepthProposalOpts:
    def integer(name, lo, hi):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, int) or v < lo or v > hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")

    def number(name, lo, hi, lo_open=False):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or v < lo or v > hi or (lo_open and v == lo):
            raise ValueError(f"{name} must be a number in {'(' if lo_open else '['}{lo}, {hi}], got {v!r}")
    integer("num_planes", 0, _lib.DEPTH_MAX_PLANES)
    integer("plane_hypotheses", 1, _lib.DEPTH_MAX_HYPOTHESES)
    integer("plane_stride", 1, 64)
    integer("min_pixels", 1, 2**31 - 1)
    integer("max_proposals", 1, _lib.DEPTH_MAX_PROPOSALS)
    integer("seed", 0, 2**64 - 1)
    number("plane_thresh_mm", 0.0, 1e9, lo_open=True)
    number("min_plane_share", 0.0, 1.0)
    number("max_depth_mm", 0.0, 1e9)
    number("object_margin_mm", -1e9, 1e9)
    number("connect_slope", 0.0, 1e9)
    number("max_area_share", 0.0, 1.0, lo_open=True)
    c = opts.connect_mm
    vals = list(c) if isinstance(c, (list, tuple)) else [c]
    if not 1 <= len(vals) <= MAX_LEVELS or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or v < 0 for v in vals) \
            or any(b <= a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"connect_mm must be a number >= 0 or a list of 1 .. {MAX_LEVELS} ascending ones, got {c!r}")
    return opts


def load_opts(path_or_dict=None) -> DepthProposalOpts:
    """{"depth_proposal_opts": {...}} or the bare dict (None: the defaults); unknown keys are an error, as for DetectOpts."""
    d = path_or_dict
    if d is None:
        d = {}
    elif isinstance(d, DepthProposalOpts):
        return check_opts(d)
    elif not isinstance(d, dict):
        with open(path_or_dict) as f:
            d = json.load(f)
    d = dict(d.get("depth_proposal_opts", d))
    known = {f.name for f in fields(DepthProposalOpts)}
    unknown = sorted(set(d) - known)
    if unknown:
        raise ValueError(f"unknown depth proposal options: {unknown}")
    return check_opts(DepthProposalOpts(**d))


def max_area_of(opts: DepthProposalOpts, height: int, width: int) -> int:
    return int(np.floor(np.float64(opts.max_area_share) * np.float64(height * width)))


def fit_planes(depth: torch.Tensor, cameras, frame_keys, opts: DepthProposalOpts, want_counts: bool = False):
    """The frames' plane sequences -> (planes fp64 [N, 4, 4] with the accepted ones in front, num_planes int32 [N], the records of every
    round [(plane [N, 4], info [N, 8], hypothesis counts or None)]).  Nothing is read back: a frame whose sequence has ended is skipped
    on the device (num_prior = -1)."""
    n = depth.shape[0]
    planes = torch.zeros(n, _lib.DEPTH_MAX_PLANES, 4, dtype=torch.float64, device=depth.device)
    num_planes = torch.zeros(n, dtype=torch.int32, device=depth.device)
    num_prior = torch.zeros(n, dtype=torch.int32, device=depth.device)
    rounds = []
    for k in range(opts.num_planes):
        plane, info, counts = ops.depth_plane_fit(depth, cameras, frame_keys, planes, num_prior, opts.plane_hypotheses, opts.plane_stride,
                                                  opts.plane_thresh_mm, opts.max_depth_mm, opts.min_plane_share, opts.seed, want_counts)
        rounds.append((plane, info, counts))
        accepted = info[:, 5] == 1
        planes[:, k] = torch.where(accepted[:, None], plane, torch.zeros_like(plane))
        num_planes += accepted.to(torch.int32)
        num_prior = torch.where(accepted, num_prior + 1, torch.full_like(num_prior, -1))
    return planes, num_planes, rounds


def segment(depth: torch.Tensor, cameras, planes: torch.Tensor, num_planes: torch.Tensor, opts: DepthProposalOpts) -> Dict[str, Any]:
    """Foreground, components, tables and run lengths on the plane records given: an exact function of (depth, cameras, planes).
    -> labels, rank_maps int32 [N, L, H, W]; tables int32 [N, L, P, 7]; counts int32 [N, L, 4]; runs int32 [total] and run_off int32
    [N L P + 1], the list of rank r of level l of frame f at group (f L + l) P + r."""
    n, h, w = depth.shape
    cam = np.asarray(cameras, np.float64).reshape(-1, 4)
    slope_fx = (np.float64(opts.connect_slope) / cam[:, 0]).astype(np.float32)
    labels, tables, counts, rank_maps = [], [], [], []
    for lv, cmm in enumerate(opts.levels()):
        lab = ops.depth_components(depth, cam, slope_fx, planes, num_planes, opts.max_depth_mm, opts.object_margin_mm, cmm)
        tab, cnt, rk = ops.component_table(lab, opts.min_pixels, max_area_of(opts, h, w), opts.max_proposals, lv,
                                           torch.stack(tables) if tables else None)
        labels.append(lab), tables.append(tab), counts.append(cnt), rank_maps.append(rk)
    out = {"labels": torch.stack(labels, 1), "tables": torch.stack(tables, 1), "counts": torch.stack(counts, 1), "rank_maps": torch.stack(rank_maps, 1)}
    out["runs"], out["run_off"] = ops.component_runs(out["rank_maps"].reshape(-1, h, w), out["counts"][:, :, 2].reshape(-1).contiguous(),
                                                     opts.max_proposals)
    return out


def propose(depth: torch.Tensor, cameras, frame_keys, opts: Optional[DepthProposalOpts] = None, want_counts: bool = False) -> Dict[str, Any]:
    """depth [N, H, W] fp32 mm on the device (0: no measurement), cameras [N, 4] = (fx, fy, cx, cy) and frame_keys [N] on the host ->
    planes fp64 [N, 4, 4], num_planes int32 [N], plane_rounds (fit_planes' records) and segment()'s entries."""
    opts = check_opts(opts or DepthProposalOpts())
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dim() != 3 or depth.dtype != torch.float32:
        raise ValueError("propose: depth must be float32 [N, H, W] on the device (there is no CPU path)")
    planes, num_planes, rounds = fit_planes(depth, cameras, frame_keys, opts, want_counts)
    out = segment(depth, cameras, planes, num_planes, opts)
    out.update(planes=planes, num_planes=num_planes, plane_rounds=rounds)
    return out


def frame_key(scene_id: int, image_id: int) -> int:
    return (int(scene_id) << 32) + int(image_id)


def _frames_of_split(split_dir: str, targets) -> List[Tuple[int, int, str, Tuple[float, float, float, float], float]]:
    """-> [(scene, image, depth path, camera, depth_scale)] in (scene, image) order."""
    wanted = None
    if targets is not None:
        if isinstance(targets, str):
            with open(targets) as f:
                targets = json.load(f)
        wanted = {(int(t["scene_id"]), int(t["im_id"] if "im_id" in t else t["image_id"])) for t in targets}
    frames = []
    for name in sorted(os.listdir(split_dir)):
        sdir = os.path.join(split_dir, name)
        cam_path = os.path.join(sdir, "scene_camera.json")
        if not (name.isdigit() and os.path.exists(cam_path)):
            continue
        with open(cam_path) as f:
            cams = json.load(f)
        for im in sorted(cams, key=int):
            sid, iid = int(name), int(im)
            if wanted is not None and (sid, iid) not in wanted:
                continue
            K = cams[im]["cam_K"]
            frames.append((sid, iid, os.path.join(sdir, "depth", f"{iid:06d}.png"), (float(K[0]), float(K[4]), float(K[2]), float(K[5])),
                           float(cams[im].get("depth_scale", 1.0))))
    return frames


def proposals_for_split(split_dir: str, opts=None, targets=None, report: Optional[List[Dict[str, Any]]] = None,
                        device: str = "cuda") -> List[Dict[str, Any]]:
    """The proposals of every frame of a BOP split (of the frames `targets` names: a list of {scene_id, im_id} or its file) as
    CNOS-shaped records, frame by frame, level by level, rank by rank.  Frames are batched by size, MAX_BATCH at most per call;
    `time` is the batch's wall time per frame.  report: a list that receives one entry per frame."""
    opts = load_opts(opts)
    frames = _frames_of_split(split_dir, targets)
    loaded = [load_depth(fr[2], fr[4]) for fr in frames]
    by_size: Dict[Tuple[int, int], List[int]] = {}
    for i, d in enumerate(loaded):
        by_size.setdefault(d.shape, []).append(i)
    per_frame: Dict[int, List[Dict[str, Any]]] = {}
    notes: Dict[int, Dict[str, Any]] = {}
    L, P = len(opts.levels()), opts.max_proposals
    for (h, w), members in by_size.items():
        for b0 in range(0, len(members), MAX_BATCH):
            batch = members[b0:b0 + MAX_BATCH]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            depth = torch.from_numpy(np.stack([loaded[i] for i in batch])).to(device)
            out = propose(depth, [frames[i][3] for i in batch], [frame_key(frames[i][0], frames[i][1]) for i in batch], opts)
            tables, counts = out["tables"].cpu().numpy(), out["counts"].cpu().numpy()
            runs, run_off = out["runs"].cpu().numpy(), out["run_off"].cpu().numpy()
            seconds = (time.perf_counter() - t0) / len(batch)
            rounds = [(p_.cpu().numpy(), i_.cpu().numpy()) for p_, i_, _ in out["plane_rounds"]]
            for f, i in enumerate(batch):
                sid, iid = frames[i][0], frames[i][1]
                recs = []
                for lv in range(L):
                    for r in range(int(counts[f, lv, 2])):
                        label, area, x0, y0, x1, y1, _ = (int(v) for v in tables[f, lv, r])
                        g = (f * L + lv) * P + r
                        recs.append({"scene_id": sid, "image_id": iid,
                                     "segmentation": {"size": [h, w], "counts": runs[run_off[g]:run_off[g + 1]].tolist()},
                                     "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1], "score": area / float(h * w), "time": seconds})
                per_frame[i] = recs
                notes[i] = {"scene_id": sid, "image_id": iid, "size": [h, w],
                            "planes": [{"plane": p_[f].tolist(), "winner": int(i_[f, 0]), "subgrid_count": int(i_[f, 1]), "support": int(i_[f, 2]),
                                        "eligible": int(i_[f, 3]), "valid": int(i_[f, 4]), "accepted": bool(i_[f, 5])}
                                       for p_, i_ in rounds if i_[f, 6] >= 0],
                            "levels": [{"connect_mm": c, "components": int(counts[f, lv, 0]), "within_area_limits": int(counts[f, lv, 1]),
                                        "kept": int(counts[f, lv, 2]), "same_as_finer": int(counts[f, lv, 3])} for lv, c in enumerate(opts.levels())]}
    if report is not None:
        report.extend(notes[i] for i in range(len(frames)))
    return [r for i in range(len(frames)) for r in per_frame[i]]


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--output", required=True, help="the proposals file to write")
    ap.add_argument("--opts", default=None, help="options JSON ({'depth_proposal_opts': {...}}); default: the defaults")
    ap.add_argument("--targets", default=None, help="a BOP targets file: only its images are segmented")
    ap.add_argument("--report", default=None, help="write the planes, their supports and the component counts per frame here")
    args = ap.parse_args(argv)
    opts = load_opts(args.opts)
    report: List[Dict[str, Any]] = []
    records = proposals_for_split(args.dataset_dir, opts, args.targets, report)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(records, f)
    if args.report:
        with open(args.report, "w") as f:
            json.dump({"opts": asdict(opts), "frames": report}, f, indent=1)
    print(f"{args.output}: {len(records)} proposals of {len(report)} frames")


if __name__ == "__main__":
    main()
