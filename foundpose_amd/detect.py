"""Detections for infer from a segmenter's raw mask proposals.

    python -m foundpose_amd.detect onboard --opts detect.json --output-path <root>
        reads <root>/templates/<templates_version>/<dataset>/<lid>/ (what gen_templates wrote) and writes detector.pth beside
        <root>/object_repre/<version>/<dataset>/<lid>/repre.pth, for every object of object_lids; with detector_score_type
        "semantic_appearance"  also detector_patches.pth, the templates' patch descriptors, which run then loads
    python -m foundpose_amd.detect run --opts detect.json --proposals proposals.json --dataset-dir <split> --output-path <root> --output detections.json
        labels the proposals of every image they name and writes a CNOS detections file (what infer --detections takes) and
        detector-decisions.json beside it; --proposals-from-depth [opts.json] in place of --proposals segments the split's depth images
        in process (depth_proposals.proposals_for_split) and labels those

proposals.json is a list of CNOS-shaped records {scene_id, image_id, segmentation (COCO RLE), time}; category_id, score and bbox, if
present, are ignored."""

import argparse
import json
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import detect_util, feature_util, gen_repre, repre_util


def _repre_dir(output_path: str, opts: detect_util.DetectOpts, lid: int) -> str:
    return repre_util.get_object_repre_dir_path(os.path.join(output_path, "object_repre"), opts.version, opts.object_dataset, lid)


def _load_templates(metadata: Sequence[Dict[str, Any]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The template images and masks the metadata points at -> (uint8 [T, 3, h, w], uint8 [T, h, w]) on the host, read as gen_repre does."""
    rgb, masks = [], []
    for s in metadata:
        img = gen_repre._load_image(s["rgb_image_path"])
        if img.ndim == 2:
            img = np.stack([img] * 3, -1)
        rgb.append(torch.from_numpy(np.array(img[..., :3])).permute(2, 0, 1))
        m = gen_repre._load_image(s["binary_mask_path"])
        masks.append(torch.from_numpy(np.array((m if m.ndim == 2 else m[..., 0]) != 0).astype(np.uint8)))
    return torch.stack(rgb), torch.stack(masks)


def onboard(opts: detect_util.DetectOpts, output_path: str, extractor, templates: Optional[Dict[int, Dict[str, Any]]] = None) -> List[str]:
    """detector.pth for every object of opts.object_lids.  templates: gen_templates.synthesize_templates(return_templates=True)'s result
    instead of the PNGs.  -> the files written."""
    if not opts.object_lids:
        raise ValueError("object_lids names the objects to onboard")
    written = []
    for lid in opts.object_lids:
        if templates is not None:
            rgb, masks = templates[lid]["rgb"], templates[lid]["mask"]
        else:
            rgb, masks = _load_templates(gen_repre.load_template_metadata(output_path, opts, lid))
        bank = detect_util.build_detector_bank(extractor, rgb.cuda(), masks.cuda(), opts.detector_crop_size, opts.detector_template_stride,
                                               opts.detector_batch, with_patches=opts.detector_score_type == "semantic_appearance")
        written.append(detect_util.save_detector_bank(bank, _repre_dir(output_path, opts, lid)))
    return written


def load_banks(opts: detect_util.DetectOpts, output_path: str, lids: Optional[Sequence[int]] = None) -> Dict[int, Dict[str, Any]]:
    lids = list(lids if lids is not None else (opts.object_lids or []))
    if not lids:
        raise ValueError("object_lids names the objects to detect")
    with_patches = opts.detector_score_type == "semantic_appearance"
    return {lid: detect_util.load_detector_bank(_repre_dir(output_path, opts, lid), with_patches=with_patches) for lid in lids}


def _load_frame_image(split_dir: str, sid: int, iid: int) -> np.ndarray:
    from PIL import Image
    sdir = os.path.join(split_dir, f"{sid:06d}")
    paths = (os.path.join(sdir, "rgb", f"{iid:06d}.png"), os.path.join(sdir, "rgb", f"{iid:06d}.jpg"), os.path.join(sdir, "gray", f"{iid:06d}.tif"))
    path = next((p for p in paths if os.path.exists(p)), None)
    if path is None:
        raise FileNotFoundError(f"no image of scene {sid} image {iid} under {sdir}")
    return np.asarray(Image.open(path).convert("RGB"))


def run(opts: detect_util.DetectOpts, proposals: Sequence[Dict[str, Any]], split_dir: str, banks, extractor, output: str) -> Tuple[str, str]:
    """Labels the proposals image by image (in the order of each image's first proposal) and writes `output` (the detections list) and
    detector-decisions.json beside it.  -> the two paths."""
    bs = banks if isinstance(banks, detect_util.BankSet) else detect_util.bank_set(banks)
    by_image: Dict[Tuple[int, int], List[int]] = {}
    for i, p_ in enumerate(proposals):
        by_image.setdefault((int(p_["scene_id"]), int(p_["image_id"])), []).append(i)
    records, decisions = [], []
    for (sid, iid), members in by_image.items():
        dets, decs = detect_util.label_proposals(opts, _load_frame_image(split_dir, sid, iid), [proposals[i] for i in members], bs, extractor)
        records.extend(detect_util.detections_to_list(dets))
        decisions.extend(dict(d, scene_id=sid, image_id=iid, proposal=members[d["proposal"]],
                              suppressed_by=members[d["suppressed_by"]] if d["suppressed_by"] >= 0 else -1) for d in decs)
    os.makedirs(os.path.dirname(os.path.abspath(output)), exist_ok=True)
    with open(output, "w") as f:
        json.dump(records, f)
    dec_path = os.path.join(os.path.dirname(os.path.abspath(output)), "detector-decisions.json")
    with open(dec_path, "w") as f:
        json.dump(decisions, f, indent=1)
    return output, dec_path


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("onboard", "run"):
        sp = sub.add_parser(name)
        sp.add_argument("--opts", required=True, help="options JSON ({'detect_opts': {...}})")
        sp.add_argument("--output-path", required=True, help="root holding templates/ and object_repre/")
        sp.add_argument("--precision", default="bf16", choices=["bf16", "f16", "f16x3", "f16f8", "fp32"])
        sp.add_argument("--weights", default=None, help="DINOv2 checkpoint file or directory; default $FOUNDPOSE_DINOV2_WEIGHTS, then the torch hub "
                        "cache; without one the run fails (no random-weight fallback)")
        if name == "run":
            src = sp.add_mutually_exclusive_group(required=True)
            src.add_argument("--proposals", help="the segmenter's proposals: a JSON list of {scene_id, image_id, segmentation, time}")
            src.add_argument("--proposals-from-depth", nargs="?", const="", default=None, metavar="OPTS_JSON",
                             help="segment the split's depth images instead (depth_proposals, DESIGN.md section 28); the optional file "
                             "holds {'depth_proposal_opts': {...}}")
            sp.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
            sp.add_argument("--output", required=True, help="the detections file to write; detector-decisions.json goes beside it")
    args = ap.parse_args(argv)
    opts = detect_util.load_opts(args.opts)
    extractor = feature_util.make_feature_extractor(opts.detector_extractor_name, precision=args.precision, weights=args.weights).to("cuda")
    if args.command == "onboard":
        print("\n".join(onboard(opts, args.output_path, extractor)))
        return
    if args.proposals is not None:
        with open(args.proposals) as f:
            proposals = json.load(f)
    else:
        from . import depth_proposals
        proposals = depth_proposals.proposals_for_split(args.dataset_dir, args.proposals_from_depth or None)
    # (the set holds its own copy of every table: the per-object ones are dropped as soon as it is built -- 6.7 GB of patch tables at 8 x 798
    #  templates of ViT-L -- and only while bank_set concatenates them does the device hold both)
    bs = detect_util.bank_set(load_banks(opts, args.output_path))
    print("\n".join(run(opts, proposals, args.dataset_dir, bs, extractor, args.output)))


if __name__ == "__main__":
    main()
