"""CPU: the host logic of the frame-major, cross-object driver (infer.infer_batched): which detections form a
batch (iter_batches), how a batch is laid out for the engine (plan_flush), and what is refused before any device work."""
import pytest

from foundpose_amd import infer
from foundpose_amd.infer import QueuedDetection as Q

BIG, SMALL = (640, 480), (320, 240)
# 3 frames, 3 objects (indices 0..2), in the order the driver queues them: frame by frame, objects ascending, instances in order.
# frame 0: object 0 twice, object 2; frame 1: objects 1 and 2; frame 2 (another size): objects 0 and 1.
STREAM = [Q(0, BIG, 0, 0), Q(0, BIG, 0, 1), Q(0, BIG, 2, 0),
          Q(1, BIG, 1, 0), Q(1, BIG, 2, 0),
          Q(2, SMALL, 0, 0), Q(2, SMALL, 1, 0)]


def _ids(batches):
    return [[STREAM.index(e) for e in b] for b in batches]


def test_plan_flush_orders_by_object_and_keeps_frame_and_group():
    queue = STREAM[:5]
    plan = infer.plan_flush(queue)
    assert plan.det_obj == [0, 0, 1, 2, 2]                       # ascending
    assert plan.order == [0, 1, 3, 2, 4]                         # stable: within an object the queue's frame / instance order
    assert plan.frames == [0, 1]
    assert plan.image_index == [0, 0, 1, 0, 1]                   # each row reads its own frame's image
    assert plan.pair_group_index == [0, 1, 0, 0, 0]              # restarts per (frame, object): only the second instance of (0, 0) has 1
    # a batch that starts in the middle of a group: the group index is the detection's, not its position in the batch
    plan = infer.plan_flush(STREAM[1:4])
    assert plan.order == [0, 2, 1] and plan.det_obj == [0, 1, 2] and plan.image_index == [0, 1, 0] and plan.pair_group_index == [1, 0, 0]
    assert plan.frames == [0, 1]
    # frames need not start at 0 in a later batch
    plan = infer.plan_flush(STREAM[3:5])
    assert plan.frames == [1] and plan.image_index == [0, 0] and plan.det_obj == [1, 2]
    empty = infer.plan_flush([])
    assert empty.order == [] and empty.frames == []


@pytest.mark.parametrize("n", [1, 3])
def test_single_group_plan_is_plan_flush_of_one_frame_and_one_object(n):
    """The per-object driver's plan: its queue is one (frame 0, object 0) group, and plan_flush of that queue is what it passes on."""
    queue = [Q(0, BIG, 0, i, inst_id=5 + i) for i in range(n)]
    assert infer.single_group_plan(n) == infer.plan_flush(queue)


def test_iter_batches_flush_rule():
    assert _ids(infer.iter_batches(iter(STREAM), 4)) == [[0, 1, 2, 3], [4], [5, 6]]     # full batch straddling frames; size change; end of stream
    assert _ids(infer.iter_batches(iter(STREAM), 1)) == [[i] for i in range(7)]
    assert _ids(infer.iter_batches(iter(STREAM), 64)) == [[0, 1, 2, 3, 4], [5, 6]]      # larger than the stream: the size change still flushes
    assert _ids(infer.iter_batches(iter(STREAM[:5]), 64)) == [[0, 1, 2, 3, 4]]
    assert _ids(infer.iter_batches(iter(STREAM), 5)) == [[0, 1, 2, 3, 4], [5, 6]]       # no empty batch when a full one meets the size change
    assert list(infer.iter_batches(iter([]), 8)) == []
    with pytest.raises(ValueError):
        list(infer.iter_batches(iter(STREAM), 0))


def test_iter_batches_reads_no_further_than_the_batch_it_fills():
    seen = []

    def stream():
        for e in STREAM:
            seen.append(e)
            yield e
    it = infer.iter_batches(stream(), 2)
    assert len(next(it)) == 2 and len(seen) == 2      # frames behind the batch are not loaded yet (and the flushed ones can go)


def test_batched_driver_refusals_come_before_any_device_work():
    base = dict(version="v", repre_version="r", object_dataset="lmo")
    ok = infer.InferOpts(**base)
    for n in (0, -3):
        with pytest.raises(ValueError, match="batch_detections"):
            infer.infer_batched(ok, [], {}, {}, "unused", batch_detections=n)
    with pytest.raises(NotImplementedError, match="per-object driver"):
        infer.infer_batched(ok, [], {}, {}, "unused", renderer=object())
    # what the per-object driver refuses (tests/test_cabi_symbols.py) is refused here too
    for bad, exc in ((dict(max_num_queries=500), NotImplementedError),
                     (dict(match_template_type="sift"), ValueError), (dict(match_feat_matching_type="1nn"), ValueError),
                     (dict(final_pose_type="refined"), ValueError), (dict(final_pose_type="featuremetric", refine_iters=-1), ValueError)):
        with pytest.raises(exc):
            infer.infer_batched(infer.InferOpts(**base, **bad), [], {}, {}, "unused")


def test_cli_refuses_pictures_in_batched_mode_at_argument_time(capsys):
    argv = ["--opts", "/nonexistent/opts.json", "--dataset-dir", "/nonexistent", "--detections", "/nonexistent.json", "--repre-dir", "/nonexistent",
            "--output-dir", "/nonexistent/out"]
    with pytest.raises(SystemExit) as e:        # argparse's error exit, before the options file (which does not exist) is opened
        infer.main(argv + ["--batch-detections", "4", "--vis"])
    assert e.value.code == 2 and "per-object driver" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        infer.main(argv + ["--batch-detections", "-1"])
    with pytest.raises(FileNotFoundError):      # accepted by the parser: the run gets as far as the options file
        infer.main(argv + ["--batch-detections", "4"])


def test_load_bop_frames_all_yields_each_image_once(tmp_path):
    import json
    import numpy as np
    from PIL import Image
    split = tmp_path / "test"
    for sid, ims in ((1, (3, 4)), (2, (3,))):
        (split / f"{sid:06d}" / "rgb").mkdir(parents=True)
        (split / f"{sid:06d}" / "scene_camera.json").write_text(json.dumps({str(i): {"cam_K": [500.0, 0, 16, 0, 510.0, 12, 0, 0, 1]} for i in ims}))
        for i in ims:
            Image.fromarray(np.full((24, 32, 3), sid * 10 + i, np.uint8)).save(split / f"{sid:06d}" / "rgb" / f"{i:06d}.png")
    targets = [{"scene_id": 1, "im_id": 3, "obj_id": 1, "inst_count": 1}, {"scene_id": 1, "im_id": 3, "obj_id": 2, "inst_count": 2},
               {"scene_id": 1, "im_id": 4, "obj_id": 2, "inst_count": 1}, {"scene_id": 2, "im_id": 3, "obj_id": 1, "inst_count": 1},
               {"scene_id": 1, "im_id": 4, "obj_id": 5, "inst_count": 1}]
    frames = list(infer.load_bop_frames_all(str(split), targets))
    assert [(f["scene_id"], f["im_id"]) for f in frames] == [(1, 3), (1, 4), (2, 3)]
    assert [int(f["image"][0, 0, 0]) for f in frames] == [13, 14, 23] and frames[0]["camera"].f == (500.0, 510.0) and "gt_annos" not in frames[0]
    # the per-object loader still yields an object's frames in target order, with the same content
    per = list(infer.load_bop_frames(str(split), targets, 2))
    assert [(f["scene_id"], f["im_id"]) for f in per] == [(1, 3), (1, 4)] and np.array_equal(per[1]["image"], frames[1]["image"])
