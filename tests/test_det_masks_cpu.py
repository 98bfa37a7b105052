"""The host side of the device mask path, no GPU needed: infer_pose_util.pack_rle, the refusals that come before any
launch, the CLI's refusal of --device-masks without the batched driver, and the decode rule of fp_detection_masks restated in numpy against
infer_pose_util.rle_to_binary_mask."""
import numpy as np
import pytest

from foundpose_amd import infer, infer_pose_util as ipu


def _compress(counts):
    """COCO's string form of a counts list (pycocotools rleToString), the inverse of ipu._decode_compressed_counts."""
    out = []
    for i, x in enumerate(counts):
        x = int(x) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
    return "".join(out)


def _det(counts, size=(6, 8)):
    return {"bbox": [0, 0, 1, 1], "score": 1.0, "time": 0.0, "segmentation": {"counts": counts, "size": list(size)}}


A, B, C = [5, 3, 40], [0, 48], [7, 1, 1, 2, 30, 4, 3]


def test_pack_rle_lists_strings_and_a_mix():
    assert ipu._decode_compressed_counts(_compress(C)) == C and ipu._decode_compressed_counts(_compress(A)) == A
    for dets in ([_det(A), _det(B), _det(C)], [_det(_compress(A)), _det(_compress(B)), _det(_compress(C))],
                 [_det(A), _det(_compress(B).encode()), _det(_compress(C))]):
        counts, run_off, size = ipu.pack_rle(dets)
        assert counts.dtype == np.int32 and run_off.dtype == np.int32 and size == (6, 8)
        assert counts.tolist() == A + B + C and run_off.tolist() == [0, 3, 5, 12]
    counts, run_off, size = ipu.pack_rle([_det(A)["segmentation"]])     # the RLE dict itself
    assert counts.tolist() == A and run_off.tolist() == [0, 3] and size == (6, 8)
    counts, run_off, _ = ipu.pack_rle([_det([]), _det(A)])              # a detection without runs: an empty mask
    assert counts.tolist() == A and run_off.tolist() == [0, 0, 3]


def test_pack_rle_refusals():
    with pytest.raises(ValueError, match="negative"):
        ipu.pack_rle([_det(A), _det([4, -1, 10])])
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        ipu.pack_rle([_det([2**30, 2**30], size=(1, 1))])
    ipu.pack_rle([_det([2**30, 2**30 - 1], size=(1, 1))])               # 2^31 - 1 itself is fine
    with pytest.raises(ValueError, match="one size at a time"):
        ipu.pack_rle([_det(A), _det(A, size=(8, 6))])
    with pytest.raises(ValueError, match="no detection"):
        ipu.pack_rle([])


def test_refusals_come_before_any_device_call(monkeypatch):
    """An image larger than the canvas and an odd difference are both refused before anything touches the device: with ops.detection_masks
    and the upload replaced by functions that fail, the ValueError still is what comes out."""
    from foundpose_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(ops, "detection_masks", boom)
    monkeypatch.setattr(_lib, "upload_async", boom)
    preds = {1: [_det([48], size=(6, 8))]}
    with pytest.raises(ValueError, match="Image is larger than mask."):
        ipu.instances_on_device(preds, (10, 6))
    with pytest.raises(ValueError, match="Image is larger than mask."):
        ipu.instances_on_device(preds, (8, 8))
    for size_wh in ((7, 6), (8, 5), (5, 3)):
        with pytest.raises(ValueError, match="odd number of pixels"):
            ipu.instances_on_device(preds, size_wh)
    # a good detection of another canvas in the same frame does not get launched first
    with pytest.raises(ValueError, match="odd number of pixels"):
        ipu.instances_on_device({1: [_det([80], size=(8, 10))], 2: [_det([54], size=(6, 9))]}, (6, 4))
    assert ipu.instances_on_device({1: [], 2: []}, (8, 6)) == {1: [], 2: []}     # nothing to do: nothing launched either


def test_cli_refuses_device_masks_without_the_batched_driver(capsys):
    argv = ["--opts", "/nonexistent/opts.json", "--dataset-dir", "/nonexistent", "--detections", "/nonexistent.json", "--repre-dir", "/nonexistent",
            "--output-dir", "/nonexistent/out", "--device-masks"]
    for extra in ([], ["--batch-detections", "0"]):
        with pytest.raises(SystemExit) as e:
            infer.main(argv + extra)
        assert e.value.code == 2 and "--device-masks needs the batched driver" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):      # with a batch size the flag is accepted: the run gets as far as reading the options
        infer.main(argv + ["--batch-detections", "4"])


def _decode_rule(counts, hc, wc):
    """fp_detection_masks' decode: pixel (x, y) has p = x hc + y; k = #{s_i <= p}; set iff k < R and k odd."""
    s = np.cumsum(np.asarray(counts, np.int64))
    p = np.arange(wc)[None, :] * hc + np.arange(hc)[:, None]
    k = np.searchsorted(s, p, side="right")
    return (k < len(counts)) & (k % 2 == 1)


def test_decode_rule_equals_rle_to_binary_mask():
    rng = np.random.default_rng(19)
    for case in range(400):
        hc, wc = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        n_runs = int(rng.integers(0, 14))
        counts = rng.integers(0, 9, n_runs)
        counts[rng.random(n_runs) < 0.25] = 0                 # zero runs, leading ones included
        if case % 4 == 0 and n_runs:                           # a total beyond the canvas
            counts[int(rng.integers(0, n_runs))] += hc * wc
        want = ipu.rle_to_binary_mask({"counts": counts.tolist(), "size": [hc, wc]})
        assert np.array_equal(_decode_rule(counts.tolist(), hc, wc), want), (hc, wc, counts.tolist())
    for counts in ([48], [0, 48], [10], [0, 0, 5], [3, 0, 0, 4, 2], [50], [0, 100]):
        assert np.array_equal(_decode_rule(counts, 6, 8), ipu.rle_to_binary_mask({"counts": counts, "size": [6, 8]})), counts
