"""GPU: eval_add.evaluate_add end to end on a BOP tree written to tmp_path (synthetic.make_bop_eval_scene: 3 images, 2 objects, both in every
image, one instance each).  The expected scores come from the numpy restatement (tests/pose_add_ref.py) run on the error table the device
computed, and are compared with ==: the errors themselves are pinned by tests/test_gpu_pose_add.py."""

import json
import os
import shutil

import numpy as np
import pytest

from foundpose_amd import eval_add, synthetic
from tests import pose_add_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("recall_add_s", "auc_add", "auc_adi", "auc_add_s")


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("add_eval"))
    sc = synthetic.make_bop_eval_scene(root, num_images=3, num_objects=2, gts_per_image=2, mesh_res=24)
    sc["root"] = root
    return sc


def _rows(sc, move=None, skip=()):
    """The GT poses as estimates, each changed by move(obj_id, T) -> T."""
    out = []
    for im, inst in sc["images"]:
        for lid, T in inst:
            if (im, lid) not in skip:
                out.append((1, im, lid, 0.9 - 0.01 * im, np.array(T, np.float64) if move is None else move(lid, np.array(T, np.float64)), 0.5))
    return out


def _shift(sc, fraction):
    def move(lid, T):
        T[:3, 3] += [fraction * sc["diameters"][lid], 0.0, 0.0]
        return T
    return move


def _turn(lid, T):
    """A quarter turn of the model about its z axis: far by ADD, nearer by ADI."""
    T[:3, :3] = T[:3, :3] @ np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return T


def _evaluate(sc, name, estimates, targets=None, **kw):
    path = os.path.join(sc["root"], name + ".csv")
    synthetic.write_bop_results_csv(path, estimates)
    return eval_add.evaluate_add(path, sc["split_dir"], sc["targets"] if targets is None else targets, sc["models_dir"], **kw)


def _check_restated(out):
    """The restatement's scores from the tables of a details=True run equal the module's, number by number."""
    s = ref.summarize(out["tables"], out["recall_factor"], out["auc_max_mm"])
    assert {k: out[k] for k in KEYS} == s["mean"] and out["all_instances"] == s["all"]
    for lid, po in s["per_object"].items():
        assert {k: out["per_object"][str(lid)][k] for k in KEYS} == po
    return s


def _scores(out):
    return {k: v for k, v in out.items() if k != "tables"}


def test_the_gt_poses_score_one(scene):
    out = _evaluate(scene, "gt", _rows(scene), details=True)
    assert out["recall_add_s"] == out["auc_add"] == out["auc_adi"] == out["auc_add_s"] == 1.0
    assert out["all_instances"] == {k: 1.0 for k in KEYS}
    assert out["num_targets"] == 6 and out["num_valid_gt_instances"] == 6 and out["num_estimates_evaluated"] == 6 and out["num_pairs"] == 6
    assert out["tables"]["err"].shape == (6, 2) and np.all(out["tables"]["err"] == 0.0)      # every matched error is exactly 0
    assert all(np.all(e == 0.0) and e.shape == (3, 3) for e in out["tables"]["instance_errors"].values())
    assert sorted(out["per_object"]) == ["1", "2"] and out["symmetric_objects"] == []
    assert all(po["error_type"] == "add" and po["num_valid_instances"] == 3 for po in out["per_object"].values())
    _check_restated(out)
    json.dumps(_scores(out))                                                                  # what main() writes


@pytest.mark.parametrize("fraction, recall", [(0.05, 1.0), (0.2, 0.0)])
def test_shifted_estimates_equal_the_restatement(scene, fraction, recall):
    out = _evaluate(scene, f"shift_{fraction}", _rows(scene, _shift(scene, fraction)), details=True)
    assert out["recall_add_s"] == recall == out["all_instances"]["recall_add_s"]
    _check_restated(out)
    # a pure translation: ADD is its length, ADI at most that; both curves lie strictly between 0 and 1
    err = out["tables"]["err"]
    diam = np.array([scene["diameters"][t["obj_id"]] for t in out["tables"]["targets"]])
    assert np.allclose(err[:, 0], fraction * diam, rtol=1e-12) and np.all(err[:, 1] <= err[:, 0]) and np.all(err[:, 1] > 0)
    assert 0.0 < out["auc_add"] < 1.0 and out["auc_add"] == out["auc_add_s"] and out["auc_adi"] >= out["auc_add"]
    # a wider factor turns the far estimates into correct ones
    if fraction == 0.2:
        assert _evaluate(scene, f"shift_{fraction}", _rows(scene, _shift(scene, fraction)), recall_factor=0.25)["recall_add_s"] == 1.0


def test_symmetric_ids_switch_that_object_to_adi_only(scene, tmp_path):
    rows = _rows(scene, _turn)
    base = _evaluate(scene, "turn", rows, details=True)
    sym = _evaluate(scene, "turn", rows, details=True, symmetric_ids=[2])
    _check_restated(base)
    _check_restated(sym)
    assert np.array_equal(base["tables"]["err"], sym["tables"]["err"]) and sym["symmetric_objects"] == [2]
    assert sym["per_object"]["1"] == base["per_object"]["1"] and base["per_object"]["1"]["error_type"] == "add"
    b2, s2 = base["per_object"]["2"], sym["per_object"]["2"]
    assert s2["error_type"] == "adi" and b2["error_type"] == "add"
    assert b2["auc_add_s"] == b2["auc_add"] and s2["auc_add_s"] == s2["auc_adi"] == b2["auc_adi"] and s2["auc_add"] == b2["auc_add"]
    assert s2["auc_adi"] > s2["auc_add"]                          # the turn is what the two metrics disagree about
    # the same through models_info.json: a discrete symmetry listed for object 2
    models = str(tmp_path / "models")
    shutil.copytree(scene["models_dir"], models)
    info = json.load(open(os.path.join(models, "models_info.json")))
    info["2"]["symmetries_discrete"] = [np.diag([-1.0, -1.0, 1.0, 1.0]).ravel().tolist()]
    info["1"]["symmetries_discrete"] = []
    json.dump(info, open(os.path.join(models, "models_info.json"), "w"))
    via_info = eval_add.evaluate_add(os.path.join(scene["root"], "turn.csv"), scene["split_dir"], scene["targets"], models)
    assert _scores(via_info) == _scores(sym)


def test_a_missing_estimate_enters_as_inf(scene):
    ims = [im for im, _ in scene["images"][:2]]
    targets = [t for t in scene["targets"] if t["im_id"] in ims]                 # two images, four instances
    lost = (ims[1], scene["images"][1][1][0][0])
    out = _evaluate(scene, "missing", _rows(scene, skip={lost}), targets=targets, details=True)
    assert out["num_targets"] == 4 and out["num_valid_gt_instances"] == 4 and out["num_estimates_evaluated"] == 3
    inst = out["tables"]["instance_errors"]
    assert sorted(np.concatenate([e[:, 2] for e in inst.values()]).tolist()) == [0.0, 0.0, 0.0, np.inf]
    # errors (0, 0, 0, inf): three of four are correct, and the accuracy curve stands at 3/4 over the whole range -> 0.75; per object
    # (0, inf) -> 0.5 and (0, 0) -> 1.0, whose mean is 0.75 again
    assert out["all_instances"] == {k: 0.75 for k in KEYS} and {k: out[k] for k in KEYS} == {k: 0.75 for k in KEYS}
    assert sorted(po["auc_add_s"] for po in out["per_object"].values()) == [0.5, 1.0]
    _check_restated(out)


def test_other_rows_and_other_target_keys_change_nothing_and_the_tool_writes_the_same(scene, tmp_path):
    rows = _rows(scene, _shift(scene, 0.05))
    base = _evaluate(scene, "base", rows)
    # rows of an image or an object that is no target are left out; a second, lower-scored estimate of a target falls to inst_count = 1
    far = np.eye(4)
    far[:3, 3] = [0.0, 0.0, 5000.0]
    im0, lid0 = scene["images"][0][0], scene["images"][0][1][0][0]
    extra = _evaluate(scene, "extra", rows + [(1, 99, 1, 2.0, np.eye(4), 0.5), (7, 0, 2, 2.0, np.eye(4), 0.5), (1, im0, 55, 2.0, np.eye(4), 0.5),
                                               (1, im0, lid0, 0.01, far, 0.5)])
    assert _scores(extra) == _scores(base)
    # keys a targets file may carry besides the four that are read
    more = [dict(t, note="x", visib=0.3) for t in scene["targets"]]
    assert _scores(_evaluate(scene, "base", rows, targets=more)) == _scores(base)
    # the command line: the default targets file beside the split, the scores written as JSON
    out_path = str(tmp_path / "scores" / "add.json")
    eval_add.main(["--result-csv", os.path.join(scene["root"], "base.csv"), "--dataset-dir", scene["split_dir"], "--output", out_path])
    assert json.load(open(out_path)) == json.loads(json.dumps(_scores(base))) and base["dataset"] == "synth"
    eval_add.main(["--result-csv", os.path.join(scene["root"], "base.csv"), "--dataset-dir", scene["split_dir"], "--output", out_path,
                   "--symmetric-ids", "2", "--recall-factor", "0.01", "--auc-max", "50"])
    tool = json.load(open(out_path))
    assert tool == json.loads(json.dumps(_scores(_evaluate(scene, "base", rows, symmetric_ids=[2], recall_factor=0.01, auc_max=50.0))))
    assert tool["symmetric_objects"] == [2] and tool["recall_factor"] == 0.01 and tool["auc_max_mm"] == 50.0
