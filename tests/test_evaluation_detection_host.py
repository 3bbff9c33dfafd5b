"""Object and action detection evaluation, the parts that need no GPU: the conditions the g13 case must meet, the
pure-Python restatement (tests/detection_eval_reference.py) against the reference's own numbers (golden g13), the
package's host stage with the restatement standing in for the kernels, the packing layout, every error decided on the
host, the refusals of the two C entries, and the discipline of csrc/evalobj/ (kernel variant table, built sources, ISA
store lint, no probe blocks, no memset, no inline assembly, no spills)."""
import ast
import ctypes
import glob
import itertools
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import cases
import cases_detection_eval as cde
import detection_eval_reference as R
import evalobj_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_EO = os.path.join(PKG, "csrc", "evalobj")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_EO, "*.hip")) + glob.glob(os.path.join(CSRC_EO, "*.h")))
ENTRIES = {"tspn_evalobj_tiou_f64", "tspn_evalobj_claim"}
OBJECT_CONFIGS = [(True, 0.5, "07_0.5"), (True, 0.3, "07_0.3"), (False, 0.5, "voc_0.5"), (False, 0.3, "voc_0.3")]
_CACHE = {}


def _E():
    import tspn_mi355x
    return tspn_mi355x.evaluation


def _D():
    import tspn_mi355x
    return tspn_mi355x.evaluation_detection


def object_case():
    if "obj" not in _CACHE:
        _CACHE["obj"] = cde.g13_object_case()
    return _CACHE["obj"]


def action_case():
    if "act" not in _CACHE:
        _CACHE["act"] = cde.g13_action_case()
    return _CACHE["act"]


def restated_objects(m07=True, thr=0.5):
    if (m07, thr) not in _CACHE:
        _CACHE[(m07, thr)] = R.evaluate_objects(*object_case(), m07, thr)
    return _CACHE[(m07, thr)]


def assert_same(got, want):
    assert type(got) is type(want) and got == want, (got, type(got), want, type(want))


@pytest.fixture
def kernels_restated(monkeypatch):
    """The device stage of both evaluators answered by the restatement from the packed arrays, on the CPU."""
    D = _D()
    monkeypatch.setattr(D, "_resolve_device", lambda device: "cpu")

    def match_object_chunk(pk, thresh_t, dev, stats):
        _, best, index, flags = R.tiou_packed(pk)
        _, hit = R.claim_packed(pk, best, index, thresh_t)
        return best, index.astype(np.int64), flags, hit.astype(bool)
    monkeypatch.setattr(D, "_match_object_chunk", match_object_chunk)
    monkeypatch.setattr(D, "_match_chunk", lambda pk, thr, dev, stats: R.relation_match_packed(pk, thr))
    return D


# ---------------------------------------------------------------------------------------------------- the g13 case
def test_g13_case_meets_its_conditions():
    gt, pred = object_case()
    gt_classes = set(t["category"] for tracks in gt.values() for t in tracks)
    pred_classes = set(t["category"] for tracks in pred.values() for t in tracks)
    for c in pred_classes:
        scores = [t["score"] for tracks in pred.values() for t in tracks if t["category"] == c]
        assert len(set(scores)) == len(scores), f"scores of class {c} are not distinct"
    assert len(gt_classes) >= 4 and gt_classes - pred_classes and pred_classes - gt_classes
    _, _, per_pred = restated_objects()
    # a duplicate claim that is a false positive: qualifies, yet names a ground truth that an earlier one took
    assert sum(mo >= 0.5 and not tp for mo, _, tp in per_pred.values()) >= 1
    # a tIoU tie between two ground truths, on a prediction that overlaps them
    ties = 0
    for vid, tracks in pred.items():
        for t in tracks:
            rows = [R.tiou(R.int_keys(g["trajectory"]), R.int_keys(t["trajectory"]))
                    for g in gt.get(vid, []) if g["category"] == t["category"]]
            ties += len(rows) >= 2 and max(rows) > 0 and rows.count(max(rows)) >= 2
    assert ties >= 1
    # a (video, class) with predictions and no ground truth; frame sets with gaps; a video that only the predictions have
    assert any(t["category"] in gt_classes and all(g["category"] != t["category"] for g in gt[vid])
               for vid, tracks in pred.items() if vid in gt for t in tracks)
    assert any(np.diff(sorted(int(k) for k in g["trajectory"])).max() > 1
               for tracks in gt.values() for g in tracks if len(g["trajectory"]) > 1)
    assert set(pred) - set(gt) and set(gt) - set(pred)
    agt, apred = action_case()
    assert any(vid not in agt for vid in apred)                     # an action prediction in a video absent from gt
    a_gt = set(t["category"] for tracks in agt.values() for t in tracks)
    a_pred = set(t["category"] for tracks in apred.values() for t in tracks)
    assert len(a_gt) >= 4 and a_gt - a_pred and a_pred - a_gt
    scores = [t["score"] for tracks in apred.values() for t in tracks]
    assert len(set(scores)) < len(scores)                           # equal scores: the stable order matters
    # the reference averages over a set of strings: the mean must not depend on its order
    for thr in (0.5, 0.7):
        ap = R.evaluate_actions(agt, apred, thr)[1]
        assert len(set(float(np.mean(list(p))) for p in itertools.permutations(ap.values()))) == 1


@pytest.mark.parametrize("m07,thr,name", OBJECT_CONFIGS)
def test_restatement_equals_g13_objects(m07, thr, name):
    g = cases.load("g13_detection_eval.npz")
    gt, pred = object_case()
    mean_ap, ap_class, per_pred = restated_objects(m07, thr)
    assert mean_ap == g[f"obj/{name}/mean_ap"][()] and isinstance(mean_ap, np.floating) == bool(g[f"obj/{name}/mean_ap_is_np"])
    assert [c for c, _ in ap_class] == list(g[f"obj/{name}/categories"])
    assert [ap for _, ap in ap_class] == list(g[f"obj/{name}/ap"])
    assert [isinstance(ap, np.floating) for _, ap in ap_class] == list(g[f"obj/{name}/ap_is_np"])
    gt_classes = set(t["category"] for tracks in gt.values() for t in tracks)
    keys = [(vid, i) for vid, tracks in pred.items() for i, t in enumerate(tracks) if t["category"] in gt_classes]
    assert [per_pred[k][0] for k in keys] == list(g["obj/max_overlap"])
    assert [per_pred[k][1] for k in keys] == list(g["obj/max_index"])


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_restatement_equals_g13_actions(thr):
    g = cases.load("g13_detection_eval.npz")
    mean_ap, ap_class, curves = R.evaluate_actions(*action_case(), thr)
    assert type(mean_ap) is np.float64 and mean_ap == g[f"act/{thr}/mean_ap"][()]
    cats = list(g[f"act/{thr}/categories"])
    assert sorted(ap_class) == cats and [ap_class[c] for c in cats] == list(g[f"act/{thr}/ap"])
    assert [isinstance(ap_class[c], np.floating) for c in cats] == list(g[f"act/{thr}/ap_is_np"])
    assert sorted(curves) == [c for c in cats if f"act/{thr}/{c}/prec" in g] and len(curves) >= 4
    for c, got in curves.items():
        for a, name in zip(got, ("prec", "rec", "hit_scores")):
            want = g[f"act/{thr}/{c}/{name}"]
            assert a.dtype == want.dtype and np.array_equal(a, want), (c, name)


def test_annotation_readers_equal_the_reference():
    g = cases.load("g13_detection_eval.npz")
    anno = cde.g13_annotation()
    E = _E()
    assert json.dumps(E.object_instances(anno)) == str(g["anno/object_insts_json"])
    assert json.dumps(E.action_instances(anno, cde.ACTION_PREDICATES)) == str(g["anno/action_insts_json"])
    insts = E.action_instances(anno, cde.ACTION_PREDICATES)
    assert [a["category"] for a in insts] == ["left", "chase", "chase"]
    assert [len(a["trajectory"]) for a in insts] == [6, 5, 4]          # the subject of the last is missing in frame 7
    assert E.action_instances(anno, []) == [] and {o["tid"] for o in E.object_instances(anno)} == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------- the host stage
@pytest.mark.parametrize("m07,thr,name", OBJECT_CONFIGS)
def test_evaluate_objects_with_the_restatement_as_the_kernels_equals_g13(kernels_restated, m07, thr, name):
    g = cases.load("g13_detection_eval.npz")
    gt, pred = object_case()
    got = kernels_restated.evaluate_objects(gt, pred, use_07_metric=m07, thresh_t=thr, details=True, max_candidates=40)
    want = restated_objects(m07, thr)
    assert_same(got[0], want[0])
    assert got[0] == g[f"obj/{name}/mean_ap"][()]
    assert [c for c, _ in got[1]] == [c for c, _ in want[1]]
    for (_, a), (_, b) in zip(got[1], want[1]):
        assert_same(a, b)
    assert list(got[2]) == list(pred)
    n = 0
    for vid, d in got[2].items():
        for pos, i in enumerate(d["order"].tolist()):
            of_class = [k for k, q in enumerate(gt.get(vid, [])) if q["category"] == pred[vid][i]["category"]]
            if of_class:
                mo, mi, tp = want[2][(vid, i)]
                assert (d["tiou"][pos], d["match"][pos], d["hit"][pos]) == (mo, of_class[mi], tp)
                n += 1
            else:
                assert (d["tiou"][pos], d["match"][pos], d["hit"][pos]) == (0.0, -1, False)
    assert n > 200


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_evaluate_actions_with_the_restatement_as_the_kernels_equals_g13(kernels_restated, thr):
    g = cases.load("g13_detection_eval.npz")
    gt, pred = action_case()
    stats = {}
    got = kernels_restated.evaluate_actions(gt, pred, viou_threshold=thr, details=True, max_candidates=10, stats=stats)
    want = R.evaluate_actions(gt, pred, thr)
    assert stats["chunks"] >= 3
    assert_same(got[0], want[0])
    assert got[0] == g[f"act/{thr}/mean_ap"][()] and list(got[1]) == list(want[1])
    for c in want[1]:
        assert_same(got[1][c], want[1][c])
    for c, curves in want[2].items():
        for a, b in zip(got[2]["classes"][c], curves):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    assert list(got[2]["videos"]) == list(pred)


def test_array_pairs_and_unsorted_keys_give_the_dict_result(kernels_restated):
    gt, pred = object_case()
    as_pairs = {vid: [dict(t, trajectory=(np.array([int(k) for k in t["trajectory"]], dtype=np.int32),
                                          np.array(list(t["trajectory"].values()), dtype=np.float64).reshape(-1, 4)))
                      for t in tracks] for vid, tracks in pred.items()}
    backwards = {vid: [dict(t, trajectory=dict(reversed(list(t["trajectory"].items())))) for t in tracks]
                 for vid, tracks in gt.items()}
    one = kernels_restated.evaluate_objects(gt, pred)
    assert kernels_restated.evaluate_objects(backwards, as_pairs) == one
    assert one[0] == restated_objects()[0]


def test_voc_ap_keyword_leaves_the_default_as_it_was():
    E = _E()
    rs = np.random.RandomState(0)
    for n in (1, 7, 40):
        tp = np.cumsum(rs.randint(0, 2, size=n)).astype(np.float64)
        rec, prec = tp / 9.0, tp / np.arange(1, n + 1)
        assert_same(E.voc_ap(rec, prec), R.voc_ap(rec, prec))
        assert_same(E.voc_ap(rec, prec, False), R.voc_ap(rec, prec, False))
        assert_same(E.voc_ap(rec, prec, use_07_metric=True), R.voc_ap(rec, prec, True))
    zero = np.zeros(3)
    assert type(E.voc_ap(zero, zero, True)) is np.float64 and type(E.voc_ap(zero - 1, zero, True)) is float
    import inspect
    assert list(inspect.signature(E.voc_ap).parameters) == ["rec", "prec", "use_07_metric"]
    assert inspect.signature(E.voc_ap).parameters["use_07_metric"].default is False
    sig = inspect.signature(E.evaluate_objects)
    assert list(sig.parameters) == ["groundtruth", "prediction", "use_07_metric", "thresh_t", "device", "max_candidates",
                                    "max_bytes", "details", "stats"]
    assert (sig.parameters["use_07_metric"].default, sig.parameters["thresh_t"].default) == (True, 0.5)
    assert list(inspect.signature(E.evaluate_actions).parameters)[:4] == ["groundtruth", "prediction", "viou_threshold", "device"]


# ---------------------------------------------------------------------------------------------------- packing
def test_object_packing_layout():
    D = _D()
    gt, pred = object_case()
    videos = D._prepare("t", gt, pred, *D._gt_classes(gt), True, D._object_rows, D._object_chunk_bytes)
    assert [v["vid"] for v in videos] == list(pred)
    pk = D._pack_objects(videos)
    traj, groups, frames, boxes = pk["traj"], pk["groups"], pk["frames"], pk["boxes"]
    assert boxes.dtype == np.float64 and boxes.shape == (pk["rows"], 4) and frames.dtype == np.int32
    assert frames.shape == (pk["rows"],) and traj.dtype == np.int64 and groups.dtype == np.int64
    assert np.array_equal(traj[:, 0], np.concatenate(([0], np.cumsum(traj[:-1, 1])))) and traj[:, 1].sum() == pk["rows"]
    for row, n in traj:
        assert (np.diff(frames[row:row + n]) > 0).all()
    assert np.array_equal(groups[:, 0], np.concatenate(([0], np.cumsum(groups[:-1, 1]))))
    assert np.array_equal(groups[:, 2], pk["n_pred"] + np.concatenate(([0], np.cumsum(groups[:-1, 3]))))
    assert np.array_equal(groups[:, 4], np.concatenate(([0], np.cumsum(groups[:-1, 1] * groups[:-1, 3]))))
    assert groups[:, 1].sum() == pk["n_pred"] and pk["n_pred"] + pk["n_gt"] == traj.shape[0] and (groups[:, 3] > 0).all()
    assert pk["candidates"] == int((groups[:, 1] * groups[:, 3]).sum())
    assert np.array_equal(pk["pred_group"], np.repeat(np.arange(len(groups)), groups[:, 1]))
    # predictions are in score order inside their group, and a packed row is the input's box of that frame
    for (p0, n, _, _, _), (v, p) in zip(groups, [(v, p) for v in videos for _, p, _ in v["groups"]]):
        sc = v["scores"][v["order"][p]]
        assert (np.diff(sc) <= 0).all() and np.array_equal(pk["pred_pos"][p0:p0 + n], p)
    v0 = videos[0]
    i = int(v0["order"][pk["pred_pos"][0]])
    t = pred[v0["vid"]][i]["trajectory"]
    row, n = traj[0]
    assert frames[row:row + n].tolist() == sorted(int(k) for k in t)
    assert boxes[row].tolist() == list(map(float, t[str(frames[row])]))
    # the cost _prepare predicts is what _pack_objects produces; chunks split by whole videos
    for v in videos:
        if v["groups"]:
            assert D._packed_object_bytes(D._pack_objects([v])) == v["bytes"]
    runs = list(_E()._chunks(videos, 40))
    assert [v["vid"] for r in runs for v in r] == list(pred) and len(runs) >= 4
    assert [len(r) for r in _E()._chunks(videos, 1 << 40, 1)] == [1] * len(videos)


def test_action_packing_stores_each_trajectory_once():
    D = _D()
    gt, pred = action_case()
    videos = D._prepare("t", gt, pred, *D._gt_classes(gt), False, D._action_rows, _E()._chunk_bytes)
    pk = D._pack_actions(videos)
    traj, groups = pk["traj"], pk["groups"]
    assert traj.shape[0] % 2 == 0 and np.array_equal(traj[0::2], traj[1::2])     # subject and object: the same rows
    one = traj[0::2]
    assert pk["rows"] == pk["boxes"].shape[0] == int((one[:, 2] - one[:, 1]).sum())
    assert np.array_equal(one[:, 0], np.concatenate(([0], np.cumsum(one[:-1, 2] - one[:-1, 1]))))
    n_inst = pk["n_pred"] + int(groups[:, 3].sum())
    assert traj.shape[0] == 2 * n_inst and pk["max_group_gt"] == groups[:, 3].max()
    packed = sum(len(p) for v in videos for _, p, _ in v["groups"])
    assert pk["n_pred"] == packed < sum(len(t) for t in pred.values())           # groups without ground truth stay out
    assert all(v["vid"] != "a_absent" or not v["groups"] for v in videos)
    assert np.array_equal(groups[:, 4], np.concatenate(([0], np.cumsum(groups[:-1, 1] * groups[:-1, 3]))))
    assert _E()._packed_bytes(pk) == sum(v["bytes"] for v in videos)


# ---------------------------------------------------------------------------------------------------- errors
def _obj(cat, traj, score=None):
    o = {"category": cat, "trajectory": traj}
    if score is not None:
        o["score"] = score
    return o


def test_object_errors_decided_on_the_host(kernels_restated):
    ev = kernels_restated.evaluate_objects
    box = (0, 0, 9, 9)
    gt = {"v": [_obj("a", {"0": box, "1": box})]}
    good = {"v": [_obj("a", {"0": box}, 0.5), _obj("a", {"1": box}, 0.25)]}
    assert ev(gt, good) == R.evaluate_objects(gt, good)[:2] and ev(gt, good, use_07_metric=False)[1] == [("a", 1.0)]
    with pytest.raises(ValueError, match="'v', prediction 1: non-finite score"):
        ev(gt, {"v": [_obj("a", {"0": box}, 0.5), _obj("a", {"1": box}, float("nan"))]})
    with pytest.raises(ValueError, match="'v', prediction 0: non-finite box"):
        ev(gt, {"v": [_obj("a", {"0": (0, 0, float("inf"), 9)}, 0.5)]})
    with pytest.raises(ValueError, match="'v', ground truth 0: non-finite box"):
        ev({"v": [_obj("a", {"0": (0, float("nan"), 9, 9)})]}, good)
    with pytest.raises(ValueError, match="'v', prediction 0: two keys of its trajectory are the same frame 1"):
        ev(gt, {"v": [_obj("a", {"1": box, "01": box}, 0.5)]})
    for bad in (2 ** 31, -2 ** 31 - 1, 2 ** 70):
        with pytest.raises(ValueError, match="'v', prediction 0: a frame id lies outside int32"):
            ev(gt, {"v": [_obj("a", {str(bad): box}, 0.5)]})
    with pytest.raises(ValueError, match="'v', prediction 0: trajectory must be"):
        ev(gt, {"v": [_obj("a", {"x": box}, 0.5)]})
    with pytest.raises(ValueError, match="'v', prediction 0: trajectory must have one 4-coordinate box per frame"):
        ev(gt, {"v": [_obj("a", (np.arange(3), np.zeros((2, 4))), 0.5)]})
    for bad in (0, 0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="thresh_t must be > 0"):
            ev(gt, good, thresh_t=bad)
    with pytest.raises(ValueError, match="max_candidates and max_bytes"):
        ev(gt, good, max_candidates=0)
    with pytest.raises(ValueError, match="max_candidates and max_bytes"):
        ev(gt, good, max_bytes=0)
    # as the reference: a predicted video of a ground-truth class that gt lacks, no ground-truth class at all
    with pytest.raises(KeyError, match="'w'"):
        ev(gt, {"w": [_obj("a", {"0": box}, 0.5)]})
    assert ev(gt, {"w": [_obj("other", {"0": box}, 0.5)], "v": good["v"]}, use_07_metric=False)[0] == 1.0
    with pytest.raises(ZeroDivisionError):
        ev({"v": []}, good)
    with pytest.raises(ZeroDivisionError):
        ev({}, {})
    # the two device flags, as the host reports them
    flat = (5, 5, 4, 4)
    with pytest.raises(ZeroDivisionError, match="'v', prediction 0: zero sIoU denominator"):
        ev({"v": [_obj("a", {"3": flat})]}, {"v": [_obj("a", {"3": flat}, 0.5)]})
    with pytest.raises(ZeroDivisionError, match="'v', prediction 1: no frame in it nor in"):
        ev({"v": [_obj("a", {})]}, {"v": [_obj("a", {"3": box}, 0.5), _obj("a", {}, 0.25)]})


def test_action_errors_and_edge_cases_decided_on_the_host(kernels_restated):
    ev = kernels_restated.evaluate_actions
    traj = [(0, 0, 9, 9)] * 3
    gt = {"v": [{"category": "run", "duration": (0, 3), "trajectory": traj}]}
    good = {"v": [{"category": "run", "duration": (0, 3), "trajectory": traj, "score": 0.5}]}
    assert ev(gt, good) == (1.0, {"run": 1.0})
    with pytest.raises(ValueError, match="'v', prediction 0: trajectory has 2 boxes for the duration"):
        ev(gt, {"v": [dict(good["v"][0], trajectory=traj[:2])]})
    with pytest.raises(ValueError, match="'v', ground truth 0: trajectory has 3 boxes for the duration"):
        ev({"v": [dict(gt["v"][0], duration=(0, 4))]}, good)
    with pytest.raises(ValueError, match="'v', prediction 0: non-finite score"):
        ev(gt, {"v": [dict(good["v"][0], score=float("-inf"))]})
    with pytest.raises(ValueError, match="'v', prediction 0: non-finite box"):
        ev(gt, {"v": [dict(good["v"][0], trajectory=[(0, 0, 9, float("nan"))] * 3)]})
    with pytest.raises(ValueError, match="'v', prediction 0: trajectory must be a list of 4-coordinate boxes"):
        ev(gt, {"v": [dict(good["v"][0], trajectory=[(0, 0, 9)] * 3)]})
    # a video that the ground truth lacks: false positives, no KeyError; an empty ground truth: nan, numpy's warning
    res = ev(gt, {"w": good["v"], "v": good["v"]})
    assert res == R.evaluate_actions(gt, {"w": good["v"], "v": good["v"]})[:2] and res[0] == 0.5
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        mean_ap, ap_class = ev({}, good)
    assert np.isnan(mean_ap) and ap_class == {} and any(issubclass(w.category, RuntimeWarning) for w in seen)


def test_there_is_no_cpu_path():
    E = _E()
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.evaluate_objects(*object_case(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.evaluate_actions(*action_case(), device="cpu")
    import tspn_mi355x
    ops = tspn_mi355x.ops
    z = torch.zeros
    args = [z((4, 4), dtype=torch.float64), z(4, dtype=torch.int32), z((2, 2), dtype=torch.int64),
            z((1, 5), dtype=torch.int64), z(1, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.evalobj_tiou(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.evalobj_claim(z(1, dtype=torch.float64), z(1, dtype=torch.int32), args[3], args[4], 1, 0.5)
    with pytest.raises(TypeError):
        ops.evalobj_tiou(args[0].numpy(), *args[1:])


def test_command_line_tool_reads_its_inputs(kernels_restated, tmp_path, monkeypatch, capsys):
    """tools/evaluate_detection.py on one annotation file, with the restatement in the kernels' place: the predicate file
    in both forms, the ground truth from the annotation readers, one line per category and the mean AP."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import evaluate_detection as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    (tmp_path / "p.json").write_text(json.dumps(list(cde.ACTION_PREDICATES)))
    (tmp_path / "p.txt").write_text("\n".join(cde.ACTION_PREDICATES) + "\n\n")
    assert tool.load_predicates(str(tmp_path / "p.json")) == tool.load_predicates(str(tmp_path / "p.txt")) \
        == list(cde.ACTION_PREDICATES)
    anno = cde.g13_annotation()
    del anno["relation_instances"][3]        # its subject is missing from a frame: evaluate_actions refuses the short trajectory
    (tmp_path / "anno").mkdir()
    (tmp_path / "anno" / "anno13.json").write_text(json.dumps(anno))
    E = _E()
    objects = [dict(o, score=1.0 / (k + 1)) for k, o in enumerate(E.object_instances(anno))]
    actions = [dict(a, score=1.0 / (k + 1)) for k, a in enumerate(E.action_instances(anno, cde.ACTION_PREDICATES))]
    for task, results, extra, lines in (("object", objects, [], ["ball", "dog", "person"]),
                                        ("action", actions, ["--action-predicates", str(tmp_path / "p.txt")], ["chase", "left"])):
        (tmp_path / "pred.json").write_text(json.dumps({"version": "VERSION 1.0", "results": {"anno13": results}}))
        monkeypatch.setattr(sys, "argv", ["evaluate_detection.py", "--task", task, "--prediction", str(tmp_path / "pred.json"),
                                          "--annotations", str(tmp_path / "anno")] + extra)
        tool.main()
        out = capsys.readouterr().out.splitlines()
        assert out[:2] == ["Number of videos in ground truth: 1", "Number of videos in prediction: 1"]
        assert [line.split()[1] for line in out[2:-1]] == lines and all(line.endswith("1.0000") for line in out[2:])
        assert out[-1].split() == ["mean", "AP", "1.0000"]


# ---------------------------------------------------------------------------------------------------- the entries
def test_entry_points_are_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    raw = ctypes.CDLL(abi.LIB_PATH)
    assert all(hasattr(raw, e) for e in ENTRIES) and abi.lib().tspn_version() == 7
    assert {"evalobj_tiou", "evalobj_claim"} <= set(tspn_mi355x.ops.__all__)
    assert {"evaluate_objects", "evaluate_actions", "object_instances", "action_instances"} <= set(tspn_mi355x.evaluation.__all__)
    assert tspn_mi355x.evaluate_objects is tspn_mi355x.evaluation_detection.evaluate_objects
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    for entry, n in (("tspn_evalobj_tiou_f64", 11), ("tspn_evalobj_claim", 10)):
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % entry, header, re.S).group(1)
        assert "workspace" not in params and len(params.split(",")) == len(abi.PROTOTYPES[entry][1]) == n
    assert "_workspace_bytes" not in "".join(e for e in abi.PROTOTYPES if "evalobj" in e)


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any launch: the pointers are made-up addresses."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    vp = ctypes.c_void_p
    ok, null = vp(0x10000), vp(0)
    names = ("boxes", "frames", "traj", "groups", "pred_group")
    outs = ("best", "best_index", "flags")

    def tiou(n_pred=3, tiou=ok, **ptr):
        rc = lib.tspn_evalobj_tiou_f64(*[ptr.get(n, ok) for n in names], n_pred, tiou, *[ptr.get(n, ok) for n in outs], null)
        return rc, lib.tspn_last_error().decode()
    w = "tspn_evalobj_tiou_f64: "
    assert tiou(n_pred=-1) == (A_.TSPN_EINVAL, w + "bad sizes n_pred=-1")
    for n in names + outs:
        assert tiou(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert tiou(boxes=vp(0x10010)) == (A_.TSPN_EINVAL, w + "boxes must be 32-byte aligned")
    assert tiou(boxes=vp(0x10008))[0] == A_.TSPN_EINVAL
    assert tiou(n_pred=2 ** 33) == (A_.TSPN_EUNSUPPORTED, w + "too many predictions")
    assert "bad sizes" in tiou(n_pred=-1, boxes=null)[1] and "null pointer" in tiou(boxes=vp(0x10010), flags=null)[1]
    nothing = {n: null for n in names + outs}
    assert tiou(n_pred=0, tiou=null, **nothing)[0] == A_.TSPN_OK         # no predictions: no launch, no pointer needed

    ins = ("best", "best_index", "groups", "pred_group")

    def claim(n_pred=3, n_gt=2, thr=0.5, claim=ok, hit=ok, **ptr):
        rc = lib.tspn_evalobj_claim(*[ptr.get(n, ok) for n in ins], n_pred, n_gt, thr, claim, hit, null)
        return rc, lib.tspn_last_error().decode()
    w = "tspn_evalobj_claim: "
    assert claim(n_pred=-1) == (A_.TSPN_EINVAL, w + "bad sizes n_pred=-1 n_gt=2")
    assert claim(n_gt=-5) == (A_.TSPN_EINVAL, w + "bad sizes n_pred=3 n_gt=-5")
    for n in ins:
        assert claim(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert claim(claim=null) == claim(hit=null) == (A_.TSPN_EINVAL, w + "null pointer")
    assert claim(thr=float("nan")) == (A_.TSPN_EINVAL, w + "thresh_t is NaN")
    assert claim(n_gt=2 ** 40) == (A_.TSPN_EUNSUPPORTED, w + "too many trajectories")
    assert "null pointer" in claim(hit=null, thr=float("nan"))[1] and "NaN" in claim(thr=float("nan"), n_pred=2 ** 40)[1]
    assert claim(n_pred=0, n_gt=0, claim=null, hit=null, **{n: null for n in ins})[0] == A_.TSPN_OK
    # what has no element may be null: claim without ground truths, the rest without predictions
    assert "null pointer" not in claim(n_gt=0, claim=null, thr=float("nan"))[1]
    assert "null pointer" not in claim(n_pred=0, hit=null, thr=float("nan"), **{n: null for n in ins})[1]


# ---------------------------------------------------------------------------------------------------- csrc/evalobj/
def test_evalobj_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_EO, "*.hip"))))
    assert in_source == {r["kernel"] for r in evalobj_kernel_variants.VARIANTS} and len(in_source) == 4
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in evalobj_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] in ENTRIES and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_EO]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "evalobj_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    # csrc/eval/ keeps its three kernels: the action evaluator adds none
    assert len(global_kernels(sorted(glob.glob(os.path.join(PKG, "csrc", "eval", "*.hip"))))) == 3


def test_evalobj_sources_are_built_and_keep_the_discipline():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert [os.path.basename(f) for f in hips] == ["tspn_eval_objects.hip"] and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "getenv" not in text, f"{f} reads the environment"
        assert "hipMemset" not in text and "hipMalloc" not in text and "Synchronize" not in text, f"{f}: launch contract"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert not re.search(r"\basm\b|__asm", code), f"{f}: plain C++ only"
        assert "workspace" not in code and '#include "tspn_common.h"' in text
        assert not re.search(r"define\s+TSPN_REQUIRE|int\s+check_launch|ceil_div\s*\(int64_t\s+\w+,\s*int64_t", code), \
            f"{f} copies a shared helper"
        atomics = re.findall(r"\batomic\w+", code)
        assert atomics and set(atomics) == {"atomicMin"}, atomics          # integer atomicMin only: deterministic
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_evalobj_sources_pass_the_store_lint():
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available: nothing to compile to ISA")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] +
                         [f for f in NEW_SOURCES if f.endswith(".hip")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert "tspn_eval_objects.hip" in res.stdout


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in evalobj_kernel_variants.VARIANTS}
    found = {n.split("::")[-1].split("(")[0]: r for n, r in res.items() if any(k + "(" in n for k in names)}
    assert set(found) == names
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
        assert r.get("lds_bytes", 0) == 0, (n, r)
