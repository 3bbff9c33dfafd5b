"""Action detection evaluation on the GPU (tspn_mi355x.evaluation.evaluate_actions: the relation evaluator's kernels of
csrc/eval/tspn_eval.hip on instances packed as relations whose two trajectories are the same rows) against the reference's
own numbers (golden g13), the pure-Python restatement of tests/detection_eval_reference.py and the relation evaluator."""
import numpy as np
import pytest

import cases
import cases_detection_eval as cde
import detection_eval_reference as R

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    assert type(got) is type(want) and got == want, (got, type(got), want, type(want))


def check_against_restatement(got, want):
    """(mean_ap, ap_class, details) of evaluate_actions against the restatement's (mean_ap, ap_class, curves).  The mean
    is taken over the same set's iteration order in both (one process)."""
    assert_same(got[0], want[0])
    assert list(got[1]) == list(want[1])
    for c in want[1]:
        assert_same(got[1][c], want[1][c])
    assert sorted(got[2]["classes"]) == sorted(want[2])
    for c, curves in want[2].items():
        for a, b in zip(got[2]["classes"][c], curves):
            assert a.dtype == b.dtype and np.array_equal(a, b), c


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_g13_actions_equal_the_reference(tspn, device, thr):
    g = cases.load("g13_detection_eval.npz")
    gt, pred = cde.g13_action_case()
    got = tspn.evaluation.evaluate_actions(gt, pred, viou_threshold=thr, device=device, details=True)
    assert type(got[0]) is np.float64 and got[0] == g[f"act/{thr}/mean_ap"][()]
    cats = list(g[f"act/{thr}/categories"])
    assert sorted(got[1]) == cats and [got[1][c] for c in cats] == list(g[f"act/{thr}/ap"])
    assert [isinstance(got[1][c], np.floating) for c in cats] == list(g[f"act/{thr}/ap_is_np"])
    assert all(type(ap) in (float, np.float64) for ap in got[1].values())
    for c, (prec, rec, hit_scores) in got[2]["classes"].items():
        for a, name in ((prec, "prec"), (rec, "rec"), (hit_scores, "hit_scores")):
            want = g[f"act/{thr}/{c}/{name}"]
            assert a.dtype == want.dtype and np.array_equal(a, want), (c, name)
    assert sorted(got[2]["classes"]) == [c for c in cats if f"act/{thr}/{c}/prec" in g]
    check_against_restatement(got, R.evaluate_actions(gt, pred, thr))
    # the two hand-made predictions of a_1: vIoU exactly 0.5 hits at 0.5 only, its duplicate finds the ground truth taken
    d = got[2]["videos"]["a_1"]
    back = np.argsort(d["order"], kind="stable")
    n = len(pred["a_1"])
    assert d["hit"][back[n - 2:]].tolist() == [thr == 0.5, False]
    assert d["match"][back[n - 2:]].tolist() == [len(gt["a_1"]) - 1 if thr == 0.5 else -1, -1]


def test_absent_video_and_missing_class(tspn, device):
    """A prediction in a video that the ground truth lacks is a false positive (no KeyError), a ground-truth class
    without predictions scores 0., a predicted class outside the ground truth is ignored."""
    traj = [(0, 0, 9, 9)] * 4
    gt = {"v": [{"category": "run", "duration": (0, 4), "trajectory": traj},
                {"category": "swim", "duration": (0, 4), "trajectory": traj}]}
    pred = {"w": [{"category": "run", "duration": (0, 4), "trajectory": traj, "score": 0.9}],
            "v": [{"category": "run", "duration": (0, 4), "trajectory": traj, "score": 0.8},
                  {"category": "fly", "duration": (0, 4), "trajectory": traj, "score": 0.7}]}
    got = tspn.evaluation.evaluate_actions(gt, pred, device=device, details=True)
    check_against_restatement(got, R.evaluate_actions(gt, pred))
    assert got[1]["swim"] == 0. and type(got[1]["swim"]) is float and got[1]["run"] == 0.5 and got[0] == 0.25
    assert got[2]["classes"]["run"][2].tolist() == [-np.inf, 0.8]
    assert got[2]["videos"]["w"]["hit"].tolist() == [False] and got[2]["videos"]["v"]["hit"].tolist() == [True, False]


def test_equals_the_relation_evaluator(tspn, device):
    """Per (video, category) the match is the relation evaluator's on the same instances rewritten as relations with a
    constant predicate and obj_traj = sub_traj: the same hits, matches and order in every video that both know."""
    gt, pred = cde.g13_action_case()
    E = tspn.evaluation
    got = E.evaluate_actions(gt, pred, device=device, details=True)
    rel_gt = {vid: R.relations_of(a) for vid, a in gt.items()}
    rel_pred = {vid: R.relations_of(pred.get(vid, [])) for vid in gt}
    rel = E.evaluate(rel_gt, rel_pred, device=device, details=True)[3]
    assert set(rel) == set(gt)
    for vid in gt:
        if vid in pred:
            d = got[2]["videos"][vid]
            for k in ("hit", "match", "order"):
                assert np.array_equal(d[k], rel[vid][k]), (vid, k)
    assert sum(int(rel[vid]["hit"].sum()) for vid in rel) > 10
    # chunking by whole videos changes nothing
    stats = {}
    many = E.evaluate_actions(gt, pred, device=device, details=True, max_candidates=10, stats=stats)
    assert stats["chunks"] >= 3 and many[0] == got[0] and many[1] == got[1]
    for vid in got[2]["videos"]:
        assert np.array_equal(many[2]["videos"][vid]["hit"], got[2]["videos"][vid]["hit"])
