"""Relation detection evaluation on the GPU (tspn_mi355x.evaluation, csrc/eval/tspn_eval.hip) against the reference's
own numbers (golden g12) and against a Python-float restatement of its vIoU and greedy match kept in this file."""
import copy

import numpy as np
import pytest
import torch

import cases
import cases_eval

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- restatement
def viou_py(t1, d1, t2, d2):
    """The reference's vIoU (lib/evaluation/common.py:65-106) in Python floats: half-open durations, the overlap
    summed in frame order over the common frames, each volume over its whole trajectory, unclamped."""
    if d1[0] >= d2[1] or d1[1] <= d2[0]:
        return 0.
    v_ov = 0
    for f in range(max(d1[0], d2[0]), min(d1[1], d2[1])):
        a, b = t1[f - d1[0]], t2[f - d2[0]]
        w = min(a[2], b[2]) - max(a[0], b[0]) + 1
        h = min(a[3], b[3]) - max(a[1], b[1]) + 1
        v_ov += max(0, w) * max(0, h)
    vols = []
    for t in (t1, t2):
        v = 0
        for b in t:
            v += (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
        vols.append(v)
    return float(v_ov) / (vols[0] + vols[1] - v_ov)


def greedy_py(gt, preds, thr=0.5):
    """Hit flags and matched ground-truth index of the predictions in stable descending score order."""
    order = sorted(range(len(preds)), key=lambda i: preds[i]["score"], reverse=True)
    detected = [False] * len(gt)
    hit, match = [], []
    for i in order:
        p = preds[i]
        best, k_best = -float("inf"), -1
        for k, g in enumerate(gt):
            if detected[k] or tuple(p["triplet"]) != tuple(g["triplet"]):
                continue
            ov = min(viou_py(p["sub_traj"], p["duration"], g["sub_traj"], g["duration"]),
                     viou_py(p["obj_traj"], p["duration"], g["obj_traj"], g["duration"]))
            if ov >= thr and ov > best:
                best, k_best = ov, k
        if k_best >= 0:
            detected[k_best] = True
        hit.append(k_best >= 0)
        match.append(k_best)
    return np.array(order), np.array(hit, dtype=bool), np.array(match, dtype=np.int64)


def check_details(info, gt, pred, thr=0.5):
    for vid, d in info.items():
        order, hit, match = greedy_py(gt[vid], pred[vid], thr)
        assert np.array_equal(d["order"], order), vid
        assert np.array_equal(d["hit"], hit), vid
        assert np.array_equal(d["match"], match), vid


def assert_same(got, want):
    """== with the numpy dtype (Python float and numpy scalars are told apart)."""
    assert type(got) is type(want) and got == want, (got, type(got), want, type(want))


def golden_aggregates(g, prefix):
    return (g[prefix + "mean_ap"][()],
            {k: g[f"{prefix}rec_at_{k}"][()] for k in (50, 100, 1000)},
            {k: g[f"{prefix}mprec_at_{k}"][()] for k in (1, 5, 10)})


def check_aggregates(got, want):
    assert_same(got[0], want[0])
    for a, b in ((got[1], want[1]), (got[2], want[2])):
        assert list(a) == list(b)
        for k in a:
            assert_same(a[k], b[k])


# ---------------------------------------------------------------------------------------------------- golden g12
@pytest.mark.parametrize("thr,prefix", [(0.5, ""), (0.7, "thr07/")])
def test_g12_aggregates_and_hits_equal_the_reference(tspn, device, thr, prefix):
    g = cases.load("g12_evaluation.npz")
    gt, pred, _ = cases_eval.g12_case()
    res = tspn.evaluation.evaluate(gt, pred, viou_threshold=thr, device=device, details=True)
    check_aggregates(res[:3], golden_aggregates(g, prefix))
    if prefix == "":
        assert list(res[3]) == list(g["vids"])
        for vid in g["vids"]:
            hs = g[f"{vid}/hit_scores"]
            assert np.array_equal(res[3][vid]["hit"], np.isfinite(hs)), vid
            assert_same(res[3][vid]["ap"], g[f"{vid}/ap"][()])
    check_details(res[3], gt, pred, thr)


@pytest.mark.parametrize("old", [False, True])
def test_g12_zeroshot_equals_the_reference(tspn, device, old):
    g = cases.load("g12_evaluation.npz")
    gt, pred, train = cases_eval.g12_case()
    got = tspn.evaluation.evaluate_zeroshot(gt, pred, train, old=old, device=device)
    check_aggregates(got, golden_aggregates(g, "zs_old/" if old else "zs_new/"))


# ---------------------------------------------------------------------------------------------------- vIoU kernel
def _random_traj(rs, n, ints, min_wh=-3):
    x = rs.randint(0, 60, size=2) if ints else rs.uniform(0, 60, size=2)
    wh = rs.randint(min_wh, 60, size=2) if ints else rs.uniform(min_wh, 60, size=2)
    steps = rs.randint(-3, 4, size=(n, 2)) if ints else rs.uniform(-3, 3, size=(n, 2))
    xy = x + np.cumsum(steps, axis=0)
    boxes = np.concatenate([xy, xy + wh], axis=1)
    return [tuple(int(c) for c in b) for b in boxes] if ints else [tuple(float(c) for c in b) for b in boxes]


@pytest.mark.parametrize("ints", [False, True])
def test_viou_bit_equal_to_the_python_restatement(tspn, device, ints):
    """One group of 7 predictions x 150 ground truths (three 64-lane chunks), random durations (disjoint, touching,
    nested, partial): every ov equals min(viou_py(subject), viou_py(object)) to the bit."""
    rs = np.random.RandomState(17 + ints)
    T = ("a", "b", "c")

    def rel(score=None):
        b = int(rs.randint(0, 60))
        e = b + int(rs.randint(1, 40))
        r = {"triplet": T, "duration": (b, e), "sub_traj": _random_traj(rs, e - b, ints),
             "obj_traj": _random_traj(rs, e - b, ints)}
        if score is not None:
            r["score"] = score
        return r
    gt = [rel() for _ in range(150)]
    gt[3]["duration"] = (gt[4]["duration"][1], gt[4]["duration"][1] + len(gt[3]["sub_traj"]))   # touching gt 4
    preds = [rel(float(s)) for s in rs.uniform(size=7)]
    k = next(k for k, g in enumerate(gt) if all(b[2] > b[0] and b[3] > b[1] for b in g["sub_traj"] + g["obj_traj"]))
    preds[0] = dict(preds[0], duration=gt[k]["duration"], sub_traj=gt[k]["sub_traj"], obj_traj=gt[k]["obj_traj"])
    E = tspn.evaluation
    videos = E._prepare({"v": gt}, {"v": preds})
    pk = E._pack(videos)
    assert pk["candidates"] == 7 * 150 and pk["groups"].shape == (1, 5)
    t = {k: torch.from_numpy(pk[k]).to(device) for k in ("boxes", "traj", "groups", "pred_group")}
    vol = tspn.ops.eval_traj_volume(t["boxes"], t["traj"])
    ov, zden = tspn.ops.eval_viou(t["boxes"], t["traj"], vol, t["groups"], t["pred_group"], pk["candidates"])
    ov = ov.cpu().numpy().reshape(7, 150)
    assert not zden.cpu().numpy().any()
    order = videos[0]["order"]
    want = np.array([[min(viou_py(preds[i]["sub_traj"], preds[i]["duration"], g["sub_traj"], g["duration"]),
                          viou_py(preds[i]["obj_traj"], preds[i]["duration"], g["obj_traj"], g["duration"]))
                      for g in gt] for i in order])
    assert np.array_equal(ov.view(np.int64), want.view(np.int64))   # to the bit, the sign of a zero included
    assert (want == 0).any() and (want > 0.5).any()


def test_zero_denominator_raises(tspn, device):
    a = [(0, 0, 1, 1)] * 2                # 4 pixels a frame
    b = [(0, 0, -1, 1)] * 2               # width 0: volume 0, so v1 + v2 - v_ov == 0
    gt = {"v": [{"triplet": (1, 2, 3), "duration": (0, 2), "sub_traj": b, "obj_traj": a}]}
    pred = {"v": [{"triplet": (1, 2, 3), "duration": (0, 2), "sub_traj": b, "obj_traj": a, "score": 1.0}]}
    with pytest.raises(ZeroDivisionError):   # subject: v_ov 0, v1 + v2 = 0
        viou_py(b, (0, 2), b, (0, 2))
    with pytest.raises(ZeroDivisionError, match="video 'v', prediction 0"):
        tspn.evaluation.evaluate(gt, pred, device=device)


# ---------------------------------------------------------------------------------------------------- greedy match
def _copy_rel(r, **kw):
    out = dict(r)
    out.update(kw)
    return out


@pytest.mark.parametrize("n_gt", [70, 130, 4200])
def test_greedy_ties_and_large_groups(tspn, device, n_gt):
    """Many identical ground truths (every ov ties: the lowest undetected index wins, in every 64-lane chunk and past
    4096 ground truths, where the detected flags leave the register), equal scores (input order), and a second
    triplet interleaved."""
    rs = np.random.RandomState(n_gt)
    base = _random_traj(rs, 6, True, min_wh=1)
    other = _random_traj(rs, 6, True, min_wh=1)
    T, U = ("p", "q", "r"), ("p", "q", "s")
    gt = [{"triplet": U if k % 61 == 60 else T, "duration": (2, 8), "sub_traj": base, "obj_traj": base if k % 5 else other}
          for k in range(n_gt)]
    n_pred = min(n_gt + 10, 80)
    preds = [{"triplet": T if i % 4 else U, "duration": (2, 8), "sub_traj": base, "obj_traj": base,
              "score": float(rs.randint(0, 3))} for i in range(n_pred)]
    gts, ps = {"v": gt}, {"v": preds}
    res = tspn.evaluation.evaluate(gts, ps, device=device, details=True)
    check_details(res[3], gts, ps)
    assert res[3]["v"]["hit"].sum() > 0


def test_max_candidates_chunks_give_the_same_result(tspn, device):
    gt, pred, train = cases_eval.g12_case()
    E = tspn.evaluation
    one = E.evaluate(gt, pred, device=device, details=True)
    stats = {}
    many = E.evaluate(gt, pred, device=device, details=True, max_candidates=50, stats=stats)
    assert stats["chunks"] >= 4
    check_aggregates(many[:3], one[:3])
    for vid in one[3]:
        assert np.array_equal(one[3][vid]["hit"], many[3][vid]["hit"])
        assert np.array_equal(one[3][vid]["match"], many[3][vid]["match"])


def _synthetic_video(rs, n_pred, n_gt, n_trip=6, frames=60):
    def traj(n):
        return _random_traj(rs, n, False, min_wh=1)
    gt = []
    for _ in range(n_gt):
        b = int(rs.randint(0, frames - 5))
        e = b + int(rs.randint(1, 25))
        gt.append({"triplet": [int(rs.randint(n_trip)), 0, 1], "duration": [b, e], "sub_traj": [
            tuple(int(c) for c in bb) for bb in traj(e - b)], "obj_traj": [tuple(int(c) for c in bb) for bb in traj(e - b)]})
    preds = []
    for i in range(n_pred):
        if i % 2 and gt:
            g = gt[rs.randint(len(gt))]
            j = rs.randint(-2, 3, size=(len(g["sub_traj"]), 4))
            preds.append({"triplet": list(g["triplet"]), "duration": list(g["duration"]),
                          "sub_traj": np.asarray(g["sub_traj"], dtype=np.float64) + j,
                          "obj_traj": [tuple(float(c) for c in bb) for bb in g["obj_traj"]],
                          "score": float(rs.randint(0, 50)) / 50})
        else:
            b = int(rs.randint(0, frames - 5))
            e = b + int(rs.randint(1, 25))
            preds.append({"triplet": [int(rs.randint(n_trip)), 0, 1], "duration": [b, e], "sub_traj": traj(e - b),
                          "obj_traj": traj(e - b), "score": float(rs.uniform())})
    return gt, preds


def test_four_videos_of_3000_predictions_against_the_restatement(tspn, device):
    rs = np.random.RandomState(3)
    gt, pred = {}, {}
    for k in range(4):
        gt[f"v{k}"], pred[f"v{k}"] = _synthetic_video(rs, 3000, 40)
    res = tspn.evaluation.evaluate(gt, pred, device=device, details=True)
    check_details(res[3], gt, pred)
    assert all(res[3][v]["hit"].sum() > 5 for v in gt)


def test_max_bytes_chunks_give_the_same_result(tspn, device):
    gt, pred, _ = cases_eval.g12_case()
    E = tspn.evaluation
    one = E.evaluate(gt, pred, device=device, details=True)
    stats = {}
    many = E.evaluate(gt, pred, device=device, details=True, max_bytes=1, stats=stats)
    assert stats["chunks"] == sum(1 for v in E._prepare(gt, pred) if v["groups"])
    check_aggregates(many[:3], one[:3])
    for vid in one[3]:
        assert np.array_equal(one[3][vid]["hit"], many[3][vid]["hit"])
        assert np.array_equal(one[3][vid]["match"], many[3][vid]["match"])


def test_chunk_of_empty_trajectories(tspn, device):
    """Every packed trajectory empty (begin == end): no box row at all, every vIoU 0 (such durations never overlap).
    With threshold 0 those zeros are hits, matched in ground-truth order like the reference's loop."""
    T = ("x", "y", "z")
    gt = {"v": [{"triplet": T, "duration": (b, b), "sub_traj": [], "obj_traj": []} for b in (3, 5, 5, 9)]}
    pred = {"v": [{"triplet": T, "duration": (b, b), "sub_traj": [], "obj_traj": [], "score": s}
                  for b, s in ((5, 0.5), (4, 0.5), (5, 0.75))]}
    assert tspn.evaluation._pack(tspn.evaluation._prepare(gt, pred))["rows"] == 0
    for thr in (0.5, 0.0):
        res = tspn.evaluation.evaluate(gt, pred, viou_threshold=thr, device=device, details=True)
        check_details(res[3], gt, pred, thr)
        assert res[3]["v"]["hit"].sum() == (3 if thr == 0.0 else 0)


def test_end_to_end_association_then_evaluation(tspn, device):
    """Synthetic short-term relations -> greedy_relational_association on the device -> evaluate: the associated
    relations, scored against ground truth made from a subset of them (exact hits) and shifted copies (misses and
    partial overlaps), give the restatement's hits."""
    rels, trajs = cases.g9_scenario(seed=23, n_seg=8, n_trk=12, n_pred=60)
    out = tspn.association.greedy_relational_association(None, copy.deepcopy(rels), trajectories=trajs, device=device)
    # the scenario exercises the reference's in-place trajectory aliasing, after which a merged relation's duration
    # (subject start, object end) need not match its trajectories: evaluate refuses those (documented addition)
    ok = [r for r in out if len(r["sub_traj"]) == len(r["obj_traj"]) == r["duration"][1] - r["duration"][0]]
    assert 10 < len(ok) < len(out)
    bad = next(r for r in out if r not in ok)
    with pytest.raises(ValueError, match="boxes for the duration"):
        tspn.evaluation.evaluate({"vid0": [bad]}, {"vid0": [bad]}, device=device)
    out = ok
    gt = []
    for i, r in enumerate(out):
        if i % 3 == 0:
            gt.append({k: r[k] for k in ("triplet", "duration", "sub_traj", "obj_traj")})
        elif i % 3 == 1:
            b, e = r["duration"]
            gt.append({"triplet": r["triplet"], "duration": [b + 2, e + 2], "sub_traj": r["sub_traj"],
                       "obj_traj": r["obj_traj"]})
    gts, preds = {"vid0": gt}, {"vid0": out}
    res = tspn.evaluation.evaluate(gts, preds, device=device, details=True)
    check_details(res[3], gts, preds)
    assert res[3]["vid0"]["hit"].sum() >= 10


def test_no_predictions_anywhere_raises_index_error(tspn, device):
    gt, _, _ = cases_eval.g12_case()
    with pytest.raises(IndexError):
        tspn.evaluation.evaluate(gt, {vid: [] for vid in gt}, device=device)
