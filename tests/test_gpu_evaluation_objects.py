"""Object detection evaluation on the GPU (tspn_mi355x.evaluation.evaluate_objects, csrc/evalobj/tspn_eval_objects.hip)
against the reference's own numbers (golden g13) and against the pure-Python restatement of
tests/detection_eval_reference.py, which tests/test_evaluation_detection_host.py holds equal to g13.  Every comparison
is `==` on float64 and on integers."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import cases_detection_eval as cde
import detection_eval_reference as R
import sentinel_buffers as sb

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
OBJECT_CONFIGS = [(True, 0.5, "07_0.5"), (True, 0.3, "07_0.3"), (False, 0.5, "voc_0.5"), (False, 0.3, "voc_0.3")]
_RESTATED = {}


def restated(name, gt, pred, m07=True, thr=0.5):
    """The restatement's answer for a named case, computed once and shared (never modified)."""
    key = (name, m07, thr)
    if key not in _RESTATED:
        _RESTATED[key] = R.evaluate_objects(gt, pred, m07, thr)
    return _RESTATED[key]


def assert_same(got, want):
    """== with the type (Python float and numpy scalars are told apart)."""
    assert type(got) is type(want) and got == want, (got, type(got), want, type(want))


def check_result(got, want, gt, pred):
    """(mean_ap, ap_class, details) of evaluate_objects against the restatement's (mean_ap, ap_class, per_pred)."""
    assert_same(got[0], want[0])
    assert [c for c, _ in got[1]] == [c for c, _ in want[1]]
    for (_, a), (_, b) in zip(got[1], want[1]):
        assert_same(a, b)
    seen = 0
    for vid, d in got[2].items():
        scores = [t["score"] for t in pred[vid]]
        assert d["order"].tolist() == sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)
        assert d["tiou"].dtype == np.float64 and d["hit"].dtype == bool and d["match"].dtype == np.int64
        for pos, i in enumerate(d["order"].tolist()):
            c = pred[vid][i]["category"]
            of_class = [k for k, g in enumerate(gt.get(vid, [])) if g["category"] == c]
            if (vid, i) in want[2] and of_class:
                mo, mi, tp = want[2][(vid, i)]
                assert (d["tiou"][pos], d["match"][pos], d["hit"][pos]) == (mo, of_class[mi], tp), (vid, i)
                seen += 1
            else:                      # a category without ground truth here: never packed, a false positive
                assert (d["tiou"][pos], d["match"][pos], d["hit"][pos]) == (0.0, -1, False), (vid, i)
    return seen


# ---------------------------------------------------------------------------------------------------- 1. golden g13
@pytest.mark.parametrize("m07,thr,name", OBJECT_CONFIGS)
def test_g13_objects_equal_the_reference(tspn, device, m07, thr, name):
    g = cases.load("g13_detection_eval.npz")
    gt, pred = cde.g13_object_case()
    got = tspn.evaluation.evaluate_objects(gt, pred, use_07_metric=m07, thresh_t=thr, device=device, details=True)
    assert isinstance(got[0], np.floating) == bool(g[f"obj/{name}/mean_ap_is_np"]) and got[0] == g[f"obj/{name}/mean_ap"][()]
    assert [c for c, _ in got[1]] == list(g[f"obj/{name}/categories"])
    assert [ap for _, ap in got[1]] == list(g[f"obj/{name}/ap"])
    assert [isinstance(ap, np.floating) for _, ap in got[1]] == list(g[f"obj/{name}/ap_is_np"])
    assert all(type(ap) in (float, np.float64) for _, ap in got[1]) and type(got[0]) in (float, np.float64)
    # per prediction of a ground-truth class, in `prediction` order: the reference's own (max_overlap, max_index)
    gt_classes = set(t["category"] for tracks in gt.values() for t in tracks)
    best, index = [], []
    for vid, tracks in pred.items():
        d = got[2][vid]
        back = np.argsort(d["order"], kind="stable")               # input index -> position in score order
        for i, t in enumerate(tracks):
            if t["category"] in gt_classes:
                of_class = [k for k, q in enumerate(gt[vid]) if q["category"] == t["category"]]
                best.append(d["tiou"][back[i]])
                index.append(of_class.index(d["match"][back[i]]) if of_class else 0)
    assert best == list(g["obj/max_overlap"]) and index == list(g["obj/max_index"])
    assert check_result(got, restated("g13", gt, pred, m07, thr), gt, pred) > 200


# ---------------------------------------------------------------------------------------------------- the kernels alone
def pack_groups(groups):
    """The ABI layout of a list of (predictions, ground truths) groups, each a list of {frame: box} dicts."""
    P = sum(len(p) for p, _ in groups)
    trajs = [t for p, _ in groups for t in p] + [t for _, g in groups for t in g]
    frames, boxes, traj = [], [], []
    for t in trajs:
        fs = sorted(t)
        traj.append((len(frames), len(fs)))
        frames += fs
        boxes += [t[f] for f in fs]
    table, p0, g0, off = [], 0, P, 0
    for p, g in groups:
        table.append((p0, len(p), g0, len(g), off))
        p0, g0, off = p0 + len(p), g0 + len(g), off + len(p) * len(g)
    return {"boxes": np.array(boxes, dtype=np.float64).reshape(-1, 4) if boxes else np.zeros((1, 4)),
            "frames": np.array(frames, dtype=np.int32) if frames else np.zeros(1, dtype=np.int32),
            "traj": np.array(traj, dtype=np.int64).reshape(-1, 2), "groups": np.array(table, dtype=np.int64).reshape(-1, 5),
            "pred_group": np.repeat(np.arange(len(groups)), [len(p) for p, _ in groups]).astype(np.int32),
            "n_pred": P, "n_gt": len(trajs) - P, "candidates": off}


def expected(groups, thr):
    """tiou, best, best_index, claim and hit of the packed groups from the restatement's statements."""
    tiou, best, index, hit, claim = [], [], [], [], []
    for p, g in groups:
        det = [False] * len(g)
        mine = [INT32_MAX] * len(g)
        for pos, pt in enumerate(p):
            tiou += [R.tiou(q, pt) for q in g]
            mo, mi = R.trajectory_overlap(g, pt)
            tp = bool(g) and mo >= thr and not det[mi]
            if tp:
                det[mi] = True
                mine[mi] = pos
            best.append(float(mo)), index.append(mi), hit.append(tp)
        claim += mine
    return (np.array(tiou, dtype=np.float64), np.array(best, dtype=np.float64), np.array(index, dtype=np.int32),
            np.array(claim, dtype=np.int32), np.array(hit, dtype=np.int8))


def run_kernels(tspn, device, pk, thr, with_tiou=True):
    t = {k: torch.from_numpy(pk[k]).to(device) for k in ("boxes", "frames", "traj", "groups", "pred_group")}
    tiou, best, index, flags = tspn.ops.evalobj_tiou(t["boxes"], t["frames"], t["traj"], t["groups"], t["pred_group"],
                                                     n_cand=pk["candidates"] if with_tiou else None)
    claim, hit = tspn.ops.evalobj_claim(best, index, t["groups"], t["pred_group"], pk["n_gt"], thr)
    return [None if x is None else x.cpu().numpy() for x in (tiou, best, index, claim, hit, flags)]


def check_kernels(tspn, device, groups, thr=0.5):
    pk = pack_groups(groups)
    got = run_kernels(tspn, device, pk, thr)
    for name, a, b in zip(("tiou", "best", "best_index", "claim", "hit"), got, expected(groups, thr)):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert not got[5].any() and got[5].dtype == np.int32
    return got


# ---------------------------------------------------------------------------------------------------- 2. tIoU
def _box(rs, ints):
    x, y = (rs.randint(0, 40, size=2) if ints else rs.uniform(0, 40, size=2)).tolist()
    w, h = (rs.randint(30, 80, size=2) if ints else rs.uniform(30, 80, size=2)).tolist()
    return (x, y, x + w, y + h)


def _near(rs, b, ints, spread):
    j = (rs.randint(-spread, spread + 1, size=4) if ints else rs.uniform(-spread, spread, size=4)).tolist()
    return tuple(c + d for c, d in zip(b, j))


@pytest.mark.parametrize("ints", [False, True])
def test_tiou_equals_the_restatement(tspn, device, ints):
    """Frame counts of 1, 63, 64, 65 and 129 on either side (the lanes' stride and its tail), and 0 on one side; frame
    sets that are identical, interleaved (even against odd: no common frame), disjoint before and after, and that share
    only the first or only the last frame; boxes near the ground truth's, so that sIoU falls on both sides of 0.5, 0.7
    and 0.9."""
    rs = np.random.RandomState(5 + ints)
    sizes = (1, 63, 64, 65, 129)
    box_of = {}

    def gbox(f):
        if f not in box_of:
            box_of[f] = _box(rs, ints)
        return box_of[f]
    gts = [{2 * i: gbox(2 * i) for i in range(n)} for n in sizes]
    preds = []
    for n in sizes:
        even = [2 * i for i in range(n)]
        odd = [2 * i + 1 for i in range(n)]
        for fs in (even, odd, [f - 1000 for f in even], [f + 1000 for f in even], [0] + odd[1:], odd[:-1] + [even[-1]],
                   sorted(set(even[::3] + odd[::2]))):
            preds.append({f: _near(rs, gbox(f) if f in box_of and f % 2 == 0 else _box(rs, ints), ints, 1 + len(preds) % 4)
                          for f in fs})
    groups = [(preds + [{}], gts), (preds[:9], gts[:2] + [{}] + gts[2:])]
    got = check_kernels(tspn, device, groups)
    tiou = got[0]
    assert (tiou == 0).any() and len(set(tiou.tolist())) > 30 and tiou.max() > 0.6


def test_exact_thresholds(tspn, device):
    """One common frame, 10 x 10 against 10 x 5 / 10 x 7 / 10 x 9: sIoU is exactly 0.5 / 0.7 (= 70 / 100) / 0.9 and counts
    for its threshold; one pixel shorter does not."""
    g = {0: (0, 0, 9, 9)}
    rows = [(4, 1), (3, 0), (6, 2), (5, 1), (8, 3), (7, 2), (9, 3)]
    for floats in (False, True):
        preds = [{0: (0.0, 0.0, 9.0, float(y2)) if floats else (0, 0, 9, y2)} for y2, _ in rows]
        got = check_kernels(tspn, device, [(preds, [g])], thr=1.0 / 3)
        assert got[0].tolist() == [n * 1.0 / 3 for _, n in rows]
        assert got[4].tolist() == [1, 0, 0, 0, 0, 0, 0] and got[3].tolist() == [0]


# ---------------------------------------------------------------------------------------------------- 3. rules
def _objects(trajs, category="c", scores=None):
    out = [{"category": category, "trajectory": {str(f): b for f, b in t.items()}} for t in trajs]
    if scores is not None:
        for o, s in zip(out, scores):
            o["score"] = s
    return out


def test_argmax_and_match_rules(tspn, device):
    box, far = (0, 0, 9, 9), (100, 100, 109, 109)
    A = {f: box for f in range(4)}
    B = {f: box for f in range(6)}                     # against a copy of A: 4 common of 6 frames, tIoU 12 / 18
    # a tie between two ground truths keeps the lower index; the second identical prediction finds it taken
    got = check_kernels(tspn, device, [([A, A], [A, dict(A)])])
    assert got[2].tolist() == [0, 0] and got[4].tolist() == [1, 0] and got[3].tolist() == [0, INT32_MAX]
    # an all-zero row gives (0.0, 0) and a false positive, with and without ground truths
    got = check_kernels(tspn, device, [([{0: far}], [A, B]), ([A], [])])
    assert got[1].tolist() == [0.0, 0.0] and got[2].tolist() == [0, 0] and not got[4].any()
    # best == thresh_t exactly: two common frames, one at sIoU 1 and one below 0.5: 3 / 6
    half = {0: box, 1: (0, 0, 9, 3)}
    got = check_kernels(tspn, device, [([half], [{0: box, 1: box}])], thr=0.5)
    assert got[1].tolist() == [0.5] and got[4].tolist() == [1]
    assert check_kernels(tspn, device, [([half], [{0: box, 1: box}])], thr=0.5000000000000001)[4].tolist() == [0]
    # both predictions name A; the second also clears the threshold on B and is a false positive all the same
    got = check_kernels(tspn, device, [([A, dict(A)], [A, B])])
    assert got[0].tolist() == [1.0, 12 / 18, 1.0, 12 / 18] and got[4].tolist() == [1, 0]
    assert got[3].tolist() == [0, INT32_MAX]
    # a higher-scored prediction below the threshold on its best ground truth does not claim it
    weak = {0: box, 1: far, 2: far}                    # 3 / 9
    got = check_kernels(tspn, device, [([weak, {0: box}], [{0: box}])])
    assert got[1].tolist() == [1 / 3, 1.0] and got[4].tolist() == [0, 1] and got[3].tolist() == [1]
    # the same through evaluate_objects, in one video with two categories
    gt = {"v": _objects([A, B], "x") + _objects([{0: box}], "y")}
    pred = {"v": _objects([A, dict(A)], "x", [0.9, 0.8]) + _objects([weak, {0: box}], "y", [0.7, 0.6])}
    res = tspn.evaluation.evaluate_objects(gt, pred, device=device, details=True)
    assert check_result(res, R.evaluate_objects(gt, pred), gt, pred) == 4
    assert res[2]["v"]["hit"].tolist() == [True, False, False, True] and res[2]["v"]["match"].tolist() == [0, 0, 2, 2]


# ---------------------------------------------------------------------------------------------------- 4. sizes
def _small_traj(rs, n=3):
    f0 = int(rs.randint(0, 4))
    return {f0 + i: _box(rs, True) for i in range(n)}


def _copy_of(rs, t):
    return {f: _near(rs, b, True, 2) for f, b in t.items() if rs.randint(0, 6)}


@pytest.mark.parametrize("n_pred", [1, 5])
def test_kernel_edge_sizes_few_predictions(tspn, device, n_pred):
    """1 and 5 predictions: the tIoU kernel's last workgroup of four waves is partial."""
    rs = np.random.RandomState(n_pred)
    gts = [_small_traj(rs) for _ in range(3)]
    check_kernels(tspn, device, [([_copy_of(rs, gts[i % 3]) for i in range(n_pred)], gts)])


def test_kernel_edge_sizes(tspn, device):
    """Groups of 0, 1, 3 and 70 ground truths next to each other, and 64, 65 and 200 predictions that claim inside one
    group of 70 (most ground truths are named several times: the smallest position wins)."""
    rs = np.random.RandomState(11)
    groups = []
    for n_gt, n_pred in ((0, 3), (1, 2), (3, 7), (70, 64), (70, 65), (70, 200), (0, 1), (1, 1)):
        gts = [_small_traj(rs) for _ in range(n_gt)]
        preds = [_copy_of(rs, gts[rs.randint(0, n_gt)]) if n_gt and i % 7 else _small_traj(rs) for i in range(n_pred)]
        groups.append((preds, gts))
    got = check_kernels(tspn, device, groups, thr=0.3)
    claim, hit = got[3], got[4]
    assert hit.sum() == (claim != INT32_MAX).sum() > 100 and (claim == INT32_MAX).any()
    pk = pack_groups(groups)
    named = np.bincount((pk["groups"][pk["pred_group"], 2] - pk["n_pred"] + got[2])[got[1] >= 0.3], minlength=pk["n_gt"])
    assert named.max() >= 3                                        # duplicate claims did happen


def test_several_groups_per_video_and_videos_per_chunk(tspn, device):
    rs = np.random.RandomState(13)
    gt, pred = _synthetic(rs, videos=3, n_pred=40, n_gt=9, classes=4, frames=12)
    stats = {}
    res = tspn.evaluation.evaluate_objects(gt, pred, device=device, details=True, stats=stats)
    assert stats["chunks"] == 1 and stats["candidates"] > 100
    E = tspn.evaluation_detection
    videos = E._prepare("t", gt, pred, *E._gt_classes(gt), True, E._object_rows, E._object_chunk_bytes)
    assert all(len(v["groups"]) >= 2 for v in videos)
    assert check_result(res, R.evaluate_objects(gt, pred), gt, pred) > 60


# ---------------------------------------------------------------------------------------------------- 5. chunking
def test_chunking_gives_the_same_result(tspn, device):
    gt, pred = cde.g13_object_case()
    E = tspn.evaluation
    one = E.evaluate_objects(gt, pred, device=device, details=True)
    for kw, least in (({"max_candidates": 20}, 4), ({"max_bytes": 1}, 4)):
        stats = {}
        many = E.evaluate_objects(gt, pred, device=device, details=True, stats=stats, **kw)
        assert stats["chunks"] >= least
        assert_same(many[0], one[0])
        assert many[1] == one[1] and list(many[2]) == list(one[2])
        for vid in one[2]:
            for k in ("hit", "match", "tiou", "order"):
                assert np.array_equal(one[2][vid][k], many[2][vid][k]), (vid, k)


# ---------------------------------------------------------------------------------------------------- 6. flags
def test_flags_raise_zero_division(tspn, device):
    flat = (5, 5, 4, 4)                                 # width and height 0: two of them share no area and have none
    gt = {"v": _objects([{0: (0, 0, 9, 9)}, {3: flat}])}
    pred = {"v": _objects([{0: (0, 0, 9, 9)}, {3: flat, 4: (0, 0, 1, 1)}], scores=[0.9, 0.8])}
    with pytest.raises(ZeroDivisionError):
        R.evaluate_objects(gt, pred)
    with pytest.raises(ZeroDivisionError, match="video 'v', prediction 1: zero sIoU denominator"):
        tspn.evaluation.evaluate_objects(gt, pred, device=device)
    gt = {"v": _objects([{0: (0, 0, 9, 9)}, {}])}
    pred = {"v": _objects([{0: (0, 0, 9, 9)}, {1: (0, 0, 9, 9)}, {}], scores=[0.9, 0.8, 0.7])}
    with pytest.raises(ZeroDivisionError):
        R.evaluate_objects(gt, pred)
    with pytest.raises(ZeroDivisionError, match="video 'v', prediction 2: no frame in it nor in"):
        tspn.evaluation.evaluate_objects(gt, pred, device=device)
    # the flags themselves: bit 0 and bit 1, on the predictions that have them and on no other
    pk = pack_groups([([{0: (0, 0, 9, 9)}, {3: flat}, {}], [{3: flat}, {}])])
    assert run_kernels(tspn, device, pk, 0.5)[5].tolist() == [0, 1, 2]


# ---------------------------------------------------------------------------------------------------- 7. sentinels
I_SENTINEL = -77                # no index, flag, claim or hit is ever this value (tests/sentinel_buffers.py's is a float)


def held_int(n, dtype, device):
    buf = torch.full((n + 2 * sb.GUARD,), I_SENTINEL, dtype=dtype, device=device)
    return buf, buf[sb.GUARD:sb.GUARD + n]


def assert_int_written_inside_only(buf, n, what):
    b = buf.cpu()
    assert bool((b[:sb.GUARD] == I_SENTINEL).all()) and bool((b[sb.GUARD + n:] == I_SENTINEL).all()), f"{what}: wrote outside"
    assert not bool((b[sb.GUARD:sb.GUARD + n] == I_SENTINEL).any()), f"{what}: an element never written"


def test_sentinels_and_null_tiou(tspn, device):
    """Through the C entries with caller-held outputs: guard bands intact, every element of tiou, best, best_index,
    flags, claim and hit written; tiou = NULL is accepted and changes nothing else."""
    rs = np.random.RandomState(3)
    groups = []
    for n_gt, n_pred in ((0, 2), (3, 5), (70, 9), (1, 1)):
        gts = [_small_traj(rs) for _ in range(n_gt)]
        groups.append(([_copy_of(rs, gts[i % n_gt]) if n_gt else _small_traj(rs) for i in range(n_pred)], gts))
    pk = pack_groups(groups)
    want = expected(groups, 0.4)
    t = {k: torch.from_numpy(pk[k]).to(device) for k in ("boxes", "frames", "traj", "groups", "pred_group")}
    lib = tspn._abi.lib()
    P, C, NG = pk["n_pred"], pk["candidates"], pk["n_gt"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_tiou in (True, False):
        tbuf, tiou = sb.held((C,), device, dtype=torch.float64)
        bbuf, best = sb.held((P,), device, dtype=torch.float64)
        ibuf, index = held_int(P, torch.int32, device)
        fbuf, flags = held_int(P, torch.int32, device)
        cbuf, claim = held_int(NG, torch.int32, device)
        hbuf, hit = held_int(P, torch.int8, device)
        rc = lib.tspn_evalobj_tiou_f64(sb.p(t["boxes"]), sb.p(t["frames"]), sb.p(t["traj"]), sb.p(t["groups"]),
                                       sb.p(t["pred_group"]), P, sb.p(tiou if with_tiou else None), sb.p(best),
                                       sb.p(index), sb.p(flags), stream)
        assert rc == 0, lib.tspn_last_error()
        rc = lib.tspn_evalobj_claim(sb.p(best), sb.p(index), sb.p(t["groups"]), sb.p(t["pred_group"]), P, NG, 0.4,
                                    sb.p(claim), sb.p(hit), stream)
        assert rc == 0, lib.tspn_last_error()
        torch.cuda.synchronize(device)
        if with_tiou:
            sb.assert_written_inside_only(tbuf, tiou, "tiou")
            assert np.array_equal(tiou.cpu().numpy(), want[0])
        else:
            sb.assert_untouched(tbuf, "tiou (NULL was passed)")
        sb.assert_written_inside_only(bbuf, best, "best")
        for buf, n, what in ((ibuf, P, "best_index"), (fbuf, P, "flags"), (cbuf, NG, "claim"), (hbuf, P, "hit")):
            assert_int_written_inside_only(buf, n, what)
        for name, a, b in zip(("best", "best_index", "claim", "hit"), (best, index, claim, hit), want[1:]):
            assert np.array_equal(a.cpu().numpy(), b), name
        assert not flags.cpu().numpy().any()
    # no predictions: claim is still written in full
    cbuf, claim = held_int(7, torch.int32, device)
    rc = lib.tspn_evalobj_claim(sb.p(None), sb.p(None), sb.p(None), sb.p(None), 0, 7, 0.5, sb.p(claim), sb.p(None), stream)
    assert rc == 0, lib.tspn_last_error()
    assert claim.cpu().tolist() == [INT32_MAX] * 7
    assert_int_written_inside_only(cbuf, 7, "claim without predictions")


# ---------------------------------------------------------------------------------------------------- 8. a middle size
def _synthetic(rs, videos=4, n_pred=300, n_gt=20, classes=8, frames=120):
    """Videos of ground truths with gapped frame sets and predictions that mostly copy one (jittered boxes, some frames
    dropped, a few added), as (frames, boxes) array pairs for the predictions; scores distinct over the whole set."""
    gt, pred = {}, {}
    scores = (rs.permutation(videos * n_pred) + 1) / float(videos * n_pred)
    for v in range(videos):
        gts = []
        for _ in range(n_gt):
            lo = int(rs.randint(0, frames // 2))
            fs = [f for f in range(lo, int(rs.randint(lo + 2, frames + 1))) if rs.randint(0, 8)] or [lo]
            b = np.array(_box(rs, True))
            gts.append({"category": int(rs.randint(0, classes)),
                        "trajectory": {str(f): tuple(int(c) for c in b + rs.randint(-1, 2, size=4) * (k % 3))
                                       for k, f in enumerate(fs)}})
        preds = []
        for i in range(n_pred):
            g = gts[rs.randint(0, n_gt)]
            if i % 5:
                fs = [int(f) for f in g["trajectory"] if rs.randint(0, 10)] or [0]
                fs = sorted(set(fs + [int(f) for f in rs.randint(0, frames, size=rs.randint(0, 3))]))
                bx = np.array([np.array(g["trajectory"].get(str(f), (0, 0, 5, 5)), dtype=np.float64)
                               + rs.randint(-8, 9, size=4) / 4.0 * (1 + i % 4) for f in fs])
                cat = g["category"] if i % 11 else int(rs.randint(0, classes + 2))
            else:
                fs = sorted(set(rs.randint(0, frames, size=rs.randint(1, 30)).tolist()))
                bx = np.array([_box(rs, False) for _ in fs])
                cat = int(rs.randint(0, classes + 2))
            preds.append({"category": cat, "score": float(scores[v * n_pred + i]),
                          "trajectory": (np.array(fs, dtype=np.int64), bx.reshape(-1, 4))})
        gt[f"v{v}"], pred[f"v{v}"] = gts, preds
    return gt, pred


def test_middle_size_against_the_restatement(tspn, device):
    """4 videos x 300 predictions x 20 ground truths in 8 classes, at most 120 frames, predictions as array pairs."""
    rs = np.random.RandomState(29)
    gt, pred = _synthetic(rs)
    want = R.evaluate_objects(gt, pred)
    for m07 in (True, False):
        res = tspn.evaluation.evaluate_objects(gt, pred, use_07_metric=m07, device=device, details=True)
        seen = check_result(res, want if m07 else R.evaluate_objects(gt, pred, False), gt, pred)
    hits = sum(int(d["hit"].sum()) for d in res[2].values())
    qualifying = sum(int((d["tiou"] >= 0.5).sum()) for d in res[2].values())
    assert seen > 800 and 20 < hits < qualifying
