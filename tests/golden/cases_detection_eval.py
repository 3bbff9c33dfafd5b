"""Inputs of the detection evaluation golden (g13) and tests, regenerated bit for bit from the build-owned hash RNG.

`g13_object_case()` is a ground truth / prediction set for the trajectory mAP of the reference's
lib/evaluation/video_object_detection.py: sparse frame sets with gaps under str(frame) keys, integer ground-truth boxes
and float predictions, several predictions that name the same ground truth (duplicate claims), duplicated ground truths
(tIoU ties), a ground-truth class that nobody predicts, a predicted class that the ground truth lacks, (video, class)
groups with predictions and no ground truth, and scores that are distinct inside every class (the reference's sort is
unspecified on ties).
`g13_action_case()` is one for the per-predicate mAP of lib/evaluation/action_detection.py: durations that overlap,
touch and miss, equal scores, a class without predictions and predictions in a video that the ground truth lacks.
`g13_annotation()` is a small annotation dict for the two annotation readers; ACTION_PREDICATES their predicate list."""
import numpy as np

from cases_eval import Draw, int_traj, jitter

OBJECT_CLASSES = ("bicycle", "car", "dog", "person")
ACTION_CLASSES = ("jump", "lift", "run", "wave")
ACTION_PREDICATES = ("chase", "left")


def _frame_set(d, lo, hi, keep_of_8):
    """Ascending frames of [lo, hi) with gaps: each kept with probability keep_of_8 / 8."""
    if hi <= lo:
        return []
    keep = d.ints(hi - lo, 0, 8) < keep_of_8
    return [lo + i for i in range(hi - lo) if keep[i]]


def _object_video(seed, tag, n_gt, n_pred, classes, frames=48):
    d = Draw(seed, tag)
    gt = []
    for k in range(n_gt):
        if k % 5 == 4:                                   # a duplicate of the previous ground truth: every tIoU ties
            gt.append({"category": gt[-1]["category"], "trajectory": dict(gt[-1]["trajectory"])})
            continue
        lo = d.int(0, frames - 12)
        fs = _frame_set(d, lo, d.int(lo + 6, frames + 1), 6) or [lo]
        boxes = int_traj(d, len(fs))
        gt.append({"category": classes[d.int(0, len(classes))], "trajectory": {str(f): b for f, b in zip(fs, boxes)}})
    preds = []
    for _ in range(n_pred):
        kind = d.int(0, 8)
        if kind < 6:                                     # a copy of a ground truth: jittered boxes, a sub / superset of frames
            g = gt[d.int(0, n_gt)]
            fs = sorted(int(f) for f in g["trajectory"])
            boxes = jitter(d, [g["trajectory"][str(f)] for f in fs], scale=1 + kind // 2)
            keep = d.ints(len(fs), 0, 8) < 7
            traj = {str(f): b for f, b, k in zip(fs, boxes, keep) if k}
            for f in _frame_set(d, max(0, fs[0] - 3), fs[0], 4):   # frames in front of the ground truth's first
                traj[str(f)] = boxes[0]
            cat = g["category"] if kind < 5 else classes[d.int(0, len(classes))]
        else:
            lo = d.int(0, frames - 12)
            fs = _frame_set(d, lo, d.int(lo + 6, frames + 1), 5) or [lo]
            traj = {str(f): b for f, b in zip(fs, jitter(d, int_traj(d, len(fs))))}
            cat = (classes + ("ufo",))[d.int(0, len(classes) + 1)]
        preds.append({"category": cat, "trajectory": traj})
    return gt, preds


def g13_object_case():
    """(groundtruth, prediction): the object set of g13."""
    gt, pred = {}, {}
    gt["v_a"], pred["v_a"] = _object_video(31, "obj_a", 9, 60, OBJECT_CLASSES)
    gt["v_b"], pred["v_b"] = _object_video(32, "obj_b", 10, 60, OBJECT_CLASSES[:3])
    gt["v_c"], pred["v_c"] = _object_video(33, "obj_c", 5, 60, OBJECT_CLASSES[1:])
    gt["v_d"], pred["v_d"] = _object_video(34, "obj_d", 6, 60, OBJECT_CLASSES)
    gt["v_nopred"], _ = _object_video(35, "obj_e", 4, 0, OBJECT_CLASSES)
    gt["v_a"].append({"category": "boat", "trajectory": {"3": (0, 0, 9, 9), "4": (1, 0, 10, 9)}})   # never predicted
    pred["v_only_ufo"] = [{"category": "ufo", "trajectory": {"0": (0.0, 0.0, 5.0, 5.0)}}]           # a video outside gt
    # scores: distinct over the whole set (so inside every class), in steps of 1/1024
    n = sum(len(p) for p in pred.values())
    d = Draw(36, "obj_scores")
    keys = d.ints(n, 0, 1 << 30)
    rank = np.argsort(np.argsort(keys, kind="stable"), kind="stable")
    k = 0
    for tracks in pred.values():
        for t in tracks:
            t["score"] = float(rank[k] + 1) / 1024.0
            k += 1
    return gt, pred


def _action_video(seed, tag, n_gt, n_pred, classes, frames=60):
    d = Draw(seed, tag)
    gt = []
    for _ in range(n_gt):
        b = d.int(0, frames - 10)
        e = d.int(b + 1, min(frames, b + 30) + 1)
        gt.append({"category": classes[d.int(0, len(classes))], "duration": (b, e), "trajectory": int_traj(d, e - b)})
    preds = []
    for _ in range(n_pred):
        kind = d.int(0, 4)
        score = d.int(0, 32) / 32.0                      # many equal scores: the reference's sorted() is stable
        if kind < 3 and gt:
            g = gt[d.int(0, len(gt))]
            b, e = g["duration"]
            nb = max(0, b + (0 if kind == 0 else d.int(-4, 5)))
            cat = g["category"] if kind < 2 else classes[d.int(0, len(classes))]
            preds.append({"category": cat, "duration": [nb, nb + e - b], "trajectory": jitter(d, g["trajectory"], 2),
                          "score": score})
        else:
            b = d.int(0, frames - 10)
            e = d.int(b + 1, min(frames, b + 30) + 1)
            preds.append({"category": (classes + ("sleep",))[d.int(0, len(classes) + 1)], "duration": [b, e],
                          "trajectory": jitter(d, int_traj(d, e - b)), "score": score})
    return gt, preds


def g13_action_case():
    """(groundtruth, prediction): the action set of g13."""
    gt, pred = {}, {}
    gt["a_0"], pred["a_0"] = _action_video(41, "act_0", 12, 50, ACTION_CLASSES)
    gt["a_1"], pred["a_1"] = _action_video(42, "act_1", 8, 40, ACTION_CLASSES[:2])
    gt["a_2"], pred["a_2"] = _action_video(43, "act_2", 6, 30, ACTION_CLASSES[1:])
    gt["a_nopred"], _ = _action_video(44, "act_3", 3, 0, ACTION_CLASSES)
    _, pred["a_absent"] = _action_video(45, "act_4", 4, 10, ACTION_CLASSES)       # a video that the ground truth lacks
    gt["a_0"].append({"category": "swim", "duration": (2, 5), "trajectory": [(0, 0, 9, 9)] * 3})   # never predicted
    # a hit at vIoU exactly 0.5 (half the pixels of every frame) and a duplicate of it that finds the ground truth taken
    gt["a_1"].append({"category": "wave", "duration": (50, 53), "trajectory": [(0, 0, 9, 9)] * 3})
    for s in (0.99, 0.98):
        pred["a_1"].append({"category": "wave", "duration": [50, 53], "trajectory": [(0.0, 0.0, 9.0, 4.0)] * 3, "score": s})
    return gt, pred


def g13_annotation():
    """A VidOR-style annotation: 3 objects over 12 frames (object 2 from frame 4 on, object 1 missing in frame 7), 5
    relation instances of which 3 have an action predicate."""
    d = Draw(46, "anno13")
    objs = [{"tid": 0, "category": "dog"}, {"tid": 1, "category": "person"}, {"tid": 2, "category": "ball"}]
    frames = []
    for f in range(12):
        fr = []
        for tid in (2, 0, 1) if f % 2 else (0, 1, 2):
            if (tid == 2 and f < 4) or (tid == 1 and f == 7):
                continue
            x, y = d.int(0, 300), d.int(0, 200)
            fr.append({"tid": tid, "bbox": {"xmin": x, "ymin": y, "xmax": x + d.int(10, 50), "ymax": y + d.int(10, 50)}})
        frames.append(fr)
    rels = [{"subject_tid": 0, "object_tid": 1, "predicate": "left", "begin_fid": 0, "end_fid": 6},
            {"subject_tid": 1, "object_tid": 0, "predicate": "right", "begin_fid": 2, "end_fid": 12},
            {"subject_tid": 0, "object_tid": 2, "predicate": "chase", "begin_fid": 4, "end_fid": 9},
            {"subject_tid": 1, "object_tid": 2, "predicate": "chase", "begin_fid": 5, "end_fid": 10},
            {"subject_tid": 2, "object_tid": 1, "predicate": "next_to", "begin_fid": 8, "end_fid": 12}]
    return {"video_id": "anno13", "frame_count": 12, "width": 640, "height": 360, "subject/objects": objs,
            "trajectories": frames, "relation_instances": rels}
