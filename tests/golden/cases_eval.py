"""Inputs of the evaluation goldens (g12) and tests, regenerated bit for bit from the build-owned hash RNG.

`g12_case()` is a ground truth / prediction set that reaches every rule of the reference's relation evaluation
(lib/evaluation/visual_relation_detection.py, common.py): ties in score and in ov (duplicate ground truths), an ov of
exactly 0.5 from integer boxes, touching and disjoint durations, negative-width boxes, float and int boxes,
predictions with no same-triplet ground truth, a video with ground truth and no predictions, a video with no ground
truth, a (video, triplet) group of more than 64 ground truths, and string and integer triplets.
`g12_annotation()` is a small VidVRD-style annotation dict for the annotation reader."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tspn_mi355x import hashrng  # noqa: E402

SUBJECTS = ("dog", "person", "car")
PREDICATES = ("left", "behind", "chase")


class Draw:
    """Sequential integer / float draws from one hash-RNG stream."""

    def __init__(self, seed, tag):
        self.seed, self.tag, self.n = seed, tag, 0

    def ints(self, n, lo, hi):
        b = hashrng.bits(self.seed, self.tag, n, offset=self.n)
        self.n += n
        return lo + (b % np.uint64(hi - lo)).astype(np.int64)

    def int(self, lo, hi):
        return int(self.ints(1, lo, hi)[0])


def int_traj(d, n, w=640, h=360):
    """n integer boxes (Python int tuples, the JSON ground-truth form) drifting from a random start."""
    x0, y0 = d.int(0, w - 100), d.int(0, h - 100)
    bw, bh = d.int(20, 100), d.int(20, 100)
    dx, dy = d.ints(n, -2, 3), d.ints(n, -2, 3)
    out = []
    for i in range(n):
        x0, y0 = x0 + int(dx[i]), y0 + int(dy[i])
        out.append((x0, y0, x0 + bw, y0 + bh))
    return out


def jitter(d, traj, scale=4):
    """Float copy of a trajectory with sub-pixel jitter in steps of 1/8 (exact in float64)."""
    j = d.ints(4 * len(traj), -scale * 8, scale * 8 + 1) / 8.0
    return [tuple(float(c) + float(j[4 * i + k]) for k, c in enumerate(b)) for i, b in enumerate(traj)]


def rel(triplet, duration, sub, obj, score=None):
    r = {"triplet": triplet, "duration": list(duration), "sub_traj": sub, "obj_traj": obj}
    if score is not None:
        r["score"] = score
    return r


def random_video(seed, tag, n_gt, n_pred, triplet_of, frames=80):
    """n_gt integer-box ground truths and n_pred predictions: most are jittered copies of a ground truth (same or
    shifted duration), the rest random; scores in steps of 1/16 so that many tie."""
    d = Draw(seed, tag)
    gt = []
    for _ in range(n_gt):
        b = d.int(0, frames - 10)
        e = d.int(b + 1, min(frames, b + 40) + 1)
        gt.append(rel(triplet_of(d), (b, e), int_traj(d, e - b), int_traj(d, e - b)))
    preds = []
    for _ in range(n_pred):
        kind = d.int(0, 4)
        score = d.int(0, 16) / 16.0
        if kind < 3 and gt:
            g = gt[d.int(0, len(gt))]
            b, e = g["duration"]
            shift = 0 if kind == 0 else d.int(-5, 6)
            nb, ne = max(0, b + shift), max(0, b + shift) + (e - b)
            sub, obj = jitter(d, g["sub_traj"]), jitter(d, g["obj_traj"])
            trip = g["triplet"] if kind < 2 else triplet_of(d)
            preds.append(rel(trip, (nb, ne), sub, obj, score))
        else:
            b = d.int(0, frames - 10)
            e = d.int(b + 1, min(frames, b + 40) + 1)
            preds.append(rel(triplet_of(d), (b, e), jitter(d, int_traj(d, e - b)), jitter(d, int_traj(d, e - b)),
                             score))
    return gt, preds


def str_triplet(d):
    return [SUBJECTS[d.int(0, 3)], PREDICATES[d.int(0, 3)], SUBJECTS[d.int(0, 3)]]


def int_triplet(d):
    return [d.int(0, 2), d.int(0, 2), d.int(0, 2)]


def edge_video():
    """Hand-made cases: ov exactly 0.5, touching / disjoint durations, negative-width boxes, duplicate ground truths
    (ov ties), equal scores, a prediction with no same-triplet ground truth."""
    T = ("person", "ride", "bicycle")
    box = [(0, 0, 9, 9)] * 3
    half = [(0, 0, 9, 4)] * 3                         # 50 of 100 pixels in every frame: vIoU exactly 0.5
    neg = [(10, 0, 5, 9), (10, 0, 5, 9)]              # width -4: a negative volume
    gt = [rel(T, (0, 3), box, box),
          rel(T, (0, 3), box, box),                   # duplicate: ov ties, the lower index wins
          rel(T, (10, 12), neg, neg),
          rel(("person", "ride", "bicycle"), (20, 23), box, box),
          rel(("dog", "sit", "sofa"), (0, 3), box, box)]
    preds = [rel(T, (0, 3), half, half, 0.5),        # ov 0.5 against gt 0 and 1: gt 0
             rel(T, (0, 3), half, half, 0.5),        # equal score, ov 0.5 against gt 1 (gt 0 taken)
             rel(T, (0, 3), box, box, 0.5),          # equal score again: both taken, a miss
             rel(T, (3, 6), box, box, 0.9),          # touching gt 0/1's end: disjoint, ov 0
             rel(T, (23, 26), box, box, 0.25),       # touching gt 3's end
             rel(T, (19, 22), [(0.5, 0.0, 9.5, 9.0)] * 3, [(0, 0, 9, 9)] * 3, 0.75),   # partial overlap of gt 3
             rel(T, (11, 13), [(10.0, 0.0, 5.0, 9.0)] * 2, [(9.0, 0.0, 6.0, 9.0)] * 2, 0.3),   # negative widths
             rel(("cat", "sit", "sofa"), (0, 3), box, box, 0.95),                 # no ground truth of its triplet
             rel(("dog", "sit", "sofa"), (1, 3), box[:2], box[:2], 0.95)]
    return gt, preds


def big_group_video(seed=5, n_gt=70, n_pred=90):
    """One triplet with more than 64 ground truths (several with identical boxes) and many predictions."""
    d = Draw(seed, "big")
    T = [7, 1, 3]
    gt = []
    for i in range(n_gt):
        if i % 10 == 9:
            gt.append(dict(gt[i - 1]))             # a duplicate of the previous ground truth
            continue
        b = d.int(0, 20)
        e = b + d.int(5, 20)
        gt.append(rel(T, (b, e), int_traj(d, e - b, 200, 200), int_traj(d, e - b, 200, 200)))
    preds = []
    for i in range(n_pred):
        g = gt[d.int(0, n_gt)]
        sub = jitter(d, g["sub_traj"], 2) if i % 3 else [tuple(float(c) for c in bb) for bb in g["sub_traj"]]
        preds.append(rel(T, g["duration"], sub, jitter(d, g["obj_traj"], 2), d.int(0, 8) / 8.0))
    return gt, preds


def g12_case():
    """(groundtruth, prediction, train_triplets): the g12 set."""
    gt, pred = {}, {}
    gt["v_str"], pred["v_str"] = random_video(1, "str", 24, 80, str_triplet)
    gt["v_edges"], pred["v_edges"] = edge_video()
    gt["v_int"], pred["v_int"] = random_video(2, "int", 16, 40, int_triplet)
    gt["v_big"], pred["v_big"] = big_group_video()
    gt["v_nopred"], _ = random_video(3, "nopred", 5, 0, str_triplet)
    pred["v_nopred"] = []
    gt["v_nogt"] = []
    _, pred["v_nogt"] = random_video(4, "nogt", 3, 12, str_triplet)
    train = [("dog", "left", "person"), ("person", "ride", "bicycle"), ("dog", "chase", "car"), (0, 1, 0), (7, 1, 3)]
    return gt, pred, train


def g12_annotation():
    """A VidVRD-style annotation: 3 objects, 12 frames (not every object in every frame), 4 relations."""
    d = Draw(6, "anno")
    objs = [{"tid": 0, "category": "dog"}, {"tid": 1, "category": "person"}, {"tid": 2, "category": "ball"}]
    frames = []
    for f in range(12):
        fr = []
        for tid in range(3):
            if tid == 2 and f < 4:
                continue
            x, y = d.int(0, 300), d.int(0, 200)
            fr.append({"tid": tid, "bbox": {"xmin": x, "ymin": y, "xmax": x + d.int(10, 50), "ymax": y + d.int(10, 50)}})
        frames.append(fr)
    rels = [{"subject_tid": 0, "object_tid": 1, "predicate": "left", "begin_fid": 0, "end_fid": 6},
            {"subject_tid": 1, "object_tid": 0, "predicate": "right", "begin_fid": 2, "end_fid": 12},
            {"subject_tid": 0, "object_tid": 2, "predicate": "chase", "begin_fid": 4, "end_fid": 9},
            {"subject_tid": 0, "object_tid": 1, "predicate": "left", "begin_fid": 8, "end_fid": 12}]
    return {"video_id": "anno0", "frame_count": 12, "width": 640, "height": 360, "subject/objects": objs,
            "trajectories": frames, "relation_instances": rels}
