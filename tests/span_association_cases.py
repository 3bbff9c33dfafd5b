"""Span-bounded association scenarios shared by tests/test_span_match_host.py, tests/test_gpu_span_match.py and
tools/bench_association.py --spans: the synthetic videos of `cases.g9_scenario` with a span drawn for every prediction."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402

# (seed, segments, tracklets, predictions per segment) of the scenarios the tests run.  What the host path
# (`greedy_relational_association(device=None)`, cap 100) makes of them:
#   scenario             relations   longer than 30 frames   starts off the 15-frame grid   IoU lookups
#   (11, 5, 7, 40)          171              22                        73                       45
#   (23, 12, 32, 120)      1161              29                       552                      325
#   (7, 8, 16, 60)          447              25                       215                       79
SCENARIOS = [(11, 5, 7, 40), (23, 12, 32, 120), (7, 8, 16, 60)]


def spanned(seed, n_seg, n_trk, n_pred):
    """`cases.g9_scenario` with a fourth element [a, e) per prediction, drawn from RandomState(seed + 1000) in list order:
    about half of the spans start at the segment's first frame and six in ten reach its last (only those can be
    continued by the next segment, whose spans must start inside them)."""
    rels, trajs = cases.g9_scenario(seed=seed, n_seg=n_seg, n_trk=n_trk, n_pred=n_pred)
    rs = np.random.RandomState(seed + 1000)
    out = []
    for index, (preds, iou, trackid) in rels:
        cut = []
        for pred in preds:
            a = 0 if rs.uniform() < 0.5 else rs.randint(0, 25)
            e = 30 if rs.uniform() < 0.6 else rs.randint(a + 1, 31)
            cut.append(tuple(pred) + (np.array([a, e]),))
        out.append((index, (cut, iou, trackid)))
    return out, trajs
