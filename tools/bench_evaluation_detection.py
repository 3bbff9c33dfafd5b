#!/usr/bin/env python3
"""Time `evaluate_objects` and `evaluate_actions` on a synthetic VidOR-scale set and print one JSON line.

The set comes from numpy's seeded RandomState: --videos videos (default 20) of --preds predicted (default 200) and --gts
ground-truth (default 30) trajectories each, categories drawn from --classes classes (default 80), 300 to 1000 frames a
trajectory out of a longer stretch (every frame kept with probability 7/8, so the frame sets have gaps).  Three
predictions in four copy a ground truth (jittered boxes, some frames dropped, its category mostly kept), the rest are
random.  The action set uses the same tracks with contiguous durations.

Reported per evaluator (ms for the whole set, mean over --repeat runs after one warm-up): pack_ms (host grouping and
packing), device_ms (uploads + kernels + the download, HIP events), kernel_ms (the kernels alone), host_ms (the AP
arithmetic in numpy), total_ms; the (prediction, ground truth) pair count and the number of chunks.  For the object
evaluator also pack_ms / total_ms with the trajectories given as (frames, boxes) array pairs instead of dicts.  Unless
--no-python, the time of the pure-Python restatement (tests/detection_eval_reference.py) on the same inputs in the same
process, with a check that its results are equal: that is the comparison, because there is no CPU path in the package.

The job may use 16 CPUs: the packing and the restatement are single-threaded Python, numpy's own threads are not needed.

    python tools/bench_evaluation_detection.py [--videos 20] [--preds 200] [--gts 30] [--classes 80] [--repeat 3]
                                               [--no-python]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tspn_mi355x as tspn  # noqa: E402


def synth(videos, n_pred, n_gt, classes, seed=0):
    """(object gt, object pred as dicts, object pred as array pairs, action gt, action pred)."""
    rs = np.random.RandomState(seed)
    ogt, opred, opairs, agt, apred = {}, {}, {}, {}, {}
    scores = (rs.permutation(videos * n_pred) + 1) / float(videos * n_pred)
    for v in range(videos):
        vid = f"v{v:03d}"
        tracks, gts, acts = [], [], []
        for _ in range(n_gt):
            n = int(rs.randint(300, 1001))
            lo = int(rs.randint(0, 400))
            xy = rs.uniform(50, 600, size=2) + np.cumsum(rs.uniform(-2, 2, size=(n, 2)), axis=0)
            wh = rs.uniform(30, 200, size=2)
            boxes = np.round(np.concatenate([xy, xy + wh], axis=1))
            keep = rs.randint(0, 8, size=n) > 0
            keep[0] = True
            cat = int(rs.randint(0, classes))
            tracks.append((lo, boxes, keep, cat))
            fs = (lo + np.flatnonzero(keep)).tolist()
            gts.append({"category": cat, "trajectory": {str(f): tuple(b) for f, b in zip(fs, boxes[keep].tolist())}})
            acts.append({"category": cat, "duration": (lo, lo + n), "trajectory": boxes})
        preds, pairs, pacts = [], [], []
        for i in range(n_pred):
            score = float(scores[v * n_pred + i])
            lo, boxes, keep, cat = tracks[rs.randint(0, n_gt)]
            n = boxes.shape[0]
            if i % 4:
                jb = boxes + rs.uniform(-6, 6, size=(n, 4))
                pk = keep & (rs.randint(0, 10, size=n) > 0)
                pcat = cat if i % 9 else int(rs.randint(0, classes))
                shift = int(rs.randint(-10, 11))
            else:
                xy = rs.uniform(50, 600, size=2) + np.cumsum(rs.uniform(-2, 2, size=(n, 2)), axis=0)
                jb = np.concatenate([xy, xy + rs.uniform(30, 200, size=2)], axis=1)
                pk = rs.randint(0, 8, size=n) > 0
                pcat = int(rs.randint(0, classes))
                shift = int(rs.randint(-200, 201))
            pk[0] = True
            fs = lo + np.flatnonzero(pk)
            pairs.append({"category": pcat, "score": score, "trajectory": (fs.astype(np.int32), np.ascontiguousarray(jb[pk]))})
            preds.append({"category": pcat, "score": score,
                          "trajectory": {str(f): tuple(b) for f, b in zip(fs.tolist(), jb[pk].tolist())}})
            b = max(0, lo + shift)
            pacts.append({"category": pcat, "score": score, "duration": (b, b + n), "trajectory": jb})
        ogt[vid], opred[vid], opairs[vid], agt[vid], apred[vid] = gts, preds, pairs, acts, pacts
    return ogt, opred, opairs, agt, apred


def timed(fn, gt, pred, dev, repeat):
    fn(gt, pred, device=dev)                               # warm-up (library load, allocator)
    runs = []
    for _ in range(repeat):
        st = {}
        res = fn(gt, pred, device=dev, stats=st)
        runs.append(st)
    out = {k: round(float(np.mean([r[k] for r in runs])), 3)
           for k in ("pack_ms", "device_ms", "kernel_ms", "host_ms", "total_ms")}
    out["candidates"], out["chunks"] = runs[-1]["candidates"], runs[-1]["chunks"]
    return res, out


def main():
    ap = argparse.ArgumentParser(description="Time evaluate_objects / evaluate_actions on a synthetic VidOR-scale set; "
                                             "the job may use 16 CPUs (packing and the Python restatement are "
                                             "single-threaded).")
    ap.add_argument("--videos", type=int, default=20)
    ap.add_argument("--preds", type=int, default=200)
    ap.add_argument("--gts", type=int, default=30)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-python", action="store_true", help="skip the pure-Python restatement")
    args = ap.parse_args()
    t0 = time.perf_counter()
    ogt, opred, opairs, agt, apred = synth(args.videos, args.preds, args.gts, args.classes)
    gen_s = time.perf_counter() - t0
    import torch
    dev = torch.device("cuda", 0)
    E = tspn.evaluation
    out = {"workload": "evaluation_detection", "videos": args.videos, "preds_per_video": args.preds,
           "gts_per_video": args.gts, "classes": args.classes, "repeat": args.repeat, "generate_s": round(gen_s, 2),
           "cpu_count": os.cpu_count(), "omp_threads": os.environ.get("OMP_NUM_THREADS")}
    obj, out["objects"] = timed(E.evaluate_objects, ogt, opred, dev, args.repeat)
    obj_pairs, st = timed(E.evaluate_objects, ogt, opairs, dev, args.repeat)
    out["objects"]["array_pairs_pack_ms"], out["objects"]["array_pairs_total_ms"] = st["pack_ms"], st["total_ms"]
    out["objects"]["array_pairs_equal"] = bool(obj_pairs == obj)
    out["objects"]["mean_ap"] = float(obj[0])
    act, out["actions"] = timed(E.evaluate_actions, agt, apred, dev, args.repeat)
    out["actions"]["mean_ap"] = float(act[0])
    if not args.no_python:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import detection_eval_reference as ref
        tp = time.perf_counter()
        want = ref.evaluate_objects(ogt, opred)
        out["objects"]["python_restatement_ms"] = round((time.perf_counter() - tp) * 1e3, 1)
        out["objects"]["python_restatement_equal"] = bool(want[:2] == obj)
        listed = {vid: [dict(a, trajectory=a["trajectory"].tolist()) for a in acts] for vid, acts in apred.items()}
        listed_gt = {vid: [dict(a, trajectory=a["trajectory"].tolist()) for a in acts] for vid, acts in agt.items()}
        tp = time.perf_counter()
        want = ref.evaluate_actions(listed_gt, listed)
        out["actions"]["python_restatement_ms"] = round((time.perf_counter() - tp) * 1e3, 1)
        out["actions"]["python_restatement_equal"] = bool(want[0] == act[0] and want[1] == act[1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
