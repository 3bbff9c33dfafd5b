#!/usr/bin/env python3
"""Time `tspn_mi355x.evaluation.evaluate` on a synthetic VidOR-scale set and print one JSON line.

The set comes from the hash RNG: --videos videos (default 20) of --preds predictions (default 11 000, the
association's VidOR-scale output) and about --gts ground truths each (default 60), durations log-uniform in
[30, 1500] frames, triplets drawn from a skewed (Zipf-like) distribution over --triplets triplets.  Half of the
predictions copy a ground truth's triplet and objects (unrounded boxes, duration shifted by up to 20 frames).
Trajectories are views of per-video object tracks, so the set itself stays small in memory.

Reported (ms per video, mean over --repeat runs after one warm-up, trajectories given as float64 arrays): pack_ms
(host grouping + packing), device_ms (uploads + the three kernels + the download, HIP events), kernel_ms (the kernels
alone), host_ms (numpy metrics), total_ms; the (prediction, same-triplet ground truth) pair count and the number of
chunks; the packing and total time of the first video in the JSON form (lists of box lists, what load_prediction
returns); and, unless --no-python, the per-video time of the Python-float restatement in tests/test_gpu_evaluation.py
on the first video, with a check that its hits are equal.

    python tools/bench_evaluation.py [--videos 20] [--preds 11000] [--repeat 3] [--no-python]
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
from tspn_mi355x import hashrng  # noqa: E402


def synth_video(seed, n_pred, n_gt, n_trip, frames=3000, n_obj=40):
    rs_bits = iter(hashrng.bits(seed, "bench_eval", 16 * (n_pred + n_gt) + 8 * n_obj))

    def u():
        return (int(next(rs_bits)) >> 11) * (1.0 / 9007199254740992.0)

    def dur():
        n = int(round(30.0 * (50.0 ** u())))                 # log-uniform in [30, 1500]
        b = int(u() * (frames - n))
        return b, b + n
    # per-object tracks: a drifting box per frame
    steps = (hashrng.uniform(seed, "bench_eval_tracks", (n_obj, frames, 2), -2.0, 2.0, np.float64)).cumsum(axis=1)
    start = hashrng.uniform(seed, "bench_eval_start", (n_obj, 1, 2), 100.0, 900.0, np.float64)
    size = hashrng.uniform(seed, "bench_eval_size", (n_obj, 1, 2), 20.0, 200.0, np.float64)
    xy = start + steps
    tracks = np.ascontiguousarray(np.concatenate([xy, xy + size], axis=2))
    itracks = np.round(tracks)
    zipf = 1.0 / np.arange(1, n_trip + 1) ** 1.1
    cdf = np.cumsum(zipf) / zipf.sum()

    def triplet():
        t = int(np.searchsorted(cdf, u()))
        return [t % 80, t // 80, (7 * t) % 80]
    gt, objs = [], []
    for _ in range(n_gt):
        b, e = dur()
        s, o = int(u() * n_obj), int(u() * n_obj)
        objs.append((s, o))
        gt.append({"triplet": triplet(), "duration": [b, e], "sub_traj": itracks[s, b:e], "obj_traj": itracks[o, b:e]})
    preds = []
    for i in range(n_pred):
        if i % 2 and gt:             # a copy of a ground truth: same objects (unrounded tracks), shifted duration
            k = int(u() * len(gt))
            b, e = gt[k]["duration"]
            sh = int(u() * 40) - 20
            b, e = max(0, b + sh), min(frames, e + sh)
            s, o = objs[k]
            preds.append({"triplet": list(gt[k]["triplet"]), "duration": [b, e], "score": u(),
                          "sub_traj": tracks[s, b:e], "obj_traj": tracks[o, b:e]})
        else:
            b, e = dur()
            preds.append({"triplet": triplet(), "duration": [b, e], "score": u(),
                          "sub_traj": tracks[int(u() * n_obj), b:e], "obj_traj": tracks[int(u() * n_obj), b:e]})
    return gt, preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=20)
    ap.add_argument("--preds", type=int, default=11000)
    ap.add_argument("--gts", type=int, default=60)
    ap.add_argument("--triplets", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-python", action="store_true")
    args = ap.parse_args()
    t0 = time.perf_counter()
    gt, pred = {}, {}
    for v in range(args.videos):
        gt[f"v{v:03d}"], pred[f"v{v:03d}"] = synth_video(v, args.preds, args.gts, args.triplets)
    gen_s = time.perf_counter() - t0
    import torch
    dev = torch.device("cuda", 0)
    tspn.evaluation.evaluate(gt, pred, device=dev)          # warm-up (library load, allocator)
    runs = []
    for _ in range(args.repeat):
        st = {}
        res = tspn.evaluation.evaluate(gt, pred, device=dev, stats=st)
        runs.append(st)
    per = {k: float(np.mean([r[k] for r in runs])) / args.videos
           for k in ("pack_ms", "device_ms", "kernel_ms", "host_ms", "total_ms")}
    out = {"workload": "evaluation", "videos": args.videos, "preds_per_video": args.preds, "gts_per_video": args.gts,
           "candidates": runs[-1]["candidates"], "chunks": runs[-1]["chunks"], "repeat": args.repeat,
           **{k + "_per_video": round(v, 3) for k, v in per.items()},
           "mean_ap": float(res[0]), "rec_at_50": float(res[1][50]), "prec_at_1": float(res[2][1]),
           "generate_s": round(gen_s, 2), "cpu_count": os.cpu_count(),
           "omp_threads": os.environ.get("OMP_NUM_THREADS")}
    # the JSON form (lists of box lists, as load_prediction returns them) of the first video
    vid = next(iter(gt))
    g1 = {vid: [dict(r, sub_traj=r["sub_traj"].tolist(), obj_traj=r["obj_traj"].tolist()) for r in gt[vid]]}
    p1 = {vid: [dict(r, sub_traj=r["sub_traj"].tolist(), obj_traj=r["obj_traj"].tolist()) for r in pred[vid]]}
    st = {}
    tspn.evaluation.evaluate(g1, p1, device=dev, stats=st)
    out["list_form_pack_ms_per_video"] = round(st["pack_ms"], 1)
    out["list_form_total_ms_per_video"] = round(st["total_ms"], 1)
    if not args.no_python:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import test_gpu_evaluation as ref
        tp = time.perf_counter()
        _, hit, _ = ref.greedy_py(g1[vid], p1[vid])
        out["python_restatement_ms_per_video"] = round((time.perf_counter() - tp) * 1e3, 1)
        info = tspn.evaluation.evaluate(g1, p1, device=dev, details=True)[3]
        out["python_restatement_hits_equal"] = bool(np.array_equal(info[vid]["hit"], hit))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
