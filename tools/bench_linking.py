#!/usr/bin/env python3
"""Time tracklet linking (`ops.link_detections`, `ops.link_fill`) on synthetic detections and print one JSON line.

Each video: --frames frames (default 900) of --dets detection rows (default 100): --objects objects (default 40) on smooth
paths with jitter, every detection missing with probability 0.1, the other rows low-score false positives at random places,
rows in a random order (numpy's seeded RandomState, one seed per video).  Batches of 1 and of --videos (default 16) videos.

Reported per batch (ms for the batch, the minimum and all of --repeat runs after one warm-up, HIP events): link_ms (the link
pass: one persistent workgroup per video), fill_ms (the fill pass for the confirmed tracks), tracks, confirmed tracks and
dropped births; for the single video also the time of the numpy restatement (tests/link_reference.py) on the same inputs in
the same process, with a check that every output is equal: that is the comparison, because there is no CPU path in the
package.  The card's clock state is read (not set) before and after.

The job may use 16 CPUs: the restatement is single-threaded numpy.

    python tools/bench_linking.py [--frames 900] [--dets 100] [--objects 40] [--videos 16] [--repeat 5] [--max-tracks 65536]
                                    [--no-python]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tspn_mi355x as tspn  # noqa: E402


def clocks():
    """The card's clock state as rocm-smi prints it (read only), or None where the tool is missing."""
    try:
        res = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--json"], stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL, text=True, timeout=60)
        return json.loads(res.stdout).get("card0") if res.returncode == 0 else None
    except (OSError, ValueError, subprocess.TimeoutExpired):
        return None


def synth(seed, frames, dets, objects):
    rs = np.random.RandomState(seed)
    boxes, scores = np.zeros((frames, dets, 4), np.float32), np.zeros((frames, dets), np.float32)
    classes, count = np.zeros((frames, dets), np.int64), np.full(frames, dets, np.int64)
    x0, y0 = rs.uniform(0, 1800, objects), rs.uniform(0, 1000, objects)
    vx, vy = rs.uniform(-1.5, 1.5, objects), rs.uniform(-0.8, 0.8, objects)
    size, cls = rs.uniform(40, 160, (objects, 2)), rs.randint(0, 35, objects)
    for t in range(frames):
        seen = np.flatnonzero(rs.uniform(size=objects) >= 0.1)[:dets]
        n = len(seen)
        cx, cy = x0[seen] + vx[seen] * t + rs.uniform(-2, 2, n), y0[seen] + vy[seen] * t + rs.uniform(-2, 2, n)
        wh = size[seen] + rs.uniform(-2, 2, (n, 2))
        fx, fy, fs = rs.uniform(0, 1900, dets - n), rs.uniform(0, 1050, dets - n), rs.uniform(20, 160, (dets - n, 2))
        cx, cy, wh = np.concatenate([cx, fx]), np.concatenate([cy, fy]), np.concatenate([wh, fs])
        order = rs.permutation(dets)
        boxes[t] = np.stack([cx - wh[:, 0] / 2, cy - wh[:, 1] / 2, cx + wh[:, 0] / 2, cy + wh[:, 1] / 2], 1)[order]
        scores[t] = np.concatenate([rs.uniform(0.6, 1.0, n), rs.uniform(0.05, 0.3, dets - n)])[order]
        classes[t] = np.concatenate([cls[seen], rs.randint(0, 35, dets - n)])[order]
    return boxes, scores, classes, count


def timed(fn, repeat):
    import torch
    fn()
    runs = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(round(a.elapsed_time(b), 4))
    return out, runs


def main():
    ap = argparse.ArgumentParser(description="Time the link and fill passes on synthetic detections; the job may use 16 CPUs "
                                             "(the numpy restatement is single-threaded).")
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-tracks", type=int, default=65536, help="ids per video (every tentative track uses one)")
    ap.add_argument("--no-python", action="store_true", help="skip the numpy restatement")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    ops = tspn.ops
    scenes = [synth(seed, args.frames, args.dets, args.objects) for seed in range(args.videos)]
    out = {"workload": "linking", "frames": args.frames, "dets": args.dets, "objects": args.objects, "repeat": args.repeat,
           "max_tracks": args.max_tracks, "cpu_count": os.cpu_count(), "omp_threads": os.environ.get("OMP_NUM_THREADS"),
           "clocks_before": clocks()}
    for V in sorted({1, args.videos}):
        det = tuple(torch.from_numpy(np.concatenate([s[k] for s in scenes[:V]])).to(dev) for k in range(4))
        off = [v * args.frames for v in range(V + 1)]
        link, link_ms = timed(lambda: ops.link_detections(*det, off, max_tracks=args.max_tracks), args.repeat)
        at = torch.nonzero(link[5] >= 3)
        sv, st = at[:, 0].contiguous(), at[:, 1].contiguous()
        fill, fill_ms = timed(lambda: ops.link_fill(det[0], link[0], link[3], link[4], sv, st, off), args.repeat)
        row = {"link_ms": min(link_ms), "link_ms_runs": link_ms, "fill_ms": min(fill_ms), "fill_ms_runs": fill_ms,
               "tracks": link[1].tolist(), "confirmed": int(at.shape[0]), "dropped": int(link[2].sum()),
               "detected_boxes": int((fill[1] == 1).sum()), "interpolated_boxes": int((fill[1] == 2).sum())}
        if V == 1 and not args.no_python:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import link_reference as ref
            tp = time.perf_counter()
            want = ref.link(*scenes[0], off, max_tracks=args.max_tracks)
            row["numpy_link_ms"] = round((time.perf_counter() - tp) * 1e3, 1)
            tp = time.perf_counter()
            want_b, want_s = ref.fill(want, scenes[0][0], off, *ref.confirmed(want))
            row["numpy_fill_ms"] = round((time.perf_counter() - tp) * 1e3, 1)
            keys = ("track_of_det", "n_tracks", "dropped", "first", "last", "hits", "cls", "score")
            row["numpy_equal"] = bool(all(np.array_equal(g.cpu().numpy(), want[k]) for g, k in zip(link, keys))
                                      and np.array_equal(fill[0].cpu().numpy(), want_b)
                                      and np.array_equal(fill[1].cpu().numpy(), want_s))
        out[f"videos_{V}"] = row
    out["clocks_after"] = clocks()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
