#!/usr/bin/env python3
"""Time the labelling of a loader batch from ground-truth relation instances (`dataset.proposal_pair_lists` with
`gt_rel_insts`: tspn_pair_labels_f32 on the kept pair tables) against the same call with `pred_labels` computed on the host
by the numpy restatement (tests/pair_labels_reference.py), the restatement's time included.  Prints one JSON line.

Default batch (cfg2-like): 16 segments, 32 proposals + 4 ground-truth tracks each (1260 stored pairs, 992 kept), K = 132,
20 instances per segment, G = 4, feature rows of --F floats (256: the feature gather is the same work in both paths and is
not what is compared).  Before anything is timed the labels, spans and counts of the device path are compared with the
restatement.  The paths alternate inside one process, --repeat rounds after --warmup unmeasured ones; a round of a path is
one call followed by a device synchronisation, wall time in ms: median [min, max].  `entry` is `ops.pair_labels` alone on the
batch's kept pair tables, --inner calls between two HIP events.

    python tools/bench_pair_labels.py [--S 16 --N 32 --gt 4 --K 132 --R 20 --G 4 --F 256] [--repeat 20] [--warmup 3]
    python tools/bench_pair_labels.py --entry-only 50        (50 calls of the entry and nothing else: for a kernel trace)
    python tools/bench_pair_labels.py --pred-labels-only     (the `pred_labels=` path alone, labels computed beforehand: runs
                                                              on a tree without the entry too, given this file's directory
                                                              and tests/pair_labels_reference.py through --root)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate(paths, warmup, repeat):
    ms = {k: [] for k in paths}
    for r in range(warmup + repeat):
        for k, fn in paths.items():
            t = _wall(fn)
            if r >= warmup:
                ms[k].append(t)
    return {k: _stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("S", 16), ("N", 32), ("gt", 4), ("K", 132), ("R", 20), ("G", 4), ("F", 256), ("repeat", 20),
                          ("warmup", 3), ("inner", 20), ("entry-only", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--pred-labels-only", action="store_true")
    ap.add_argument("--root", default=HERE_ROOT, help="the tree whose package is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE_ROOT, "tests"))         # the restatement (the timed tree may not have it)
    sys.path.insert(0, a.root)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import pair_labels_reference as ref
    import tspn_mi355x as tspn
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_labels: needs a HIP device (there is nothing to time on a CPU)")
    dev, ds, K, G, thr = torch.device("cuda", 0), tspn.dataset, a.K, a.G, 0.5
    segs = []
    for s in range(a.S):
        seg = ref.make_segment(900 + s, a.N, tuple(range(a.gt)), 1, a.R, K, thr, fstart=15 * s)
        M = a.N + a.gt
        seg["pairs"] = np.array([(i, j) for i in range(M) for j in range(M) if i != j], np.int64)
        rs = np.random.RandomState(s)
        seg["feats"] = rs.uniform(0, 1, (len(seg["pairs"]), a.F)).astype(np.float32)
        seg["cls"] = rs.uniform(-1, 1, (a.N, 35)).astype(np.float32)
        segs.append(seg)
    base = [dict(pairs=s["pairs"], feats=torch.from_numpy(s["feats"]).to(dev), iou=s["iou"], trackid=s["trackid"],
                 cls_logits=s["cls"]) for s in segs]

    def host_labels():
        return [ref.segment_ref(s, K, 0, thr, "last")[0] for s in segs]

    def by_pred_labels(labels=None):
        labels = host_labels() if labels is None else labels
        return ds.proposal_pair_lists([dict(d, pred_labels=l) for d, l in zip(base, labels)], preprocess=False, device=dev)

    shape = {"S": a.S, "N": a.N, "gt": a.gt, "K": K, "R": a.R, "G": G, "F": a.F, "stored_pairs": sum(len(s["pairs"]) for s in segs)}
    if a.pred_labels_only:
        fixed = host_labels()
        res = {"shape": shape, "root": a.root, "repeat": a.repeat, "warmup": a.warmup,
               "wall_ms": _alternate({"pred_labels_path": lambda: by_pred_labels(fixed)}, a.warmup, a.repeat)}
        print(json.dumps(res))
        return

    def by_insts():
        return ds.proposal_pair_lists([dict(d, gt_rel_insts=s["insts"], segment=s["frames"]) for d, s in zip(base, segs)],
                                      preprocess=False, device=dev, max_spans=G, iou_thres=thr, num_predicates=K)

    # the entry alone, on the kept pair tables of the batch
    kept = [dict(s, pairs=s["pairs"][(s["trackid"][s["pairs"]] < 0).all(axis=1)]) for s in segs]
    case = {"K": K, "G": G, "thr": thr, "merge": "last", "segments": kept}
    b = {k: torch.from_numpy(v).to(dev) for k, v in ref.batch_of(case).items()}

    def entry():
        return tspn.ops.pair_labels(b["pairs"], b["trackid"], b["iou"], b["insts"], K, thr, "last", G, b["seg_frames"],
                                    b["pair_off"], b["track_off"], b["iou_off"], b["inst_off"])

    P = int(b["pairs"].shape[0])
    if a.entry_only:
        for _ in range(a.entry_only):
            entry()
        torch.cuda.synchronize()
        print(json.dumps({"entry_calls": a.entry_only, "P": P, "K": K, "G": G, "R": int(b["insts"].shape[0])}))
        return
    want = ref.case_ref(case)
    got = entry()
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), "the entry is wrong"
    off = 0
    for (_, tl), (_, tl2), s in zip(by_insts(), by_pred_labels(), kept):
        n = len(s["pairs"])
        assert torch.equal(tl.target, tl2.target) and np.array_equal(tl.target.cpu().numpy(), want[0][off:off + n])
        assert np.array_equal(tl.get_field("spans").cpu().numpy(), want[1][off:off + n]), "the loader path is wrong"
        off += n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms = []
    for r in range(a.warmup + a.repeat):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            entry()
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            dev_ms.append(e0.elapsed_time(e1) / a.inner)
    t0 = time.perf_counter()
    host_labels()
    restatement_ms = (time.perf_counter() - t0) * 1e3
    fixed = host_labels()
    res = {"shape": dict(shape, kept_pairs=P, instances=int(b["insts"].shape[0])),
           "positive_rows": int((want[0].sum(axis=1) > 0).sum()), "pairs_with_spans": int((want[2] > 0).sum()),
           "label_bytes": P * K * 4, "span_bytes": P * G * 16 + P * 4,
           "repeat": a.repeat, "warmup": a.warmup, "inner": a.inner,
           "wall_ms": _alternate({"gt_rel_insts": by_insts, "host_restatement_then_pred_labels": by_pred_labels,
                                  "pred_labels_given": lambda: by_pred_labels(fixed)}, a.warmup, a.repeat),
           "restatement_alone_ms": round(restatement_ms, 3), "entry_device_ms": _stats(dev_ms)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
