"""Plain-loop numpy restatement of `tspn_span_match_f64` (DESIGN.md §2 "span match") and the association that only applies
its answer.

* `span_match`: the two stages pair by pair - the gate tests, `association._cubic_iou_1x1` on the window slices (the
  rounding recipe of the reference's trajectory.py), -1 for every pair that is no candidate; then the greedy pass.
* `segment_arrays`: the arrays of the C entry from a segment's state, written independently of the package's own packing.
* `associate`: `span_relations_reference.associate` with the per-candidate scan replaced by one `span_match` per segment.
"""
import numpy as np

from span_relations_reference import _merge


def span_match(rel_boxes, rel_range, rel_fend, rel_triplet, trk_boxes, pred_triplet, pred_pair, pred_span, iou_thr=0.5):
    """-> (match int32 [P], iou float32 [U,P,2]); operands as the C entry takes them (numpy)."""
    from tspn_mi355x.association import _cubic_iou_1x1
    U, P = len(rel_fend), len(pred_triplet)
    N, L = trk_boxes.shape[0], trk_boxes.shape[1]
    iou = np.full((U, P, 2), -1.0, dtype=np.float32)
    for u in range(U):
        for p in range(P):
            a, e = int(pred_span[p, 0]), int(pred_span[p, 1])
            if not (0 <= a < e <= L) or not all(0 <= int(j) < N for j in pred_pair[p]):
                continue
            if tuple(int(v) for v in rel_triplet[u]) != tuple(int(v) for v in pred_triplet[p]):
                continue
            if not a < int(rel_fend[u]):
                continue
            if not all(int(rel_range[u, c, 0]) <= a < int(rel_range[u, c, 1]) <= e for c in range(2)):
                continue
            for c in range(2):
                end = int(rel_range[u, c, 1])
                iou[u, p, c] = _cubic_iou_1x1(rel_boxes[u, c, a:end], trk_boxes[int(pred_pair[p, c]), a:end])
    match = np.full((P,), -1, dtype=np.int32)
    taken = np.zeros((U,), dtype=bool)
    for p in range(P):
        for u in range(U):
            if not taken[u] and float(iou[u, p, 0]) >= iou_thr and float(iou[u, p, 1]) >= iou_thr:
                match[p], taken[u] = u, True
                break
    return match, iou


def segment_arrays(rows, preds, boxes, fs):
    """rows: relation dicts of span_relations_reference.associate ({"trip", "s", "o", "fend"}, tracks {"ps", "pe", "rois"})
    in candidate order; preds: (score, triplet, (si, oi), (a, e)) in score order; boxes [N,L,4]; fs: the segment's first
    frame."""
    N, L = boxes.shape[0], boxes.shape[1]
    U, P = len(rows), len(preds)
    rel_boxes = np.zeros((U, 2, L, 4))
    rel_range = np.zeros((U, 2, 2), dtype=np.int32)
    rel_fend = np.zeros((U,), dtype=np.int32)
    rel_triplet = np.zeros((U, 3), dtype=np.int64)
    for u, r in enumerate(rows):
        for c, t in enumerate((r["s"], r["o"])):
            rel_range[u, c] = max(t["ps"] - fs, 0), max(t["pe"] - fs, 0)
            for f in range(L):                                   # frame by frame: the relation's box at video frame fs + f
                if t["ps"] <= fs + f < t["pe"]:
                    rel_boxes[u, c, f] = t["rois"][fs + f - t["ps"]]
        rel_fend[u] = r["fend"] - fs
        rel_triplet[u] = [int(v) for v in r["trip"]]
    pred_triplet = np.array([[int(v) for v in p[1]] for p in preds], dtype=np.int64).reshape(P, 3)
    pred_pair = np.array([[int(v) for v in p[2]] for p in preds], dtype=np.int32).reshape(P, 2)
    pred_span = np.array([[int(v) for v in p[3]] for p in preds], dtype=np.int32).reshape(P, 2)
    return rel_boxes, rel_range, rel_fend, rel_triplet, np.asarray(boxes, dtype=np.float64), pred_triplet, pred_pair, pred_span


def associate(short_term_relations, trajectories, max_traj_num_in_clip=100, match_fn=span_match, stats=None):
    """Span-bounded predictions -> serialised video relations (ids kept), the match computed ONCE per segment, before
    the loop, and only applied inside it.  `match_fn(*segment_arrays(...)) -> (match, iou)`."""
    rels, last, calls, pairs = [], [], 0, 0
    for i, (index, (preds, _, _)) in enumerate(sorted(short_term_relations, key=lambda x: int(x[0][1]))):
        _, fs, _ = index
        boxes = np.asarray(trajectories[index], dtype=np.float64)
        preds = sorted(preds, key=lambda x: x[0], reverse=True)[:max_traj_num_in_clip]
        rows = sorted(last, key=lambda r: np.mean(r["confs"]), reverse=True)
        match = None
        if i > 0 and preds and rows:
            match = match_fn(*segment_arrays(rows, preds, boxes, fs))[0]
            calls, pairs = calls + 1, pairs + len(rows) * len(preds)
        cur = []
        for k, (score, trip, (si, oi), (a, e)) in enumerate(preds):
            a, e = int(a), int(e)
            st = {"ps": fs + a, "pe": fs + e, "rois": boxes[int(si), a:e].copy()}
            ot = {"ps": fs + a, "pe": fs + e, "rois": boxes[int(oi), a:e].copy()}
            if match is not None and match[k] >= 0:
                hit = rows[match[k]]
                _merge(hit["s"], st)
                _merge(hit["o"], ot)
                hit["confs"].append(score)
                hit["fstart"], hit["fend"] = hit["s"]["ps"], hit["o"]["pe"]
            else:
                hit = {"trip": trip, "s": st, "o": ot, "confs": [score if i == 0 else 1], "fstart": st["ps"], "fend": st["pe"]}
                rels.append(hit)
            cur.append(hit)
        last = cur
    if stats is not None:
        stats.update(calls=calls, pairs=pairs)
    return [{"triplet": [int(v) for v in r["trip"]], "score": float(np.mean(r["confs"])),
             "duration": [int(r["fstart"]), int(r["fend"])],
             "sub_traj": list(map(tuple, r["s"]["rois"].tolist())), "obj_traj": list(map(tuple, r["o"]["rois"].tolist()))}
            for r in rels]
