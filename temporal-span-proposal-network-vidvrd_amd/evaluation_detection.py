"""Video object detection and action detection evaluation on the GPU: trajectory mAP and per-predicate mAP.

Same arguments, return values (numpy types included) and numbers as the reference's
`lib.evaluation.video_object_detection.evaluate` (video_object_detection.py:12-129, common.py:4-62) and
`lib.evaluation.action_detection.evaluate` (action_detection.py:6-97, common.py:65-106); they print nothing.
DESIGN.md 2 freezes the semantics.

What runs where:
  * host: validation, the score order (`np.argsort(-scores, kind="stable")`; the reference's object evaluator uses
    numpy's default sort, which is unspecified on ties, so the two agree whenever the scores of a class are distinct),
    grouping by (video, category), packing, and the AP arithmetic in numpy with the reference's types;
  * device, objects (csrc/evalobj/tspn_eval_objects.hip): the tIoU of every (prediction, same-class ground truth) pair
    of a video over their common frames, each prediction's (max_overlap, max_index), and the first-claimant match;
  * device, actions (csrc/eval/tspn_eval.hip): the relation evaluator's three kernels, with each instance packed as a
    relation whose subject and object trajectories are the same box rows (min(v, v) is v, bit for bit).

Only (video, category) groups that have both predictions and ground truths are packed; a prediction of any other group
is a false positive without a look at its trajectory.

Deliberate additions to the reference's behaviour (ValueError naming the video and the item): a non-finite score or
box; two keys of one trajectory that parse to the same frame; a frame id outside int32; `thresh_t <= 0`; an action
trajectory whose length is not `end - begin`.  A zero sIoU / vIoU denominator or two empty object trajectories raise
ZeroDivisionError and a predicted video of a ground-truth class that the ground truth lacks raises KeyError, as in the
reference.  There is no CPU path.
"""
import time

import numpy as np
import torch

from . import ops
from .evaluation import (DEFAULT_MAX_BYTES, DEFAULT_MAX_CANDIDATES, _as_boxes, _chunk_bytes, _chunks, _detection_scores,
                         _match_chunk, _resolve_device, voc_ap)

__all__ = ["evaluate_objects", "evaluate_actions", "object_instances", "action_instances"]

_INT32 = np.iinfo(np.int32)


# ---------------------------------------------------------------------------------------------------- annotations
def object_instances(annotation):
    """The object (trajectory) list of one VidVRD / VidOR annotation dict, as the reference's `Dataset.get_object_insts`
    builds it (lib/dataset/dataset.py:119-141): tid, category and trajectory {str(frame index): (xmin, ymin, xmax,
    ymax)} over the frames that show the object, in order of first appearance."""
    category = {so["tid"]: so["category"] for so in annotation["subject/objects"]}
    boxes = {}
    for fid, frame in enumerate(annotation["trajectories"]):
        for b in frame:
            bb = b["bbox"]
            boxes.setdefault(b["tid"], {})[str(fid)] = (bb["xmin"], bb["ymin"], bb["xmax"], bb["ymax"])
    return [{"tid": tid, "category": category[tid], "trajectory": t} for tid, t in boxes.items()]


def action_instances(annotation, action_predicates):
    """The action list of one annotation dict, as the reference's `Dataset.get_action_insts` builds it
    (lib/dataset/dataset.py:143-171): for every relation instance whose predicate is in `action_predicates`, category
    (the predicate), duration (begin_fid, end_fid) and the subject's boxes over the frames of the duration that show it
    (so the trajectory is shorter than the duration where the subject is missing from a frame)."""
    out = []
    for a in annotation["relation_instances"]:
        if a["predicate"] not in action_predicates:
            continue
        b, e = a["begin_fid"], a["end_fid"]
        traj = [(o["bbox"]["xmin"], o["bbox"]["ymin"], o["bbox"]["xmax"], o["bbox"]["ymax"])
                for frame in annotation["trajectories"][b:e] for o in frame if o["tid"] == a["subject_tid"]]
        out.append({"category": a["predicate"], "duration": (b, e), "trajectory": traj})
    return out


# ---------------------------------------------------------------------------------------------------- shared
def _budgets(who, max_candidates, max_bytes):
    max_candidates = DEFAULT_MAX_CANDIDATES if max_candidates is None else int(max_candidates)
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    if max_candidates < 1 or max_bytes < 1:
        raise ValueError(f"{who}: max_candidates and max_bytes must be positive")
    return max_candidates, max_bytes


def _gt_classes(groundtruth):
    """The reference's `gt_classes` set, built by the same insertions (so it iterates in the same order in one process)
    and, per video, the ground-truth indices of each category."""
    classes, by_class = set(), {}
    for vid, tracks in groundtruth.items():
        mine = by_class[vid] = {}
        for k, t in enumerate(tracks):
            classes.add(t["category"])
            mine.setdefault(t["category"], []).append(k)
    return classes, by_class


def _prepare(who, groundtruth, prediction, gt_classes, gt_by_class, missing_video_raises, rows_of, bytes_of):
    """Per predicted video: the stable descending score order over all its predictions, and per category of
    `gt_classes` the (category, positions in that order, ground-truth indices) group, for the categories that have both
    here; the predictions of any other category are false positives (`by_cat` keeps their positions for the AP)."""
    videos = []
    for vid, tracks in prediction.items():
        n = len(tracks)
        scores = np.fromiter((t["score"] for t in tracks), dtype=np.float64, count=n)
        bad = np.flatnonzero(~np.isfinite(scores))
        if bad.size:
            raise ValueError(f"{who}: video {vid!r}, prediction {int(bad[0])}: non-finite score {scores[bad[0]]!r}")
        order = np.argsort(-scores, kind="stable")
        by_cat = {}
        for pos, i in enumerate(order.tolist()):
            c = tracks[i]["category"]
            if c in gt_classes:
                by_cat.setdefault(c, []).append(pos)
        if by_cat and vid not in groundtruth:
            if missing_video_raises:
                raise KeyError(vid)
            gts = {}
        else:
            gts = gt_by_class.get(vid, {})
        groups = [(c, np.array(p, dtype=np.int64), np.array(gts[c], dtype=np.int64)) for c, p in by_cat.items() if c in gts]
        sel_p = order[np.concatenate([p for _, p, _ in groups])] if groups else np.zeros(0, dtype=np.int64)
        sel_g = np.concatenate([g for _, _, g in groups]) if groups else np.zeros(0, dtype=np.int64)
        rows = sum(rows_of(tracks[i]) for i in sel_p.tolist()) + \
            sum(rows_of(groundtruth[vid][k]) for k in sel_g.tolist())
        cand = int(sum(len(p) * len(g) for _, p, g in groups))
        videos.append({"vid": vid, "preds": tracks, "gt": groundtruth.get(vid, []), "scores": scores, "order": order,
                       "by_cat": by_cat, "groups": groups, "candidates": cand,
                       "bytes": bytes_of(rows, len(sel_p), len(sel_g), len(groups), cand),
                       "hit": np.zeros(n, dtype=bool), "match": np.full(n, -1, dtype=np.int64)})
    return videos


def _class_columns(videos, category):
    """Scores and hit flags of one category's predictions over all videos, in the reference's collection order (videos
    in `prediction` order, tracks in input order), then sorted by descending score (stable)."""
    scores, hits = [], []
    for v in videos:
        pos = v["by_cat"].get(category)
        if pos:
            idx = np.sort(v["order"][np.asarray(pos, dtype=np.int64)])
            hit_in = np.zeros(len(v["preds"]), dtype=bool)
            hit_in[v["order"]] = v["hit"]
            scores.append(v["scores"][idx])
            hits.append(hit_in[idx])
    scores, hits = np.concatenate(scores), np.concatenate(hits)
    srt = np.argsort(-scores, kind="stable")
    return scores[srt], hits[srt]


def _group_tables(videos):
    """The group tables both layouts share (include/tspn_mi355x.h): the packed instances as (video, kind, input index,
    instance), predictions first (grouped, score order inside a group), then ground truths; groups [G, 5], pred_group
    [P], and per packed prediction (video slot, position in score order), per packed ground truth its video index."""
    preds, gts, groups, pred_group, pred_slot, pred_pos, gt_index = [], [], [], [], [], [], []
    n_pred = sum(len(p) for v in videos for _, p, _ in v["groups"])
    gt_base, cand = n_pred, 0
    for s, v in enumerate(videos):
        for _, p, g in v["groups"]:
            groups.append((len(preds), len(p), gt_base, len(g), cand))
            pred_group.extend([len(groups) - 1] * len(p))
            cand += len(p) * len(g)
            gt_base += len(g)
            for i in v["order"][p].tolist():
                preds.append((v["vid"], "prediction", i, v["preds"][i]))
            pred_slot.extend([s] * len(p))
            pred_pos.extend(p.tolist())
            for k in g.tolist():
                gts.append((v["vid"], "ground truth", k, v["gt"][k]))
            gt_index.extend(g.tolist())
    return preds + gts, {"groups": np.array(groups, dtype=np.int64).reshape(-1, 5),
                         "pred_group": np.array(pred_group, dtype=np.int32), "n_pred": n_pred, "n_gt": len(gts),
                         "candidates": cand, "pred_slot": np.array(pred_slot, dtype=np.int64),
                         "pred_pos": np.array(pred_pos, dtype=np.int64), "gt_index": np.array(gt_index, dtype=np.int64)}


def _scatter(run, pk, hit, match, extra=None):
    """Per-chunk results (packed prediction order) back to each video's score-order arrays."""
    cut = np.searchsorted(pk["pred_slot"], np.arange(len(run) + 1))   # packed predictions are in video order
    for s, v in enumerate(run):
        sel = slice(cut[s], cut[s + 1])
        v["hit"][pk["pred_pos"][sel]] = hit[sel]
        v["match"][pk["pred_pos"][sel]] = match[sel]
        if extra is not None:
            v["tiou"][pk["pred_pos"][sel]] = extra[sel]


def _finish_stats(stats, t0, th, pack_ms, n_cand, n_chunks):
    if stats is not None:
        stats["pack_ms"] = pack_ms
        stats["host_ms"] = (time.perf_counter() - th) * 1e3
        stats["total_ms"] = (time.perf_counter() - t0) * 1e3
        stats["candidates"] = n_cand
        stats["chunks"] = n_chunks


# ---------------------------------------------------------------------------------------------------- objects: packing
def _object_rows(track):
    t = track["trajectory"]
    return len(t) if isinstance(t, dict) else len(t[0])


def _object_chunk_bytes(rows, n_pred, n_gt, n_groups, cand):
    """Host / device bytes of a packed object chunk: boxes + frames (36 per row), traj (16 per trajectory), groups (40
    each), pred_group + best + best_index + flags + hit (21 per prediction), claim (4 per ground truth).  The tiou matrix
    is not stored."""
    return 36 * rows + 16 * (n_pred + n_gt) + 40 * n_groups + 21 * n_pred + 4 * n_gt


def _object_traj(vid, kind, idx, t):
    """One object trajectory as (frames int32 [n] ascending, boxes float64 [n, 4]): a {frame key: box} dict (keys
    through int()) or a (frames, boxes) pair of arrays."""
    who = f"evaluate_objects: video {vid!r}, {kind} {idx}"
    try:
        if isinstance(t, dict):
            frames = np.fromiter((int(k) for k in t), dtype=np.int64, count=len(t))
            boxes = _as_boxes(list(t.values()))
        else:
            f, boxes = t
            frames = np.asarray(f)
            if frames.dtype.kind not in "iu" or frames.ndim != 1:
                raise ValueError(f"frames must be a 1-d integer array, got {frames.dtype} {frames.shape}")
            if frames.dtype == np.uint64 and frames.size and int(frames.max()) > _INT32.max:
                raise OverflowError
            frames = frames.astype(np.int64)
            boxes = np.asarray(boxes, dtype=np.float64)
    except OverflowError:
        raise ValueError(f"{who}: a frame id lies outside int32") from None
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{who}: trajectory must be a {{frame: 4-coordinate box}} dict or a (frames, boxes [n, 4]) "
                         f"pair ({exc})") from None
    n = frames.shape[0]
    if boxes.size == 0:
        boxes = boxes.reshape(0, 4)
    if boxes.ndim != 2 or boxes.shape != (n, 4):
        raise ValueError(f"{who}: trajectory must have one 4-coordinate box per frame (got boxes of shape {boxes.shape} "
                         f"for {n} frames)")
    if n:
        if frames.min() < _INT32.min or frames.max() > _INT32.max:
            raise ValueError(f"{who}: a frame id lies outside int32")
        step = np.diff(frames)
        if (step <= 0).any():
            srt = np.argsort(frames, kind="stable")
            frames, boxes = frames[srt], boxes[srt]
            same = np.flatnonzero(np.diff(frames) == 0)
            if same.size:
                raise ValueError(f"{who}: two keys of its trajectory are the same frame {int(frames[same[0]])}")
        if not np.isfinite(boxes).all():
            raise ValueError(f"{who}: non-finite box in its trajectory")
    return frames.astype(np.int32), boxes


def _pack_objects(videos):
    """Flat arrays of one chunk (layout: include/tspn_mi355x.h, tspn_evalobj_*): predictions first (grouped, score order
    inside a group), then ground truths.  Also, per packed prediction, (video slot, position in score order) and the
    video ground-truth index of each packed ground truth."""
    items, tables = _group_tables(videos)
    frames, boxes, traj, rows = [], [], [], 0
    for vid, kind, idx, inst in items:
        f, b = _object_traj(vid, kind, idx, inst["trajectory"])
        frames.append(f)
        boxes.append(b)
        traj.append((rows, f.shape[0]))
        rows += f.shape[0]
    # a chunk whose trajectories are all empty still hands the kernels a valid (never read) row
    return {"boxes": np.concatenate(boxes) if rows else np.zeros((1, 4)),
            "frames": np.concatenate(frames) if rows else np.zeros(1, dtype=np.int32),
            "traj": np.array(traj, dtype=np.int64).reshape(-1, 2), "rows": rows, **tables}


def _packed_object_bytes(pk):
    return _object_chunk_bytes(pk["rows"], pk["n_pred"], pk["n_gt"], pk["groups"].shape[0], pk["candidates"])


def _match_object_chunk(pk, thresh_t, dev, stats):
    """Launch the kernels over one packed chunk; one device -> host copy of best / best_index / flags / hit."""
    P = pk["n_pred"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.device(dev):
        ev[0].record()
        t = {k: torch.from_numpy(pk[k]).to(dev) for k in ("boxes", "frames", "traj", "groups", "pred_group")}
        out = torch.empty(17 * P, dtype=torch.uint8, device=dev)   # best float64 | best_index int32 | flags int32 | hit int8
        best, bidx = out[:8 * P].view(torch.float64), out[8 * P:12 * P].view(torch.int32)
        flags, hit = out[12 * P:16 * P].view(torch.int32), out[16 * P:].view(torch.int8)
        ev[1].record()
        ops.evalobj_tiou(t["boxes"], t["frames"], t["traj"], t["groups"], t["pred_group"], best=best, best_index=bidx,
                         flags=flags)
        ops.evalobj_claim(best, bidx, t["groups"], t["pred_group"], pk["n_gt"], thresh_t, hit=hit)
        ev[2].record()
        host = out.cpu().numpy()
        ev[3].record()
        ev[3].synchronize()
    if stats is not None:
        stats["device_ms"] = stats.get("device_ms", 0.0) + ev[0].elapsed_time(ev[3])
        stats["kernel_ms"] = stats.get("kernel_ms", 0.0) + ev[1].elapsed_time(ev[2])
    return (host[:8 * P].view(np.float64).copy(), host[8 * P:12 * P].view(np.int32).astype(np.int64),
            host[12 * P:16 * P].view(np.int32), host[16 * P:].view(np.int8).astype(bool))


# ---------------------------------------------------------------------------------------------------- objects: public
def evaluate_objects(groundtruth, prediction, use_07_metric=True, thresh_t=0.5, device=None, max_candidates=None,
                     max_bytes=None, details=False, stats=None):
    """Trajectory mAP of `prediction` ({vid: [{category, score, trajectory}]}) against `groundtruth` ({vid: [{category,
    trajectory}]}) as the reference's `evaluate` (lib/evaluation/video_object_detection.py:46-129) returns it:
    (mean_ap, ap_class), ap_class the list of (category, ap) sorted by category, same values and types.  A trajectory is
    a {frame key: (x1, y1, x2, y2)} dict (keys through int(), any frame set) or a (frames int array, boxes float64 [n, 4])
    pair, which skips the conversion.
    device, max_candidates, max_bytes, stats: as for `evaluation.evaluate` (chunks of whole videos).
    details: also return {vid: {"hit", "match", "tiou", "order"}} for every predicted video: hit flags, the video's
    ground-truth index of the best-overlapping ground truth (max_index; -1 where the video has no ground truth of the
    category) and that overlap (max_overlap) of the predictions in score order, and that order (input indices)."""
    who = "evaluate_objects"
    t0 = time.perf_counter()
    max_candidates, max_bytes = _budgets(who, max_candidates, max_bytes)
    if not thresh_t > 0:
        raise ValueError(f"{who}: thresh_t must be > 0, got {thresh_t!r} (at 0 every prediction would claim ground "
                         "truth 0, which need not exist)")
    dev = None if device is None else _resolve_device(device)
    gt_classes, gt_by_class = _gt_classes(groundtruth)
    videos = _prepare(who, groundtruth, prediction, gt_classes, gt_by_class, True, _object_rows, _object_chunk_bytes)
    for v in videos:
        v["tiou"] = np.zeros(len(v["preds"]), dtype=np.float64)
    pack_ms, n_chunks, n_cand = 0.0, 0, 0
    for run in _chunks(videos, max_candidates, max_bytes):
        tp = time.perf_counter()
        pk = _pack_objects(run)
        pack_ms += (time.perf_counter() - tp) * 1e3
        if pk["n_pred"] == 0:
            continue
        if dev is None:
            dev = _resolve_device(device)
        best, bidx, flags, hit = _match_object_chunk(pk, float(thresh_t), dev, stats)
        if flags.any():
            p = int(np.flatnonzero(flags)[0])
            v = run[pk["pred_slot"][p]]
            what = "zero sIoU denominator on a common frame with" if flags[p] & 1 else "no frame in it nor in"
            raise ZeroDivisionError(f"{who}: video {v['vid']!r}, prediction {int(v['order'][pk['pred_pos'][p]])}: "
                                    f"{what} a ground truth of its category")
        gt_base = pk["groups"][pk["pred_group"], 2] - pk["n_pred"]   # first packed ground truth of each prediction's group
        _scatter(run, pk, hit, pk["gt_index"][gt_base + bidx], best)
        n_chunks += 1
        n_cand += pk["candidates"]
    th = time.perf_counter()
    npos = {}
    for by in gt_by_class.values():
        for c, ks in by.items():
            npos[c] = npos.get(c, 0) + len(ks)
    predicted = set(t["category"] for tracks in prediction.values() for t in tracks)
    ap_class = {}
    for c in gt_classes:
        if c not in predicted:
            ap_class[c] = 0.
            continue
        _, hit = _class_columns(videos, c)
        tp = np.cumsum(hit.astype(np.float64))
        fp = np.cumsum((~hit).astype(np.float64))
        rec = tp / float(npos[c])
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap_class[c] = voc_ap(rec, prec, use_07_metric)
    ap_class = sorted(ap_class.items(), key=lambda kv: kv[0])
    total_ap = 0.
    for _, ap in ap_class:
        total_ap += ap
    mean_ap = total_ap / len(gt_classes)
    _finish_stats(stats, t0, th, pack_ms, n_cand, n_chunks)
    if not details:
        return mean_ap, ap_class
    info = {v["vid"]: {"hit": v["hit"], "match": v["match"], "tiou": v["tiou"], "order": v["order"]} for v in videos}
    return mean_ap, ap_class, info


# ---------------------------------------------------------------------------------------------------- actions
def _action_rows(inst):
    return max(int(inst["duration"][1]) - int(inst["duration"][0]), 0)


def _action_traj(vid, kind, idx, inst):
    """One action trajectory as float64 [n, 4], its length checked against the duration (as evaluation._traj_array)."""
    who = f"evaluate_actions: video {vid!r}, {kind} {idx}"
    b, e = int(inst["duration"][0]), int(inst["duration"][1])
    try:
        a = _as_boxes(inst["trajectory"])
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{who}: trajectory must be a list of 4-coordinate boxes ({exc})") from None
    if a.size == 0:
        a = a.reshape(0, 4)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"{who}: trajectory must be a list of 4-coordinate boxes (got shape {a.shape})")
    if a.shape[0] != e - b:
        raise ValueError(f"{who}: trajectory has {a.shape[0]} boxes for the duration [{b}, {e}) of {e - b} frames")
    if not np.isfinite(a).all():
        raise ValueError(f"{who}: non-finite box in its trajectory")
    return a, b, e


def _pack_actions(videos):
    """Flat arrays of one chunk in the relation evaluator's layout (include/tspn_mi355x.h, tspn_eval_*): instance r is
    "relation" r, whose subject row 2r and object row 2r + 1 of `traj` are equal, so its boxes are stored once."""
    items, tables = _group_tables(videos)
    arrays, traj, rows = [], [], 0
    for it in items:
        a, b, e = _action_traj(*it)
        arrays.append(a)
        traj.extend([(rows, b, e)] * 2)
        rows += a.shape[0]
    return {"boxes": np.concatenate(arrays) if rows else np.zeros((1, 4)),
            "traj": np.array(traj, dtype=np.int64).reshape(-1, 3), "rows": rows,
            "max_group_gt": int(tables["groups"][:, 3].max(initial=0)), **tables}


def evaluate_actions(groundtruth, prediction, viou_threshold=0.5, device=None, max_candidates=None, max_bytes=None,
                     details=False, stats=None):
    """Per-predicate mAP of `prediction` ({vid: [{category, score, duration, trajectory}]}) against `groundtruth`
    ({vid: [{category, duration, trajectory}]}, e.g. from `action_instances`) as the reference's `evaluate`
    (lib/evaluation/action_detection.py:33-97) returns it: (mean_ap, ap_class) with mean_ap an np.float64 and ap_class
    the {category: ap} dict, in the iteration order of the reference's set of ground-truth categories.  A duration is
    [begin, end) and a trajectory its end - begin boxes (a list of (x1, y1, x2, y2) or a float64 [n, 4] array).
    device, max_candidates, max_bytes, stats: as for `evaluation.evaluate` (a chunk's bytes count each instance's boxes
    once).  details: also return {"videos": {vid: {"hit", "match", "order"}}, "classes": {category: (prec, rec,
    hit_scores)}}: per predicted video what `evaluation.evaluate` gives (match: the video's ground-truth index, -1 for
    none), and per predicted ground-truth category the reference's compute_detection_scores_per_class outputs."""
    who = "evaluate_actions"
    t0 = time.perf_counter()
    max_candidates, max_bytes = _budgets(who, max_candidates, max_bytes)
    dev = None if device is None else _resolve_device(device)
    gt_classes, gt_by_class = _gt_classes(groundtruth)
    videos = _prepare(who, groundtruth, prediction, gt_classes, gt_by_class, False, _action_rows, _chunk_bytes)
    pack_ms, n_chunks, n_cand = 0.0, 0, 0
    for run in _chunks(videos, max_candidates, max_bytes):
        tp = time.perf_counter()
        pk = _pack_actions(run)
        pack_ms += (time.perf_counter() - tp) * 1e3
        if pk["n_pred"] == 0:
            continue
        if dev is None:
            dev = _resolve_device(device)
        hit, match, zden = _match_chunk(pk, viou_threshold, dev, stats)
        if zden.any():
            p = int(np.flatnonzero(zden)[0])
            v = run[pk["pred_slot"][p]]
            raise ZeroDivisionError(f"{who}: video {v['vid']!r}, prediction {int(v['order'][pk['pred_pos'][p]])}: "
                                    "zero vIoU denominator against a ground truth of its category")
        gt_base = pk["groups"][pk["pred_group"], 2] - pk["n_pred"]
        _scatter(run, pk, hit, np.where(match >= 0, pk["gt_index"][gt_base + np.maximum(match, 0)], -1))
        n_chunks += 1
        n_cand += pk["candidates"]
    th = time.perf_counter()
    n_gt = {}
    for by in gt_by_class.values():
        for c, ks in by.items():
            n_gt[c] = n_gt.get(c, 0) + len(ks)
    predicted = set(t["category"] for tracks in prediction.values() for t in tracks)
    ap_class, curves = {}, {}
    for c in gt_classes:
        if c not in predicted:
            ap_class[c] = 0.
            continue
        scores, hit = _class_columns(videos, c)
        prec, rec, hit_scores = _detection_scores(n_gt[c], scores, hit)
        curves[c] = (prec, rec, hit_scores)
        ap_class[c] = voc_ap(rec, prec)
    mean_ap = np.mean(list(ap_class.values()))
    _finish_stats(stats, t0, th, pack_ms, n_cand, n_chunks)
    if not details:
        return mean_ap, ap_class
    info = {v["vid"]: {"hit": v["hit"], "match": v["match"], "order": v["order"]} for v in videos}
    return mean_ap, ap_class, {"videos": info, "classes": curves}
