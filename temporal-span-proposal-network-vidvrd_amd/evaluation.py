"""Video relation detection evaluation on the GPU: mAP, Recall@K and tagging Precision@K.

Same arguments, return values (numpy dtypes included) and numbers as the reference's
`lib.evaluation.visual_relation_detection.evaluate` (visual_relation_detection.py:8-103, common.py:4-106) and the
relation part of its `evaluate.py` (`evaluate_zeroshot`, evaluate.py:24-55); it prints nothing.

What runs where:
  * host: validation, the score order (`np.argsort(-score, kind="stable")` = the reference's stable
    `sorted(key=score, reverse=True)`), grouping by (video, triplet), packing, and the per-video metrics in numpy with
    the reference's dtypes (float32 cumsums, non-07 VOC AP, Recall@N, tagging Precision@N);
  * device (csrc/eval/tspn_eval.hip): every trajectory's volume, the vIoU of every (prediction, same-triplet ground
    truth) pair in float64 in the reference's summation order, and the greedy match of each group.  A ground truth is
    only ever detected by a prediction of its own triplet, so the (video, triplet) groups are independent.

Deliberate additions to the reference's behaviour:
  * a non-finite score, or a non-finite box in a trajectory that takes part in a vIoU, raises ValueError naming the
    video and the relation (under the reference a +inf score would count as a hit whatever the match);
  * such a trajectory whose length is not `end - begin` raises ValueError (the reference would index past it or
    silently use a prefix);
  * a zero vIoU denominator on any same-triplet pair with overlapping durations raises ZeroDivisionError (the
    reference raises it only for the pairs its loop reaches).
Where the reference raises, the same exception type is raised: a ground-truth video missing from the predictions
raises KeyError, and no prediction in any video with ground truth raises IndexError (the reference's `rec[-1]`).

The reference's two other evaluators, video object detection and action detection, live in evaluation_detection.py and
are re-exported here (`evaluate_objects`, `evaluate_actions`, `object_instances`, `action_instances`).
"""
import itertools
import json
import time
from collections import defaultdict

import numpy as np
import torch

from . import ops

__all__ = ["evaluate", "evaluate_zeroshot", "relation_instances", "triplets", "load_prediction", "voc_ap",
           "DEFAULT_MAX_CANDIDATES", "DEFAULT_MAX_BYTES"]

# A launch set (chunk) is a run of whole videos within both budgets; a single video that exceeds one goes alone.
DEFAULT_MAX_CANDIDATES = 1 << 24   # (prediction, ground truth) pairs: the float64 ov matrix, 128 MiB at most
DEFAULT_MAX_BYTES = 1 << 30        # everything a chunk packs and allocates on the device (_packed_bytes), boxes included
_REG_MASK_MAX_GT = 4096            # tspn_eval_greedy_match_f64 keeps larger groups' detected flags in det_ws


# ---------------------------------------------------------------------------------------------------- annotations
def relation_instances(annotation, no_traj=False):
    """The ground-truth relation list of one VidVRD / VidOR annotation dict, as the reference's
    `Dataset.get_relation_insts` builds it (lib/dataset/dataset.py:173-208): triplet (subject category, predicate,
    object category), subject_tid, object_tid, duration (begin_fid, end_fid) and, unless `no_traj`, the subject and
    object trajectories as lists of (xmin, ymin, xmax, ymax) tuples."""
    sub_objs = {so["tid"]: so["category"] for so in annotation["subject/objects"]}
    if not no_traj:
        trajs = []
        for frame in annotation["trajectories"]:
            trajs.append({b["tid"]: (b["bbox"]["xmin"], b["bbox"]["ymin"], b["bbox"]["xmax"], b["bbox"]["ymax"])
                          for b in frame})
    insts = []
    for a in annotation["relation_instances"]:
        inst = {"triplet": (sub_objs[a["subject_tid"]], a["predicate"], sub_objs[a["object_tid"]]),
                "subject_tid": a["subject_tid"], "object_tid": a["object_tid"],
                "duration": (a["begin_fid"], a["end_fid"])}
        if not no_traj:
            frames = trajs[inst["duration"][0]:inst["duration"][1]]
            inst["sub_traj"] = [bb[a["subject_tid"]] for bb in frames]
            inst["obj_traj"] = [bb[a["object_tid"]] for bb in frames]
        insts.append(inst)
    return insts


def triplets(annotations):
    """The set of relation triplets of annotation dicts (an iterable of them, or a dict of them keyed by video id),
    like the reference's `Dataset.get_triplets(split)` (lib/dataset/dataset.py:92-97)."""
    if isinstance(annotations, dict):
        annotations = annotations.values()
    out = set()
    for anno in annotations:
        out.update(inst["triplet"] for inst in relation_instances(anno, no_traj=True))
    return out


def load_prediction(path):
    """The `results` dict (video id -> relation list) of a prediction JSON file `{"version": ..., "results": ...}`."""
    with open(path, "r") as fh:
        pred = json.load(fh)
    return pred["results"]


# ---------------------------------------------------------------------------------------------------- host metrics
def voc_ap(rec, prec, use_07_metric=False):
    """VOC AP of the reference (lib/evaluation/common.py:4-37).  Non-07 (the default): the precision envelope is a
    reversed running maximum, which np.maximum.accumulate computes exactly.  `use_07_metric`: the 11-point form, the
    largest precision at a recall >= t (0 where there is none) over np.arange(0., 1.1, 0.1), each divided by 11. and added
    in that order to a Python 0. (so a curve that never reaches recall 0 gives a Python float, any other an np.float64)."""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            reached = rec >= t
            ap = ap + (np.max(prec[reached]) if np.sum(reached) != 0 else 0) / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _detection_scores(n_gt, sorted_scores, hit):
    """eval_detection_scores' tail (visual_relation_detection.py:27-35) from the hit flags in score order."""
    hit_scores = np.ones((len(sorted_scores))) * -np.inf
    hit_scores[hit] = sorted_scores[hit]
    tp = np.isfinite(hit_scores)
    fp = ~tp
    cum_tp = np.cumsum(tp).astype(np.float32)
    cum_fp = np.cumsum(fp).astype(np.float32)
    rec = cum_tp / np.maximum(n_gt, np.finfo(np.float32).eps)
    prec = cum_tp / np.maximum(cum_tp + cum_fp, np.finfo(np.float32).eps)
    return prec, rec, hit_scores


def _tagging_prec(gt_keys, sorted_pred_keys):
    """eval_tagging_scores' precision (visual_relation_detection.py:38-61): triplets deduplicated in score order."""
    gt_set = set(gt_keys)
    tp = np.array([k in gt_set for k in dict.fromkeys(sorted_pred_keys)], dtype=bool)
    fp = ~tp
    cum_tp = np.cumsum(tp).astype(np.float32)
    cum_fp = np.cumsum(fp).astype(np.float32)
    return cum_tp / np.maximum(cum_tp + cum_fp, np.finfo(np.float32).eps)


def _aggregate(videos, det_nreturns, tag_nreturns):
    """The reference's `evaluate` loop and aggregates (visual_relation_detection.py:64-103) over the videos with
    ground truth, in ground-truth order.  `videos`: list of dicts with vid, n_gt, scores (float64, score order),
    hit (bool, score order), gt_keys and pred_keys (triplet ids, pred_keys in score order).
    Returns (mean_ap, rec_at_n, mprec_at_n, per-video {vid: (ap, prec, rec, hit_scores)})."""
    video_ap = dict()
    per_video = dict()
    tot_scores = defaultdict(list)
    tot_tp = defaultdict(list)
    prec_at_n = defaultdict(list)
    tot_gt_relations = 0
    for v in videos:
        tot_gt_relations += v["n_gt"]
        det_prec, det_rec, det_scores = _detection_scores(v["n_gt"], v["scores"], v["hit"])
        video_ap[v["vid"]] = voc_ap(det_rec, det_prec)
        per_video[v["vid"]] = (video_ap[v["vid"]], det_prec, det_rec, det_scores)
        tp = np.isfinite(det_scores)
        for nre in det_nreturns:
            cut_off = min(nre, det_scores.size)
            tot_scores[nre].append(det_scores[:cut_off])
            tot_tp[nre].append(tp[:cut_off])
        tag_prec = _tagging_prec(v["gt_keys"], v["pred_keys"])
        for nre in tag_nreturns:
            cut_off = min(nre, tag_prec.size)
            if cut_off > 0:
                prec_at_n[nre].append(tag_prec[cut_off - 1])
            else:
                prec_at_n[nre].append(0.)
    mean_ap = np.mean(list(video_ap.values()))
    rec_at_n = dict()
    for nre in det_nreturns:
        scores = np.concatenate(tot_scores[nre])
        tps = np.concatenate(tot_tp[nre])
        tps = tps[np.argsort(scores)[::-1]]
        cum_tp = np.cumsum(tps).astype(np.float32)
        rec = cum_tp / np.maximum(tot_gt_relations, np.finfo(np.float32).eps)
        rec_at_n[nre] = rec[-1]
    mprec_at_n = dict()
    for nre in tag_nreturns:
        mprec_at_n[nre] = np.mean(prec_at_n[nre])
    return mean_ap, rec_at_n, mprec_at_n, per_video


# ---------------------------------------------------------------------------------------------------- packing
def _prepare(groundtruth, prediction):
    """Per video with ground truth (in ground-truth order): the score order, triplet ids (one dict per call) and the
    (triplet) groups that have both predictions and ground truths."""
    key_of = {}
    videos = []
    for vid, gt in groundtruth.items():
        if len(gt) == 0:
            continue
        preds = prediction[vid]
        scores = np.empty(len(preds), dtype=np.float64)
        pkeys = np.empty(len(preds), dtype=np.int64)
        plen = np.empty(len(preds), dtype=np.int64)
        for i, r in enumerate(preds):
            scores[i] = r["score"]
            pkeys[i] = key_of.setdefault(tuple(r["triplet"]), len(key_of))
            plen[i] = r["duration"][1] - r["duration"][0]
        bad = np.flatnonzero(~np.isfinite(scores))
        if bad.size:
            raise ValueError(f"evaluate: video {vid!r}, prediction {int(bad[0])}: non-finite score {scores[bad[0]]!r}")
        gkeys = np.array([key_of.setdefault(tuple(r["triplet"]), len(key_of)) for r in gt], dtype=np.int64)
        order = np.argsort(-scores, kind="stable")
        skeys = pkeys[order]
        # groups: stable sorts by triplet id keep score order (predictions) and index order (ground truths) inside
        pos = np.argsort(skeys, kind="stable")
        gidx = np.argsort(gkeys, kind="stable")
        pk, pstart, pcount = np.unique(skeys[pos], return_index=True, return_counts=True)
        gk, gstart, gcount = np.unique(gkeys[gidx], return_index=True, return_counts=True)
        _, pi, gi = np.intersect1d(pk, gk, assume_unique=True, return_indices=True)
        groups = [(pos[pstart[a]:pstart[a] + pcount[a]], gidx[gstart[b]:gstart[b] + gcount[b]]) for a, b in zip(pi, gi)]
        # what packing this video costs, from the durations (= the box rows of valid trajectories; _pack checks them)
        glen = np.array([r["duration"][1] - r["duration"][0] for r in gt], dtype=np.int64)
        sel_p = order[np.concatenate([p for p, _ in groups])] if groups else np.zeros(0, dtype=np.int64)
        sel_g = np.concatenate([g for _, g in groups]) if groups else np.zeros(0, dtype=np.int64)
        rows = 2 * int(np.maximum(plen[sel_p], 0).sum() + np.maximum(glen[sel_g], 0).sum())
        cand = int(sum(len(p) * len(g) for p, g in groups))
        videos.append({"vid": vid, "gt": gt, "preds": preds, "n_gt": len(gt), "scores": scores[order], "order": order,
                       "gt_keys": gkeys, "pred_keys": skeys, "groups": groups, "candidates": cand,
                       "bytes": _chunk_bytes(rows, len(sel_p), len(sel_g), len(groups), cand)})
    return videos


def _chunk_bytes(rows, n_pred, n_gt, n_groups, cand):
    """Host / device bytes of a packed chunk: boxes (32 per row), traj + volumes (32 per trajectory), ov (8 per pair),
    groups (40 each), pred_group + hit / match / zero flags (13 per prediction), det_ws (1 per relation)."""
    n_rel = n_pred + n_gt
    return 32 * rows + 64 * n_rel + 8 * cand + 40 * n_groups + 13 * n_pred + n_rel


def _packed_bytes(pk):
    """_chunk_bytes of a packed chunk, from its arrays."""
    return _chunk_bytes(pk["rows"], pk["n_pred"], pk["traj"].shape[0] // 2 - pk["n_pred"], pk["groups"].shape[0],
                        pk["candidates"])


def _as_boxes(t):
    """float64 [n, 4] view or copy of a trajectory.  The JSON form (a list of 4-coordinate lists / tuples) goes
    through one np.fromiter over the chained coordinates, about twice as fast as np.asarray on nested lists; every
    box is checked to have 4 coordinates first, so that a ragged box cannot shift the ones after it."""
    if isinstance(t, (list, tuple)) and t:
        if set(map(len, t)) != {4}:                 # (TypeError for a box without a length)
            raise ValueError(f"box lengths {sorted(set(map(len, t)))}")
        return np.fromiter(itertools.chain.from_iterable(t), dtype=np.float64, count=4 * len(t)).reshape(-1, 4)
    return np.asarray(t, dtype=np.float64)


def _traj_array(vid, kind, idx, rel, side):
    """One trajectory as float64 [n, 4] (one conversion), its length checked against the duration."""
    b, e = rel["duration"][0], rel["duration"][1]
    try:
        a = _as_boxes(rel[side])
    except (TypeError, ValueError) as exc:
        a, err = None, exc
    if a is not None and a.size == 0:
        a = a.reshape(0, 4)
    if a is None or a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"evaluate: video {vid!r}, {kind} {idx}: {side} must be a list of 4-coordinate boxes "
                         f"({err if a is None else f'got shape {a.shape}'})")
    if a.shape[0] != e - b:
        raise ValueError(f"evaluate: video {vid!r}, {kind} {idx}: {side} has {a.shape[0]} boxes for the duration "
                         f"[{b}, {e}) of {e - b} frames")
    return a, int(b), int(e)


def _pack(videos):
    """Flat arrays of one chunk (layout: include/tspn_mi355x.h, tspn_eval_*).  Only relations of groups are packed:
    predictions first (grouped, score order inside a group), then ground truths.  Also returns, per packed
    prediction, (video slot, position in score order) and the video ground-truth index of each packed ground truth."""
    pred_rels, gt_rels, groups, pred_group = [], [], [], []
    pred_slot, pred_pos, gt_index = [], [], []
    n_pred = sum(len(p) for v in videos for p, _ in v["groups"])
    cand = 0
    gt_base = n_pred
    for s, v in enumerate(videos):
        for p, g in v["groups"]:
            groups.append((len(pred_rels), len(p), gt_base, len(g), cand))
            pred_group.extend([len(groups) - 1] * len(p))
            cand += len(p) * len(g)
            gt_base += len(g)
            for k in p:
                pred_rels.append((v["vid"], "prediction", int(v["order"][k]), v["preds"][v["order"][k]]))
            pred_slot.extend([s] * len(p))
            pred_pos.extend(p.tolist())
            for k in g:
                gt_rels.append((v["vid"], "ground truth", int(k), v["gt"][k]))
            gt_index.extend(g.tolist())
    arrays, traj, rows = [], [], 0
    for vid, kind, idx, rel in pred_rels + gt_rels:
        for side in ("sub_traj", "obj_traj"):
            a, b, e = _traj_array(vid, kind, idx, rel, side)
            arrays.append(a)
            traj.append((rows, b, e))
            rows += a.shape[0]
    # a chunk whose trajectories are all empty still hands the kernels a valid (never read) row
    boxes = np.concatenate(arrays) if rows else np.zeros((1, 4))
    traj = np.array(traj, dtype=np.int64).reshape(-1, 3)
    if not np.isfinite(boxes).all():
        bad_row = int(np.flatnonzero(~np.isfinite(boxes).all(axis=1))[0])
        t = int(np.searchsorted(traj[:, 0], bad_row, side="right")) - 1   # (an empty one shares the next one's row)
        vid, kind, idx, _ = (pred_rels + gt_rels)[t // 2]
        raise ValueError(f"evaluate: video {vid!r}, {kind} {idx}: non-finite box in its "
                         f"{('sub_traj', 'obj_traj')[t % 2]}")
    return {"boxes": boxes, "traj": traj, "groups": np.array(groups, dtype=np.int64).reshape(-1, 5),
            "pred_group": np.array(pred_group, dtype=np.int32), "n_pred": n_pred, "candidates": cand, "rows": rows,
            "max_group_gt": max((gr[3] for gr in groups), default=0),
            "pred_slot": np.array(pred_slot, dtype=np.int64), "pred_pos": np.array(pred_pos, dtype=np.int64),
            "gt_index": np.array(gt_index, dtype=np.int64)}


def _chunks(videos, max_candidates, max_bytes=DEFAULT_MAX_BYTES):
    """Consecutive runs of videos whose candidate pairs stay within max_candidates and whose packed bytes stay within
    max_bytes (a video that exceeds either alone goes alone)."""
    run, cand, nbytes = [], 0, 0
    for v in videos:
        if run and (cand + v["candidates"] > max_candidates or nbytes + v["bytes"] > max_bytes):
            yield run
            run, cand, nbytes = [], 0, 0
        run.append(v)
        cand += v["candidates"]
        nbytes += v["bytes"]
    if run:
        yield run


def _resolve_device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"evaluate: the vIoU / matching kernels need a HIP device, got {device!r} "
                           "(there is no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _match_chunk(pk, viou_threshold, dev, stats):
    """Launch the three kernels over one packed chunk; one device -> host copy of hit / match / zero flags."""
    P = pk["n_pred"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.device(dev):
        ev[0].record()
        boxes = torch.from_numpy(pk["boxes"]).to(dev)
        traj = torch.from_numpy(pk["traj"]).to(dev)
        groups = torch.from_numpy(pk["groups"]).to(dev)
        pred_group = torch.from_numpy(pk["pred_group"]).to(dev)
        out = torch.empty(9 * P, dtype=torch.uint8, device=dev)   # match int32 | zden int32 | hit int8
        match, zden, hit = out[:4 * P].view(torch.int32), out[4 * P:8 * P].view(torch.int32), out[8 * P:].view(torch.int8)
        det_ws = None
        if pk["max_group_gt"] > _REG_MASK_MAX_GT:
            det_ws = torch.zeros(pk["traj"].shape[0] // 2, dtype=torch.uint8, device=dev)
        ev[1].record()
        vol = ops.eval_traj_volume(boxes, traj)
        ov, _ = ops.eval_viou(boxes, traj, vol, groups, pred_group, pk["candidates"], zden=zden)
        ops.eval_greedy_match(ov, groups, P, viou_threshold, pk["max_group_gt"], det_ws=det_ws, hit=hit, match=match)
        ev[2].record()
        host = out.cpu().numpy()
        ev[3].record()
        ev[3].synchronize()
    if stats is not None:
        stats["device_ms"] = stats.get("device_ms", 0.0) + ev[0].elapsed_time(ev[3])
        stats["kernel_ms"] = stats.get("kernel_ms", 0.0) + ev[1].elapsed_time(ev[2])
    return (host[8 * P:].view(np.int8).astype(bool), host[:4 * P].view(np.int32).astype(np.int64),
            host[4 * P:8 * P].view(np.int32))


# ---------------------------------------------------------------------------------------------------- public
def evaluate(groundtruth, prediction, viou_threshold=0.5, det_nreturns=(50, 100, 1000), tag_nreturns=(1, 5, 10),
             device=None, max_candidates=None, details=False, stats=None, max_bytes=None):
    """Relation detection mAP, Recall@N and tagging Precision@N of `prediction` (video id -> relation list) against
    `groundtruth` (video id -> ground-truth relation list, e.g. from `relation_instances`), as the reference's
    `evaluate` (lib/evaluation/visual_relation_detection.py:64-103) returns them: (mean_ap, rec_at_n, mprec_at_n),
    same values and numpy dtypes.  A relation is a dict with triplet, duration [begin, end), sub_traj and obj_traj
    (lists of (x1, y1, x2, y2) or float64 [n, 4] arrays) and, for a prediction, score.
    device: the HIP device of the vIoU / matching kernels (default: the current one).
    max_candidates, max_bytes: budgets of one launch set (chunk) of whole videos: (prediction, same-triplet ground
    truth) pairs (default DEFAULT_MAX_CANDIDATES) and bytes packed on the host and allocated on the device, boxes
    included (default DEFAULT_MAX_BYTES = 1 GiB); a single video over a budget forms a chunk of its own.  details: also return {vid: {"ap", "hit", "match", "order"}}: hit flags and matched
    ground-truth index (-1: none) of the predictions in score order, and that order (input indices).
    stats: optional dict, receives pack_ms, device_ms (uploads + kernels + download, events), kernel_ms,
    host_ms, candidates, chunks."""
    t0 = time.perf_counter()
    max_candidates = DEFAULT_MAX_CANDIDATES if max_candidates is None else int(max_candidates)
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    if max_candidates < 1 or max_bytes < 1:
        raise ValueError("evaluate: max_candidates and max_bytes must be positive")
    dev = None if device is None else _resolve_device(device)
    videos = _prepare(groundtruth, prediction)
    for v in videos:
        v["hit"] = np.zeros(len(v["preds"]), dtype=bool)
        v["match"] = np.full(len(v["preds"]), -1, dtype=np.int64)
    pack_ms = 0.0
    n_chunks = n_cand = 0
    for run in _chunks(videos, max_candidates, max_bytes):
        tp = time.perf_counter()
        pk = _pack(run)
        pack_ms += (time.perf_counter() - tp) * 1e3
        if pk["n_pred"] == 0:
            continue
        if dev is None:
            dev = _resolve_device(device)
        hit, match, zden = _match_chunk(pk, viou_threshold, dev, stats)
        if zden.any():
            p = int(np.flatnonzero(zden)[0])
            v = run[pk["pred_slot"][p]]
            raise ZeroDivisionError(f"evaluate: video {v['vid']!r}, prediction {int(v['order'][pk['pred_pos'][p]])}: "
                                    "zero vIoU denominator against a ground truth of its triplet")
        gt_base = pk["groups"][pk["pred_group"], 2] - pk["n_pred"]   # first packed ground truth of each prediction's group
        vmatch = np.where(match >= 0, pk["gt_index"][gt_base + np.maximum(match, 0)], -1)
        cut = np.searchsorted(pk["pred_slot"], np.arange(len(run) + 1))   # packed predictions are in video order
        for s, v in enumerate(run):
            sel = slice(cut[s], cut[s + 1])
            v["hit"][pk["pred_pos"][sel]] = hit[sel]
            v["match"][pk["pred_pos"][sel]] = vmatch[sel]
        n_chunks += 1
        n_cand += pk["candidates"]
    th = time.perf_counter()
    mean_ap, rec_at_n, mprec_at_n, per_video = _aggregate(videos, det_nreturns, tag_nreturns)
    if stats is not None:
        stats["pack_ms"] = pack_ms
        stats["host_ms"] = (time.perf_counter() - th) * 1e3
        stats["total_ms"] = (time.perf_counter() - t0) * 1e3
        stats["candidates"] = n_cand
        stats["chunks"] = n_chunks
    if not details:
        return mean_ap, rec_at_n, mprec_at_n
    info = {v["vid"]: {"ap": per_video[v["vid"]][0], "hit": v["hit"], "match": v["match"], "order": v["order"]}
            for v in videos}
    return mean_ap, rec_at_n, mprec_at_n, info


def evaluate_zeroshot(groundtruth, prediction, train_triplets, old=False, **kwargs):
    """The zero-shot setting of the reference's evaluate_relation (evaluate.py:24-55): only ground truths whose
    triplet appears in `groundtruth` but not in `train_triplets`, only videos that have one; the predictions are
    filtered to those triplets too unless `old` (the old setting keeps every prediction of such a video).
    Keyword arguments go to `evaluate`."""
    split = set(tuple(r["triplet"]) for rels in groundtruth.values() for r in rels)
    zeroshot = split.difference(set(tuple(t) for t in train_triplets))
    gt, pred = dict(), dict()
    for vid, rels in groundtruth.items():
        zs = [r for r in rels if tuple(r["triplet"]) in zeroshot]
        if len(zs) > 0:
            gt[vid] = zs
            pred[vid] = prediction[vid] if old else [r for r in prediction[vid] if tuple(r["triplet"]) in zeroshot]
    return evaluate(gt, pred, **kwargs)


# object and action detection (evaluation_detection.py builds on the helpers above, hence the late import)
from .evaluation_detection import action_instances, evaluate_actions, evaluate_objects, object_instances  # noqa: E402

__all__ += ["evaluate_objects", "evaluate_actions", "object_instances", "action_instances"]
