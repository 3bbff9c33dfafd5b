"""Pure-Python restatement of the reference's object and action detection evaluation, statement by
statement in its order, written from that description: Python numbers for every overlap, numpy only where the reference
uses numpy (the score sort, the cumulative sums, the AP).  tests/test_evaluation_detection_host.py holds it equal to
golden g13, which the reference's own modules produced, so the GPU tests may compare against it on any input.

The one deliberate difference: the object evaluator's score order is `np.argsort(-scores, kind="stable")` (the reference's
default sort is unspecified on ties) and frame keys are compared as int(key)."""
import numpy as np

THRESH_S = (0.5, 0.7, 0.9)


# ---------------------------------------------------------------------------------------------------- AP
def voc_ap(rec, prec, use_07_metric=False):
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            if np.sum(rec >= t) == 0:
                p = 0
            else:
                p = np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


# ---------------------------------------------------------------------------------------------------- objects
def siou(g, p):
    """Spatial IoU of a ground-truth box and a predicted box: + 1 widths, max(0, .) on the overlap sides."""
    area_g = (g[2] - g[0] + 1) * (g[3] - g[1] + 1)
    area_p = (p[2] - p[0] + 1) * (p[3] - p[1] + 1)
    ov_w = max(0, min(g[2], p[2]) - max(g[0], p[0]) + 1)
    ov_h = max(0, min(g[3], p[3]) - max(g[1], p[1]) + 1)
    ov = ov_w * ov_h
    return ov * 1.0 / (area_g + area_p - ov)


def int_keys(traj):
    """{int(key): box}; a (frames, boxes) pair becomes the same."""
    if isinstance(traj, dict):
        return {int(k): b for k, b in traj.items()}
    frames, boxes = traj
    return {int(f): tuple(b.tolist()) for f, b in zip(frames, boxes)}


def tiou(gt_traj, pred_traj):
    """tIoU of two {frame: box} dicts: the three threshold counters over the common frames / (3 * |union|)."""
    total = len(set(gt_traj.keys()) | set(pred_traj.keys()))
    top = [0, 0, 0]
    for fid in gt_traj:
        if fid not in pred_traj:
            continue
        s = siou(gt_traj[fid], pred_traj[fid])
        for k, thr in enumerate(THRESH_S):
            if s >= thr:
                top[k] += 1
    return (top[0] + top[1] + top[2]) * 1.0 / (3 * total)


def trajectory_overlap(gt_trajs, pred_traj):
    """(max_overlap, max_index) over all ground truths, from (0, 0), strict `>`."""
    max_overlap, max_index = 0, 0
    for t, gt_traj in enumerate(gt_trajs):
        v = tiou(gt_traj, pred_traj)
        if v > max_overlap:
            max_overlap, max_index = v, t
    return max_overlap, max_index


def evaluate_objects(gt, pred, use_07_metric=True, thresh_t=0.5):
    """(mean_ap, ap_class list, per_pred) with per_pred = {(vid, input index): (max_overlap, max_index within the
    video's ground truths of the category, is true positive)} for every prediction of a ground-truth category."""
    gt_classes = set(trk["category"] for tracks in gt.values() for trk in tracks)
    by_class = {}
    for vid, tracks in pred.items():
        for i, trk in enumerate(tracks):
            by_class.setdefault(trk["category"], []).append((vid, i, trk["score"], int_keys(trk["trajectory"])))
    ap_class, per_pred = {}, {}
    for c in gt_classes:
        if c not in by_class:
            ap_class[c] = 0.
            continue
        recs, npos = {}, 0
        for vid in gt:
            trajs = [int_keys(trk["trajectory"]) for trk in gt[vid] if trk["category"] == c]
            recs[vid] = (trajs, [False] * len(trajs))
            npos += len(trajs)
        dets = by_class[c]
        nd = len(dets)
        tp, fp = np.zeros(nd), np.zeros(nd)
        order = np.argsort(-np.array([d[2] for d in dets]), kind="stable")
        for d, k in enumerate(order):
            vid, i, _, traj = dets[k]
            trajs, det = recs[vid]
            max_overlap, max_index = trajectory_overlap(trajs, traj)
            if max_overlap >= thresh_t and not det[max_index]:
                tp[d] = 1.
                det[max_index] = True
            else:
                fp[d] = 1.
            per_pred[(vid, i)] = (max_overlap, max_index, bool(tp[d]))
        fp, tp = np.cumsum(fp), np.cumsum(tp)
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap_class[c] = voc_ap(rec, prec, use_07_metric)
    ap_class = sorted(ap_class.items(), key=lambda kv: kv[0])
    total_ap = 0.
    for _, ap in ap_class:
        total_ap += ap
    return total_ap / len(gt_classes), ap_class, per_pred


# ---------------------------------------------------------------------------------------------------- actions
def viou(t1, d1, t2, d2):
    """vIoU of two trajectories given as [begin, end) durations and one box per frame."""
    if d1[0] >= d2[1] or d1[1] <= d2[0]:
        return 0.
    v_ov = 0
    for f in range(max(d1[0], d2[0]), min(d1[1], d2[1])):
        a, b = t1[f - d1[0]], t2[f - d2[0]]
        v_ov += max(0, min(a[2], b[2]) - max(a[0], b[0]) + 1) * max(0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    vols = []
    for t in (t1, t2):
        v = 0
        for b in t:
            v += (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
        vols.append(v)
    return float(v_ov) / (vols[0] + vols[1] - v_ov)


def detection_scores_per_class(gt_actions, pred_actions, viou_threshold):
    """(prec, rec, hit_scores) of one category: gt_actions / pred_actions carry "id" (the video)."""
    pred_actions = sorted(pred_actions, key=lambda x: x["score"], reverse=True)
    detected = [False] * len(gt_actions)
    hit_scores = np.ones(len(pred_actions)) * -np.inf
    for pi, p in enumerate(pred_actions):
        ov_max, k_max = -float("inf"), -1
        for gi, g in enumerate(gt_actions):
            if detected[gi] or p["id"] != g["id"]:
                continue
            ov = viou(p["trajectory"], p["duration"], g["trajectory"], g["duration"])
            if ov >= viou_threshold and ov > ov_max:
                ov_max, k_max = ov, gi
        if k_max >= 0:
            hit_scores[pi] = p["score"]
            detected[k_max] = True
    tp = np.isfinite(hit_scores)
    cum_tp = np.cumsum(tp).astype(np.float32)
    cum_fp = np.cumsum(~tp).astype(np.float32)
    rec = cum_tp / np.maximum(len(gt_actions), np.finfo(np.float32).eps)
    prec = cum_tp / np.maximum(cum_tp + cum_fp, np.finfo(np.float32).eps)
    return prec, rec, hit_scores


def evaluate_actions(gt, pred, viou_threshold=0.5):
    """(mean_ap, ap_class dict, {category: (prec, rec, hit_scores)})."""
    gt_classes = set()
    for tracks in gt.values():
        for trk in tracks:
            gt_classes.add(trk["category"])
    preds = {}
    for vid, tracks in pred.items():
        for trk in tracks:
            preds.setdefault(trk["category"], []).append(dict(trk, id=vid))
    ap_class, curves = {}, {}
    for c in gt_classes:
        if c not in preds:
            ap_class[c] = 0.
            continue
        gts = [dict(trk, id=vid) for vid in gt for trk in gt[vid] if trk["category"] == c]
        curves[c] = detection_scores_per_class(gts, preds[c], viou_threshold)
        ap_class[c] = voc_ap(curves[c][1], curves[c][0])
    return np.mean(list(ap_class.values())), ap_class, curves


def relations_of(instances):
    """Action instances rewritten as relations with a constant predicate and obj_traj = sub_traj."""
    out = []
    for a in instances:
        r = {"triplet": (a["category"], "does", a["category"]), "duration": a["duration"], "sub_traj": a["trajectory"],
             "obj_traj": a["trajectory"]}
        if "score" in a:
            r["score"] = a["score"]
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------- packed stand-ins
# The device stage answered from the packed arrays (include/tspn_mi355x.h) by the statements above: what the host tests
# put in the kernels' place, so that the package's own packing and scatter run without a GPU.
INT32_MAX = 2 ** 31 - 1


def tiou_packed(pk):
    """(tiou, best, best_index, flags) of a packed object chunk; a pair that divides by zero stores 0 and sets its flag."""
    boxes, frames, traj, groups, pred_group = pk["boxes"], pk["frames"], pk["traj"], pk["groups"], pk["pred_group"]
    P = len(pred_group)

    def as_dict(t):
        row, n = traj[t]
        return {int(frames[row + i]): tuple(boxes[row + i].tolist()) for i in range(n)}
    out = np.zeros(int((groups[:, 1] * groups[:, 3]).sum()))
    best, index, flags = np.zeros(P), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    for p in range(P):
        p0, _, g0, ng, off = groups[pred_group[p]]
        pt = as_dict(p)
        max_overlap, max_index = 0.0, 0
        for j in range(ng):
            g = as_dict(g0 + j)
            try:
                v = tiou(g, pt)
            except ZeroDivisionError:
                v = 0.0
                flags[p] |= 1 if (g or pt) else 2
            if v > max_overlap:
                max_overlap, max_index = v, j
            out[off + (p - p0) * ng + j] = v
        best[p], index[p] = max_overlap, max_index
    return out, best, index, flags


def claim_packed(pk, best, index, thresh_t):
    """(claim, hit): predictions in packed order take the det[] flag of the ground truth they name."""
    groups, pred_group = pk["groups"], pk["pred_group"]
    P = len(pred_group)
    claim = np.full(pk["n_gt"], INT32_MAX, dtype=np.int32)
    hit = np.zeros(P, dtype=np.int8)
    for p in range(P):
        p0, _, g0, ng, _ = groups[pred_group[p]]
        if ng > 0 and best[p] >= thresh_t and claim[g0 - P + index[p]] == INT32_MAX:
            claim[g0 - P + index[p]] = p - p0
            hit[p] = 1
    return claim, hit


def relation_match_packed(pk, threshold):
    """(hit, match, zden) of a chunk in the relation evaluator's layout: the greedy match on min(subject, object vIoU)."""
    boxes, traj, groups = pk["boxes"], pk["traj"], pk["groups"]
    P = pk["n_pred"]

    def side(r, k):
        row, b, e = traj[2 * r + k]
        return [tuple(x) for x in boxes[row:row + e - b].tolist()], (int(b), int(e))
    hit, match = np.zeros(P, dtype=bool), np.full(P, -1, dtype=np.int64)
    for p0, n_pred, g0, ng, _ in groups:
        detected = [False] * ng
        for q in range(n_pred):
            ov_max, k_max = -float("inf"), -1
            for j in range(ng):
                if detected[j]:
                    continue
                ov = min(viou(*side(p0 + q, 0), *side(g0 + j, 0)), viou(*side(p0 + q, 1), *side(g0 + j, 1)))
                if ov >= threshold and ov > ov_max:
                    ov_max, k_max = ov, j
            if k_max >= 0:
                detected[k_max] = True
                hit[p0 + q], match[p0 + q] = True, k_max
    return hit, match, np.zeros(P, dtype=np.int32)
