"""References for the relations decoded with their temporal spans (`tspn_decode_span_relations_f32`):

* `compose`: the unfused composition in torch.  Given q [S*P*J, K] (what `ops.span_predicate` returns for the flattened
  (pair, span) rows) and the `decode_spans` outputs: per row a stable descending sort -> the first R, times the span
  score in fp32, rows j >= count dropped, flattened, a stable descending sort -> the first M, then the gathers.
* `associate`: a plain-Python restatement of `greedy_relational_association` for span-bounded (4-tuple) predictions.
"""
import numpy as np
import torch


def flat_rows(pairs, n):
    """pairs int64 [S,P,2] segment-local -> [S*P,2] global tracklet ids (segment s owns tracklets [s*n, (s+1)*n))."""
    S = pairs.shape[0]
    off = (torch.arange(S, dtype=torch.int64, device=pairs.device) * n).view(S, 1, 1)
    return (pairs + off).reshape(-1, 2)


def span_rows(pairs, n, spans):
    """The (global pair, span) rows `ops.span_predicate` takes for spans [S*P,J,2]: ([S*P*J,2], [S*P*J,2])."""
    J = spans.shape[-2]
    g = flat_rows(pairs, n)
    return g.repeat_interleave(J, dim=0).contiguous(), spans.reshape(-1, 2).contiguous()


def compose(q, pairs, spans, span_scores, span_counts, cls_logits, topk_per_span, topk_per_seg):
    """q [S*P*J, K] fp32, pairs [S,P,2], spans [S*P,J,2], span_scores [S*P,J], span_counts [S*P], cls_logits [S,N,NO]
    (all on one device) -> a list of S dicts of host numpy arrays: scores, triplets, pair_tids, spans, span_rank (each
    with `valid` rows) and valid."""
    S, P, _ = pairs.shape
    J = spans.shape[-2]
    K = q.shape[1]
    R = min(topk_per_span, K)
    vals, idx = torch.sort(q.view(S, P, J, K), dim=-1, descending=True, stable=True)
    vals, idx = vals[..., :R], idx[..., :R]
    prod = vals * span_scores.view(S, P, J, 1)                                      # one fp32 product
    j = torch.arange(J, device=q.device).view(1, 1, J, 1)
    keep = (j < span_counts.view(S, P, 1, 1)).expand(S, P, J, R)
    spans = spans.view(S, P, J, 2)
    cls = torch.argmax(cls_logits, dim=-1)                                          # [S,N]
    out = []
    for s in range(S):
        flat = keep[s].reshape(-1).nonzero().view(-1)                               # ascending flat index
        order = torch.sort(prod[s].reshape(-1)[flat], descending=True, stable=True)[1][:topk_per_seg]
        win = flat[order]
        row = win // R
        p, jj = row // J, row % J
        tids = pairs[s, p]
        trip = torch.stack([cls[s, tids[:, 0]], idx[s].reshape(-1)[win], cls[s, tids[:, 1]]], dim=1)
        out.append({"scores": prod[s].reshape(-1)[win].cpu().numpy(), "triplets": trip.cpu().numpy(),
                    "pair_tids": tids.cpu().numpy(), "spans": spans[s, p, jj].cpu().numpy(),
                    "span_rank": jj.cpu().numpy(), "valid": int(win.numel())})
    return out


def _iou(t1, t2):
    """IoU on the common frames, with the package's own box arithmetic (the float32 / float64 roundings of the
    reference's trajectory.py are not what this restatement is about)."""
    from tspn_mi355x.association import _cubic_iou_1x1
    if t1["pe"] <= t2["ps"] or t2["pe"] <= t1["ps"]:
        return 0
    if t1["ps"] > t2["ps"]:
        t1, t2 = t2, t1
    return _cubic_iou_1x1(t1["rois"][t2["ps"] - t1["ps"]:t1["pe"] - t1["ps"]], t2["rois"][:t1["pe"] - t2["ps"]])


def _follows(prev, cur):
    return prev["ps"] <= cur["ps"] < prev["pe"] <= cur["pe"]


def _merge(t1, t2):
    ov = t1["pe"] - t2["ps"]
    n1 = len(t1["rois"])
    t1["rois"][n1 - ov:] = (t1["rois"][n1 - ov:] + t2["rois"][:ov]) / 2
    t1["rois"] = np.concatenate([t1["rois"], t2["rois"][ov:]])
    t1["pe"] = t2["pe"]


def associate(short_term_relations, trajectories, max_traj_num_in_clip=100):
    """Span-bounded predictions (score, triplet, (s_idx, o_idx), (a, e)) per segment -> serialised video relations,
    ids kept (dataset=None).  `trajectories`: {(vid, fstart, fend): [N, L, 4] boxes}."""
    rels, last = [], []
    for i, (index, (preds, _, _)) in enumerate(sorted(short_term_relations, key=lambda x: int(x[0][1]))):
        _, fs, _ = index
        boxes = np.asarray(trajectories[index], dtype=np.float64)
        preds = sorted(preds, key=lambda x: x[0], reverse=True)[:max_traj_num_in_clip]
        order = sorted(last, key=lambda r: np.mean(r["confs"]), reverse=True)
        cur = []
        for score, trip, (si, oi), (a, e) in preds:
            a, e = int(a), int(e)
            st = {"ps": fs + a, "pe": fs + e, "rois": boxes[int(si), a:e].copy()}
            ot = {"ps": fs + a, "pe": fs + e, "rois": boxes[int(oi), a:e].copy()}
            hit = None
            for r in order if i > 0 else ():
                if any(r is c for c in cur) or tuple(int(v) for v in r["trip"]) != tuple(int(v) for v in trip):
                    continue
                if not (st["ps"] < r["fend"] and ot["ps"] < r["fend"]):
                    continue
                if not (_follows(r["s"], st) and _follows(r["o"], ot)):
                    continue
                if _iou(r["s"], st) >= 0.5 and _iou(r["o"], ot) >= 0.5:
                    hit = r
                    break
            if hit is not None:
                _merge(hit["s"], st)
                _merge(hit["o"], ot)
                hit["confs"].append(score)
                hit["fstart"], hit["fend"] = hit["s"]["ps"], hit["o"]["pe"]
            else:
                hit = {"trip": trip, "s": st, "o": ot, "confs": [score if i == 0 else 1], "fstart": st["ps"], "fend": st["pe"]}
                rels.append(hit)
            cur.append(hit)
        last = cur
    return [{"triplet": [int(v) for v in r["trip"]], "score": float(np.mean(r["confs"])),
             "duration": [int(r["fstart"]), int(r["fend"])],
             "sub_traj": list(map(tuple, r["s"]["rois"].tolist())), "obj_traj": list(map(tuple, r["o"]["rois"].tolist()))}
            for r in rels]
