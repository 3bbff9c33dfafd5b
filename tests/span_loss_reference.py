"""Float64 restatement of the span training targets and losses (DESIGN.md 2 "span training targets and losses"), written
from the formulas there: the labels in numpy, the losses in torch autograd on the CPU; the input generators of
tests/test_gpu_span_loss.py and tests/test_span_loss_host.py; and the training step of tests/train_reference.py with the two
new losses in place of the BCE on 'duration'.

Exactness of the inputs: ground-truth frames are integers and anchor widths multiples of 0.25, so t -+ size/2, inter and
union are exact in float64 and every IoU is ONE correctly rounded division of exact operands.  The equality of the
low-quality rule and the comparisons with the thresholds therefore come out the same on the device and here."""
import numpy as np
import torch

import oracle
from train_reference import oracle_weights, t as _t

POS_IOU, NEG_IOU, BETA = 0.7, 0.3, 1.0 / 9.0


def sizes64(sizes):
    """The widths as the library sees them: fp32 values (tspn_decode_spans_f32 takes them as fp32 too), then float64."""
    return np.asarray(sizes, dtype=np.float32).astype(np.float64)


def make_sizes(A, T):
    """(a + 1) T / A rounded to a multiple of 0.25 (BaseModel.anchor_sizes itself where A divides 4 T)."""
    return [max(0.25, round((a + 1) * T / A * 4) / 4) for a in range(A)]


def anchor_iou(gt, sizes, T):
    """iou [P, G, A, T] float64 of every anchor with every row (-1 at padding rows), valid [P, G]."""
    gt = np.asarray(gt, dtype=np.int64).reshape(len(gt), -1, 2)
    gs = gt[:, :, 0].astype(np.float64)[:, :, None, None]
    ge = gt[:, :, 1].astype(np.float64)[:, :, None, None]
    size = sizes64(sizes)[None, None, :, None]
    t = np.arange(T, dtype=np.float64)[None, None, None, :]
    half = size / 2.0
    lo, hi = t - half, t + half
    inter = np.maximum(0.0, np.minimum(hi, ge) - np.maximum(lo, gs))
    union = (hi - lo) + (ge - gs) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
    valid = gt[:, :, 1] > gt[:, :, 0]
    return np.where(valid[:, :, None, None], iou, -1.0), valid


def labels_ref(gt, sizes, T, pos_iou=POS_IOU, neg_iou=NEG_IOU):
    """label int8 [P, A, T], matched int8 [P, A, T], and what the input checks look at."""
    iou, valid = anchor_iou(gt, sizes, T)
    P, G, A = iou.shape[:3]
    has_gt = valid.any(axis=1)
    if G == 0:
        z = np.zeros((P, A, T), np.int8)
        return z, z - 1, {"iou": iou, "valid": valid, "lowq": np.zeros((P, A, T), bool), "thr": np.zeros((P, A, T), bool)}
    matched = iou.argmax(axis=1)                                    # the first maximum: the lower g on ties
    best = iou.max(axis=1)
    thr = best >= pos_iou
    label = np.where(thr, 1, np.where(best < neg_iou, 0, -1))
    rowmax = iou.reshape(P, G, -1).max(axis=2)
    lowq = ((iou == rowmax[:, :, None, None]) & (valid & (rowmax > 0))[:, :, None, None]).any(axis=1)
    label = np.where(lowq, 1, label)
    label = np.where(has_gt[:, None, None], label, 0).astype(np.int8)
    matched = np.where(has_gt[:, None, None], matched, -1).astype(np.int8)
    return label, matched, {"iou": iou, "valid": valid, "lowq": lowq & has_gt[:, None, None],
                            "thr": thr & has_gt[:, None, None]}


def targets_ref(gt, sizes, T, matched):
    """(t_c, t_w) float64 [P, A, T] of the matched rows; 0 where there is no matched ground truth."""
    gt = np.asarray(gt, dtype=np.int64).reshape(len(gt), -1, 2)
    P, A = matched.shape[:2]
    tc, tw = np.zeros(matched.shape), np.zeros(matched.shape)
    if gt.shape[1] == 0:
        return tc, tw
    m = np.clip(matched.astype(np.int64), 0, None)
    rows = np.take_along_axis(gt, m.reshape(P, -1, 1).repeat(2, axis=2), axis=1).reshape(P, A, T, 2).astype(np.float64)
    gs, ge = rows[..., 0], rows[..., 1]
    ok = (matched >= 0) & (ge > gs)
    size = sizes64(sizes)[None, :, None]
    t = np.arange(T, dtype=np.float64)[None, None, :]
    tc = np.where(ok, ((gs + ge) / 2.0 - t) / size, 0.0)
    tw = np.log(np.where(ok, (ge - gs) / size, 1.0))
    return tc, tw


def smooth_l1(d, beta):
    return torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)


def losses_torch(heads, gt, sizes, label, matched, mask=None, beta=BETA):
    """(loss_relationness, loss_duration_proposal, n_lab, n_pos) as torch values on heads' device and dtype; label,
    matched, mask as numpy or torch.  Only the anchors that enter a loss are read."""
    P, H, T = heads.shape
    A = H // 3
    dev = heads.device
    lab = torch.as_tensor(np.asarray(label) if not isinstance(label, torch.Tensor) else label).to(dev)
    on = torch.ones_like(lab, dtype=torch.bool) if mask is None else (torch.as_tensor(mask).to(dev) != 0)
    sel, pos = on & (lab >= 0), on & (lab == 1)
    x, y = heads[:, :A][sel], (lab[sel] == 1).to(heads.dtype)
    n_lab, n_pos = int(sel.sum()), int(pos.sum())
    loss_rel = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum() / max(1, n_lab)
    mt = matched.cpu().numpy() if isinstance(matched, torch.Tensor) else np.asarray(matched)
    tc, tw = targets_ref(gt.cpu().numpy() if isinstance(gt, torch.Tensor) else gt, sizes, T, mt)
    tc, tw = torch.from_numpy(tc).to(dev, heads.dtype), torch.from_numpy(tw).to(dev, heads.dtype)
    dc = heads[:, A::2][pos] - tc[pos]
    dw = heads[:, A + 1::2][pos] - tw[pos]
    loss_reg = (smooth_l1(dc, beta) + smooth_l1(dw, beta)).sum() / max(1, n_pos)
    return loss_rel, loss_reg, n_lab, n_pos


def span_loss_ref(heads, gt, sizes, mask=None, pos_iou=POS_IOU, neg_iou=NEG_IOU, beta=BETA):
    """heads fp32 numpy [P, 3A, T] -> (out float64 [4], dheads float64 [P, 3A, T], label, matched)."""
    P, H, T = heads.shape
    label, matched, _ = labels_ref(gt, sizes, T, pos_iou, neg_iou)
    h = torch.from_numpy(np.array(heads)).double().requires_grad_(True)
    lr, lp, n_lab, n_pos = losses_torch(h, gt, sizes, label, matched, mask, beta)
    (lr + lp).backward()
    return np.array([float(lr.detach()), float(lp.detach()), n_lab, n_pos]), h.grad.numpy(), label, matched


# --------------------------------------------------------------------------------------------------------- generators
PADDING = ((0, 0), (-1, -1), (9, 4))           # rows with end <= start


def make_gt(seed, P, G, T):
    """gt int64 [P, G, 2] with integer frames.  Where the shape allows it: pair 0 has only padding; pair 1 has two
    identical rows around a padding row (the tie goes to the lower g); pair 2 has a single one-frame span [k, k + 1)
    (its positives come from the low-quality rule alone under anchors wider than 1 / POS_IOU); the others have 1..G
    random spans at random rows, padding in between."""
    rs = np.random.RandomState(seed)
    gt = np.empty((P, G, 2), np.int64)
    for p in range(P):
        for g in range(G):
            gt[p, g] = PADDING[rs.randint(len(PADDING))]
        if G == 0 or (p == 0 and P >= 3):
            continue

        def span():
            s = rs.randint(0, T)
            return s, rs.randint(s + 1, T + 1)
        if p == 1 and G >= 2 and P >= 3:
            gt[p, 0] = gt[p, G - 1] = span()
        elif p == 2 and P >= 3:
            k = rs.randint(0, T)
            gt[p, rs.randint(G)] = (k, k + 1)
        else:
            for g in rs.permutation(G)[:rs.randint(1, G + 1)]:
                gt[p, g] = span()
    return gt


def make_heads(seed, gt, sizes, T, beta=BETA):
    """heads fp32 [P, 3A, T]: logits of a few units; the regression channels of the anchors with a matched row sit at
    their target plus a residual that is, in equal parts, inside (|d| < beta / 2) and outside (0.5 <= |d| < 1.5) the
    quadratic zone of the smooth L1, on both channels; elsewhere standard normal."""
    gt = np.asarray(gt)
    P, A = len(gt), len(sizes)
    rs = np.random.RandomState(seed)
    label, matched, _ = labels_ref(gt, sizes, T)
    tc, tw = targets_ref(gt, sizes, T, matched)
    heads = rs.randn(P, 3 * A, T) * 2.0
    for ch, tgt in ((0, tc), (1, tw)):
        inside = rs.rand(P, A, T) < 0.5
        res = np.where(inside, (rs.rand(P, A, T) - 0.5) * beta, (0.5 + rs.rand(P, A, T)) * rs.choice([-1.0, 1.0], (P, A, T)))
        heads[:, A + ch::2] = np.where(matched >= 0, tgt + res, heads[:, A + ch::2])
    return heads.astype(np.float32)


def input_conditions(gt, sizes, T, heads=None, beta=BETA):
    """What the tests need to find in their own inputs (every label, a pair whose positives are low-quality only, a tie, a
    pair without ground truth, both zones of the smooth L1), as booleans."""
    label, matched, info = labels_ref(gt, sizes, T)
    iou, valid = info["iou"], info["valid"]
    has_gt = valid.any(axis=1)
    pos = label == 1
    lowq_only = [bool(has_gt[p] and pos[p].any() and not (pos[p] & info["thr"][p]).any()) for p in range(len(gt))]
    best = iou.max(axis=1) if iou.shape[1] else np.full(label.shape, -1.0)
    tied = ((iou == best[:, None]) & valid[:, :, None, None]).sum(axis=1) >= 2 if iou.shape[1] else np.zeros(label.shape, bool)
    out = {"all three labels": all((label == v).any() for v in (1, 0, -1)),
           "a pair whose positives are low-quality only": any(lowq_only),
           "an anchor with two tied maxima": bool((tied & (best > 0)).any()),
           "a pair without ground truth": bool((~has_gt).any())}
    if heads is not None:
        A = len(sizes)
        tc, tw = targets_ref(gt, sizes, T, matched)
        for name, d in (("d_c", heads[:, A::2].astype(np.float64) - tc), ("d_w", heads[:, A + 1::2].astype(np.float64) - tw)):
            out[f"|{name}| < beta at a positive"] = bool((np.abs(d)[pos] < beta).any())
            out[f"|{name}| > beta at a positive"] = bool((np.abs(d)[pos] > beta).any())
    return out


# the hand-made threshold edges; every inter and union below is an exact integer or half-integer
def edge_cases():
    """[(name, gt [1, 1, 2], sizes, T, {(a, t): expected label})].  Anchor (a=0, t=10) of width 10 is [5, 15).  In the
    first two cases a narrower second width holds the row's largest IoU, so the 10-wide anchor's label comes from the
    thresholds alone, not from the low-quality rule."""
    return [
        # inter 7, union 10: 7/10 >= POS_IOU.  The 7-wide anchors at t = 8, 9 have 6.5 / 7.5
        ("iou 7/10 is positive", [[[5, 12]]], [10.0, 7.0], 21, {(0, 10): 1, (1, 8): 1, (1, 9): 1, (0, 20): 0}),
        # inter 3, union 10: 3/10 is not < NEG_IOU.  The 3-wide anchors at t = 13, 14 have 2.5 / 3.5 (positive)
        ("iou 3/10 is ignored", [[[12, 15]]], [10.0, 3.0], 21, {(0, 10): -1, (1, 13): 1, (1, 14): 1, (0, 0): 0}),
        ("a span equal to an anchor has iou 1", [[[5, 15]]], [10.0], 21, {(0, 10): 1, (0, 9): 1, (0, 7): -1, (0, 0): 0}),
        # [0, 1) under 10-wide anchors: inter 1, union 10 for t = 0..5, a plateau of six tied maxima, all positive by the
        # low-quality rule alone (1/10 < NEG_IOU); from t = 6 on the anchors miss the span
        ("a plateau of low-quality positives", [[[0, 1]]], [10.0], 21,
         {**{(0, t): 1 for t in range(6)}, **{(0, t): 0 for t in range(6, 21)}}),
    ]


# ------------------------------------------------------------------------------------------------ the training step
def train_reference_spans(segments, sd, sizes, pos_iou=POS_IOU, neg_iou=NEG_IOU, beta=BETA, dtype=torch.float64):
    """tests/train_reference.py's step with `loss_relationness` and `loss_duration_proposal` from ground-truth spans in
    place of the BCE on 'duration'.  `segments`: [(video dict, pairs [P,2], gt spans [P,G,2], targets [P,K])]; `sizes(T)`
    gives the anchor widths.  Returns losses and parameter gradients."""
    import torch.nn.functional as F
    w = {k: x.to(dtype).requires_grad_(True) for k, x in oracle_weights(sd).items()}
    losses = {}

    def add(name, value):
        losses[name] = losses[name] + value if name in losses else value

    for v, pairs, gt, targets in segments:
        pf, _ = oracle.pair_gather(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), pairs)
        pf = pf.to(dtype)
        rel, dur, _ = oracle.dpn_head(pf, w["conv_w"], w["conv_b"], w["dur_w"], w["dur_b"], w["rel_w"], w["rel_b"])
        heads = torch.cat([rel, dur], dim=1)
        T = heads.shape[2]
        gt = np.asarray(gt)
        label, matched, _ = labels_ref(gt, sizes(T), T, pos_iou, neg_iou)
        lr, lp, _, _ = losses_torch(heads, gt, sizes(T), label, matched, None, beta)
        add("loss_relationness", lr)
        add("loss_duration_proposal", lp)
        logit = oracle.predicate_head(pf.mean(dim=2), w["cls_w"], w["cls_b"])
        add("loss_rel", F.binary_cross_entropy(logit, targets.to(dtype)))
    sum(losses.values()).backward()
    return {k: float(x.detach()) for k, x in losses.items()}, {k: x.grad for k, x in w.items()}
