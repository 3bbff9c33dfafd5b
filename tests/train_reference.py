"""Float64 torch-autograd restatement of the training step (CPU), shared by tests/test_gpu_model.py and
tests/test_gpu_training_shapes.py: what the HIP forward + backward of model.py is compared with."""
import numpy as np
import torch
import torch.nn.functional as F

import oracle

DPN_PRE = "relpn.duration_proposal_network.dpn_head."


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def oracle_weights(sd):
    return {"conv_w": t(sd[DPN_PRE + "conv.weight"]), "conv_b": t(sd[DPN_PRE + "conv.bias"]),
            "dur_w": t(sd[DPN_PRE + "duration_pred.weight"]), "dur_b": t(sd[DPN_PRE + "duration_pred.bias"]),
            "rel_w": t(sd[DPN_PRE + "relness_pred.weight"]), "rel_b": t(sd[DPN_PRE + "relness_pred.bias"]),
            "cls_w": t(sd["classifier.rel_predictor.weight"]), "cls_b": t(sd["classifier.rel_predictor.bias"])}


def train_reference_segments(segments, sd, dtype=torch.float64, backward_calls=1):
    """The reference's intended DPN training step in plain torch autograd on the CPU: per segment materialised
    pair features -> oracle.dpn_head (relpn/dpn.py:69-73) -> BCEWithLogits (dpn.py:44); RelOIPool over the
    segment -> RelationPredictor -> BCE (model.py:59-64); every loss summed over the segments (model.py:62-64).
    `segments`: [(video dict, pairs [P,2], gt_dur, gt_rel or None, targets)].  `dtype` float64 is the reference;
    float32 gives the deviation a plain fp32 step has from it.  Returns losses and parameter gradients."""
    w = {k: x.to(dtype).requires_grad_(True) for k, x in oracle_weights(sd).items()}
    losses = {}

    def add(name, value):
        losses[name] = losses[name] + value if name in losses else value

    for v, pairs, gt_dur, gt_rel, targets in segments:
        pf, _ = oracle.pair_gather(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), pairs)
        pf = pf.to(dtype)
        rel, dur, _ = oracle.dpn_head(pf, w["conv_w"], w["conv_b"], w["dur_w"], w["dur_b"], w["rel_w"], w["rel_b"])
        add("loss_duration", F.binary_cross_entropy_with_logits(dur, gt_dur.to(dtype)))
        if gt_rel is not None:
            add("loss_relationness", F.binary_cross_entropy_with_logits(rel, gt_rel.to(dtype)))
        logit = oracle.predicate_head(pf.mean(dim=2), w["cls_w"], w["cls_b"])
        add("loss_rel", F.binary_cross_entropy(logit, targets.to(dtype)))
    total = sum(losses.values())
    for k in range(backward_calls):
        total.backward(retain_graph=k + 1 < backward_calls)
    return {k: float(x) for k, x in losses.items()}, {k: x.grad for k, x in w.items()}


def train_reference(v, pairs, sd, gt_dur, gt_rel, targets):
    """One segment, float64 (see train_reference_segments)."""
    return train_reference_segments([(v, pairs, gt_dur, gt_rel, targets)], sd)
