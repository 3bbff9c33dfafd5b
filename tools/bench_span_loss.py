#!/usr/bin/env python3
"""Time the span anchor targets and losses (`ops.span_anchor_labels` + `ops.span_loss`: tspn_span_anchor_labels,
tspn_span_loss_f32, tspn_span_loss_finish) against a torch composition of the same float64 maths on the same GPU, and one
training step of the tracklet form with a 'spans' target against the same step with a 'duration' target.  Prints one
JSON line.

Default shape: one cfg2 segment, P = 992 pairs (N = 32 tracklets), A = 4, T = 150, G = 3 ground-truth rows per pair.
The composition is the restatement of tests/span_loss_reference.py moved onto the device: labels from a [P, G, A, T]
float64 IoU tensor, losses and the gradient with respect to the heads by autograd; tests/test_span_loss_host.py holds its
labels to the numpy restatement.  Its results are compared with the kernels' before anything is timed (labels exact,
losses to 1e-9, gradient to 2^-22).  The two paths alternate inside one process, --repeat rounds after --warmup unmeasured
ones; a round of a path is --inner calls between two HIP events (a single call is tens of microseconds of GPU work), and
the figures are per call: median [min, max] in ms.  The training steps (forward, backward, no optimiser) alternate the same
way, one step per round; `--train-d 0` leaves them out.

    python tools/bench_span_loss.py [--P 992 --A 4 --T 150 --G 3] [--repeat 20] [--warmup 3] [--inner 20] [--train-d 2048]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _iou_torch(gt, sizes, T):
    dev = gt.device
    gs = gt[:, :, 0].double()[:, :, None, None]
    ge = gt[:, :, 1].double()[:, :, None, None]
    size = torch.tensor(sizes, dtype=torch.float32, device=dev).double()[None, None, :, None]
    t = torch.arange(T, dtype=torch.float64, device=dev)[None, None, None, :]
    half = size / 2.0
    lo, hi = t - half, t + half
    inter = torch.clamp(torch.minimum(hi, ge) - torch.maximum(lo, gs), min=0.0)
    union = (hi - lo) + (ge - gs) - inter
    valid = gt[:, :, 1] > gt[:, :, 0]
    return torch.where(valid[:, :, None, None], inter / union, -torch.ones((), dtype=torch.float64, device=dev)), valid


def labels_torch(gt, sizes, T, pos_iou, neg_iou):
    """(label int8 [P, A, T], matched int8 [P, A, T]) of span_loss_reference.labels_ref in torch, on gt's device (G >= 1)."""
    iou, valid = _iou_torch(gt, sizes, T)
    P, G = valid.shape
    has_gt = valid.any(dim=1)[:, None, None]
    best = iou.max(dim=1).values
    # the first maximum (the lower g on ties): torch.max's index on a tie is not specified
    g_idx = torch.arange(G, device=gt.device)[None, :, None, None]
    matched = torch.where(iou == best[:, None], g_idx, G).min(dim=1).values
    label = torch.where(best >= pos_iou, 1, torch.where(best < neg_iou, 0, -1))
    rowmax = iou.reshape(P, G, -1).max(dim=2).values
    lowq = ((iou == rowmax[:, :, None, None]) & (valid & (rowmax > 0))[:, :, None, None]).any(dim=1)
    label = torch.where(lowq, 1, label)
    return torch.where(has_gt, label, 0).to(torch.int8), torch.where(has_gt, matched, -1).to(torch.int8)


def composition(heads, gt, sizes, pos_iou, neg_iou, beta):
    """Labels, both losses and the gradient with respect to the heads, everything left on the device:
    (label, matched, out float64 [4], dheads float64)."""
    P, H, T = heads.shape
    A = H // 3
    label, matched = labels_torch(gt, sizes, T, pos_iou, neg_iou)
    h = heads.double().requires_grad_(True)
    lab = label.long()
    sel, pos = lab >= 0, lab == 1
    x, y = h[:, :A][sel], (lab[sel] == 1).double()
    n_lab, n_pos = sel.sum(), pos.sum()
    loss_rel = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum() / n_lab.clamp(min=1)
    rows = torch.gather(gt.double(), 1, matched.long().clamp(min=0).reshape(P, -1, 1).expand(-1, -1, 2)).view(P, A, T, 2)
    size = torch.tensor(sizes, dtype=torch.float32, device=heads.device).double()[None, :, None]
    t = torch.arange(T, dtype=torch.float64, device=heads.device)[None, None, :]
    gs, ge = rows[..., 0][pos], rows[..., 1][pos]
    size_p, t_p = size.expand(P, A, T)[pos], t.expand(P, A, T)[pos]
    d = torch.cat([h[:, A::2][pos] - ((gs + ge) / 2.0 - t_p) / size_p, h[:, A + 1::2][pos] - torch.log((ge - gs) / size_p)])
    sl1 = torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)
    loss_reg = sl1.sum() / n_pos.clamp(min=1)
    (loss_rel + loss_reg).backward()
    return label, matched, torch.stack([loss_rel.detach(), loss_reg.detach(), n_lab.double(), n_pos.double()]), h.grad


def _timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def _alternate(paths, warmup, repeat, inner):
    times = {k: [] for k in paths}
    for r in range(warmup + repeat):
        for k, fn in paths.items():                     # alternating: one round of each path per repeat
            ms = _timed(fn, inner)
            if r >= warmup:
                times[k].append(ms)
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in times.items()}


def train_steps(tspn, dev, N, T, D, G, gt):
    """(step with a 'spans' target, step with a 'duration' target) on one tracklet segment: forward + backward."""
    cfg = tspn.default_cfg()
    cfg.RELPN.USE_PPN = False
    cfg.RELPN.DPN.IN_CHANNELS = 2 * D
    cfg.PREDICT.FEATURE_DIM = 2 * D
    model = tspn.BaseModel(cfg).to(dev).train()
    g = torch.Generator().manual_seed(7)
    P, A, K = N * (N - 1), cfg.RELPN.DPN.NUM_ANCHORS_PER_LOCATION, cfg.PREDICT.PREDICATE_NUM
    plist = tspn.PairList.from_tracklets((torch.rand(N, T, D, generator=g) * 2 - 1)).to(dev)
    targets = (torch.rand(P, K, generator=g) < 0.05).float()
    t_spans, t_dur = tspn.TargetList(targets), tspn.TargetList(targets)
    t_spans.add_field("spans", gt.cpu())
    t_dur.add_field("duration", (torch.rand(P, 2 * A, T, generator=g) < 0.3).float())
    t_spans, t_dur = t_spans.to(dev), t_dur.to(dev)

    def step(tl):
        def run():
            model.zero_grad(set_to_none=True)
            sum(model([plist], [tl]).values()).backward()
        return run
    return step(t_spans), step(t_dur)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("P", 992), ("A", 4), ("T", 150), ("G", 3), ("repeat", 20), ("warmup", 3), ("inner", 20),
                          ("train-d", 2048), ("train-repeat", 5)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    import span_loss_reference as ref
    import tspn_mi355x as tspn
    if not torch.cuda.is_available():
        raise SystemExit("bench_span_loss: needs a HIP device (there is nothing to time on a CPU)")
    ops, dev = tspn.ops, torch.device("cuda", 0)
    P, A, T, G = a.P, a.A, a.T, a.G
    sizes = [(i + 1) * float(T) / A for i in range(A)]
    gt_np = ref.make_gt(11, P, G, T)
    heads = torch.from_numpy(ref.make_heads(12, gt_np, sizes, T)).to(dev)
    gt = torch.from_numpy(gt_np).to(dev)

    def kernels():
        label, matched = ops.span_anchor_labels(gt, sizes, T, ref.POS_IOU, ref.NEG_IOU)
        out, dh = ops.span_loss(heads, gt, sizes, label, matched, beta=ref.BETA)
        return label, matched, out, dh

    def comp():
        return composition(heads, gt, sizes, ref.POS_IOU, ref.NEG_IOU, ref.BETA)

    k, c = kernels(), comp()
    assert torch.equal(k[0], c[0]) and torch.equal(k[1], c[1]), "labels differ"
    assert torch.equal(k[2][2:], c[2][2:]) and torch.allclose(k[2][:2], c[2][:2], rtol=1e-9, atol=0), (k[2], c[2])
    assert torch.allclose(k[3].double(), c[3], rtol=2.0 ** -22, atol=0), "gradients differ"
    counts = {"n_lab": int(k[2][2]), "n_pos": int(k[2][3])}
    del k, c
    res = {"shape": {"P": P, "A": A, "T": T, "G": G}, "repeat": a.repeat, "warmup": a.warmup, "inner": a.inner, **counts,
           "ms_per_call": _alternate({"kernels": kernels, "composition": comp}, a.warmup, a.repeat, a.inner),
           "iou_tensor_the_composition_forms_mib": round(P * G * A * T * 8 / 2 ** 20, 2)}
    res["composition_over_kernels"] = round(res["ms_per_call"]["composition"]["median"] /
                                            res["ms_per_call"]["kernels"]["median"], 2)
    if a.train_d > 0:
        N = int(round((1 + (1 + 4 * P) ** 0.5) / 2))
        if N * (N - 1) != P:
            raise SystemExit(f"bench_span_loss: the training step needs P = N (N - 1) pairs (P = {P})")
        spans_step, dur_step = train_steps(tspn, dev, N, T, a.train_d, G, torch.from_numpy(gt_np))
        res["train_step"] = {"N": N, "T": T, "D": a.train_d, "repeat": a.train_repeat,
                             "ms": _alternate({"spans": spans_step, "duration": dur_step}, 1, a.train_repeat, 1)}
        res["train_step"]["spans_minus_duration_ms"] = round(res["train_step"]["ms"]["spans"]["median"] -
                                                             res["train_step"]["ms"]["duration"]["median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
