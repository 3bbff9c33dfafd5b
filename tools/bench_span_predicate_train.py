#!/usr/bin/env python3
"""Time the span-pooled predicate training (`_SpanPredicateLossFn`: ops.span_predicate_loss, ops.span_predicate_grad and
the dW GEMM; DESIGN.md §2 "span-pooled predicate training") against a torch composition of the same loss on the same GPU.
Prints one JSON line.

Default shape: cfg2, 16 videos of N = 32 tracklets, T = 150, D = 2048, K = 132, G = 4 span rows per pair, canonical pair
tables (P = 16 * 992).  Span counts are drawn from {0, 1, 2, G, G + 1}, spans uniformly, labels with density 0.02.
The composition leg pools the rows with torch -- a float64 cumsum of the features over time, a gather of the two prefix
rows per row and half, the division by the span length -- and runs `_PredicateHeadFn` (the library's GEMM with the sigmoid
in its reduce kernel, HIP backward) and `F.binary_cross_entropy` per segment on the pooled rows: what a caller had to write
before.  Both legs compute loss_rel, dW and db; they are compared before anything is timed (loss rtol 2e-5, gradients atol
2e-4 max|ref|).  The legs alternate inside one process, --repeat rounds after --warmup unmeasured ones, one call per round
between two HIP events: median [min, max] in ms.  The stages of the new leg are timed the same way in rounds of their own.

    python tools/bench_span_predicate_train.py [--videos 16 --N 32 --T 150 --D 2048 --K 132 --G 4] [--repeat 10] [--warmup 2]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(dev, S, N, T, D, K, G, seed=5):
    g = torch.Generator().manual_seed(seed)
    feats = (torch.rand(S * N, T, D, generator=g) * 2 - 1).to(dev)
    local = torch.tensor([(i, j) for i in range(N) for j in range(N) if i != j], dtype=torch.int64)
    P1 = local.shape[0]
    pairs = torch.cat([local + s * N for s in range(S)]).to(dev)
    pair_off = (torch.arange(S + 1, dtype=torch.int64) * P1).to(dev)
    choices = torch.tensor([0, 1, 2, G, G + 1], dtype=torch.int32)
    count = choices[torch.randint(0, len(choices), (S * P1,), generator=g)]
    a = torch.randint(0, T, (S * P1, G), generator=g)
    e = (a + 1 + (torch.rand(S * P1, G, generator=g) * (T - a)).long()).clamp(max=T)      # a < e <= T
    spans = torch.stack([a, e], dim=2)
    spans[torch.arange(G)[None, :] >= count.clamp(max=G)[:, None].long()] = 0
    labels = (torch.rand(S * P1, G, K, generator=g) < 0.02).float()
    w = (torch.randn(K, 2 * D, generator=g) / (2 * D) ** 0.5).to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(K, generator=g)).to(dev).requires_grad_(True)
    return feats, pairs, pair_off, spans.to(dev), count.to(dev), labels.to(dev), w, b


def composition(mod, feats, pairs, pair_off_host, spans, count, labels, w, b):
    """loss_rel over explicitly pooled rows: the row table and the pooling in torch, the head and its backward on the
    library's GEMM.  Returns the loss (its backward fills w.grad / b.grad)."""
    NT, T, D = feats.shape
    P, G = spans.shape[:2]
    rows = torch.where(count >= 1, count.clamp(max=G), (count == 0).int())
    valid = torch.arange(G, device=feats.device)[None, :] < rows[:, None]
    neg = (count == 0)[:, None].expand(-1, G)
    a = torch.where(neg, 0, spans[..., 0])
    e = torch.where(neg, T, spans[..., 1])
    ps = torch.zeros((NT, T + 1, D), dtype=torch.float64, device=feats.device)
    ps[:, 1:] = torch.cumsum(feats, dim=1, dtype=torch.float64)
    loss = 0
    for s in range(len(pair_off_host) - 1):
        lo, hi = pair_off_host[s], pair_off_host[s + 1]
        p_idx, g_idx = torch.nonzero(valid[lo:hi], as_tuple=True)
        p_idx = p_idx + lo
        aa, ee = a[p_idx, g_idx], e[p_idx, g_idx]
        inv = 1.0 / (ee - aa).double()[:, None]
        halves = [((ps[pairs[p_idx, h], ee] - ps[pairs[p_idx, h], aa]) * inv).float() for h in range(2)]
        y = torch.where(neg[p_idx, g_idx][:, None], 0.0, labels[p_idx, g_idx])
        q = mod._PredicateHeadFn.apply(torch.cat(halves, dim=1), w, b)
        loss = loss + F.binary_cross_entropy(q, y)
    return loss


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(paths, warmup, repeat):
    times = {k: [] for k in paths}
    for r in range(warmup + repeat):
        for k, fn in paths.items():                     # alternating: one call of each path per round
            ms = _timed(fn)
            if r >= warmup:
                times[k].append(ms)
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("videos", 16), ("N", 32), ("T", 150), ("D", 2048), ("K", 132), ("G", 4), ("repeat", 10), ("warmup", 2)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    import tspn_mi355x as tspn
    if not torch.cuda.is_available():
        raise SystemExit("bench_span_predicate_train: needs a HIP device (there is nothing to time on a CPU)")
    ops, mod, dev = tspn.ops, importlib.import_module(tspn.BaseModel.__module__), torch.device("cuda", 0)
    feats, pairs, pair_off, spans, count, labels, w, b = make_inputs(dev, a.videos, a.N, a.T, a.D, a.K, a.G)
    off_host = pair_off.cpu().tolist()

    def grads_of(loss):
        w.grad = b.grad = None
        loss.backward()
        return loss.detach().double().item(), w.grad.clone(), b.grad.clone()

    def new():
        return mod._SpanPredicateLossFn.apply(feats, pairs, spans, count, labels, w, b, pair_off)

    def comp():
        return composition(mod, feats, pairs, off_host, spans, count, labels, w, b)

    k, c = grads_of(new()), grads_of(comp())
    assert abs(k[0] - c[0]) <= 2e-5 * abs(c[0]), (k[0], c[0])
    for x, y in zip(k[1:], c[1:]):
        assert float((x - y).abs().max()) <= 2e-4 * float(y.abs().max()) + 1e-9, float((x - y).abs().max())
    del k, c

    def step(fn):
        def run():
            w.grad = b.grad = None
            fn().backward()
        return run

    res = {"shape": {"videos": a.videos, "N": a.N, "T": a.T, "D": a.D, "K": a.K, "G": a.G, "P": pairs.shape[0],
                     "rows": int(torch.where(count >= 1, count.clamp(max=a.G), (count == 0).int()).sum())},
           "repeat": a.repeat, "warmup": a.warmup,
           "ms_per_step": _alternate({"span_predicate_loss_fn": step(new), "composition": step(comp)}, a.warmup, a.repeat)}
    res["composition_over_new"] = round(res["ms_per_step"]["composition"]["median"] /
                                        res["ms_per_step"]["span_predicate_loss_fn"]["median"], 2)
    # the stages of the new leg, each between its own events
    wd, bd = w.detach(), b.detach()
    NT, T = feats.shape[:2]
    state = {}

    def loss_stage():
        state["loss"] = ops.span_predicate_loss(feats, pairs, spans, count, labels, wd, bd, pair_off=pair_off)

    def grad_stage():
        state["grad"] = ops.span_predicate_grad(state["loss"][2], pairs, spans, count, NT, T, scratch=state["loss"][4])

    def gemm_stage():
        mod._span_cls_weight_grad(state["grad"][1], feats)

    res["ms_per_stage"] = _alternate({"loss (projection GEMM, prefix sums, rows, loss, finish)": loss_stage,
                                      "grad (db, dG)": grad_stage, "dW GEMM (two transposes, one product)": gemm_stage},
                                     a.warmup, a.repeat)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
