#!/usr/bin/env python3
"""Time the fused span relation decode (`ops.decode_span_relations`) against the unfused composition
(`ops.span_predicate` on the flattened (pair, span) rows + two stable torch sorts + gathers) on synthetic data and print
one JSON line.

Default shape: cfg2, S=16 segments of N=32 tracklets, T=150, D=2048, K=132 predicates, J=4 spans per pair, 20 predicates
kept per span, 200 relations per segment.  Spans are `ops.decode_spans(top_k=J)` of random DPN heads.  Both paths start
with the same stage: G = f W'^T and its float64 prefix sums (timed alone as a one-row `span_predicate` call).  The two
paths alternate inside one process, --repeat times after --warmup unmeasured rounds; times are HIP events around each
call, reported as median [min, max] in ms.  `after_stage_a_ms` is each path's median minus the median of the shared
stage.  `peak_alloc_mib` is the peak of torch's allocator over one call of each path, inputs excluded.  The results are
compared bit for bit before anything is timed.

    python tools/bench_span_relations.py [--S 16 --N 32 --T 150 --D 2048 --K 132 --J 4] [--repeat 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tspn_mi355x as tspn  # noqa: E402


def composition(ops, c, R, M):
    """The unfused path, everything left on the device: (scores, triplets, pair_tids, spans, span_rank) per segment."""
    S, P, J, N = c["S"], c["P"], c["J"], c["N"]
    off = (torch.arange(S, dtype=torch.int64, device=c["pairs"].device) * N).view(S, 1, 1)
    rows_p = (c["pairs"] + off).reshape(-1, 2).repeat_interleave(J, dim=0).contiguous()
    q = ops.span_predicate(c["feats"], rows_p, c["spans"].reshape(-1, 2), c["w"], c["b"])       # [S*P*J, K]
    K = q.shape[1]
    R = min(R, K)
    vals, idx = torch.sort(q.view(S, P, J, K), dim=-1, descending=True, stable=True)
    vals, idx = vals[..., :R], idx[..., :R]
    prod = vals * c["score"].view(S, P, J, 1)
    keep = torch.arange(J, device=q.device).view(1, 1, J, 1) < c["count"].view(S, P, 1, 1)
    cls = torch.argmax(c["cls"], dim=-1)
    spans = c["spans"].view(S, P, J, 2)
    out = []
    for s in range(S):
        flat = keep[s].expand(P, J, R).reshape(-1).nonzero().view(-1)
        win = flat[torch.sort(prod[s].reshape(-1)[flat], descending=True, stable=True)[1][:M]]
        row = win // R
        p, j = row // J, row % J
        tids = c["pairs"][s, p]
        trip = torch.stack([cls[s, tids[:, 0]], idx[s].reshape(-1)[win], cls[s, tids[:, 1]]], dim=1)
        out.append((prod[s].reshape(-1)[win], trip, tids, spans[s, p, j], j))
    return out


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("S", 16), ("N", 32), ("T", 150), ("D", 2048), ("K", 132), ("J", 4), ("R", 20), ("M", 200),
                          ("repeat", 20), ("warmup", 3)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    ops = tspn.ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    u = lambda *sh: (torch.rand(*sh, generator=g) * 2 - 1).to(dev)   # noqa: E731
    S, N, T, D, K, J = a.S, a.N, a.T, a.D, a.K, a.J
    pairs = ops.pair_index(N, dev)
    P = pairs.shape[0]
    A = 4
    c = {"S": S, "N": N, "P": P, "J": J, "feats": u(S * N, T, D), "w": u(K, 2 * D) * (D ** -0.5), "b": u(K) * 0.1,
         "cls": u(S, N, 35), "pairs": pairs.unsqueeze(0).repeat(S, 1, 1).contiguous()}
    sp = ops.decode_spans(u(S * P, 3 * A, T), [(i + 1) * float(T) / A for i in range(A)], top_k=J)
    c["spans"], c["score"], c["count"] = sp["span"], sp["score"], sp["count"]
    one_pair, one_span = torch.zeros((1, 2), dtype=torch.int64, device=dev), torch.tensor([[0, T]], device=dev)

    def fused():
        return ops.decode_span_relations(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["w"], c["b"],
                                         c["cls"], topk_per_span=a.R, topk_per_seg=a.M, check_pairs=False)

    def comp():
        return composition(ops, c, a.R, a.M)

    def stage_a():
        return ops.span_predicate(c["feats"], one_pair, one_span, c["w"], c["b"])

    # same results, to the bit
    f, want = fused(), comp()
    valid = f[5].tolist()
    for s, w in enumerate(want):
        assert valid[s] == w[0].numel(), (s, valid[s], w[0].numel())
        assert torch.equal(f[0][s, :valid[s]].view(torch.int32), w[0].view(torch.int32))
        assert all(torch.equal(x[s, :valid[s]], y) for x, y in zip(f[1:5], w[1:]))
    del f, want

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    paths = {"fused": fused, "composition": comp, "stage_a": stage_a}
    times = {k: [] for k in paths}
    for r in range(a.warmup + a.repeat):
        for k, fn in paths.items():                     # alternating: one call of each per round
            ms = timed(fn)
            if r >= a.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"shape": {"S": S, "N": N, "T": T, "D": D, "K": K, "J": J, "P": P, "topk_per_span": a.R, "topk_per_seg": a.M},
           "repeat": a.repeat, "warmup": a.warmup,
           "ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()},
           "after_stage_a_ms": {k: round(med[k] - med["stage_a"], 4) for k in ("fused", "composition")},
           "composition_spread_ms": round(max(times["composition"]) - min(times["composition"]), 4),
           "peak_alloc_mib": {k: round(peak(fn), 2) for k, fn in paths.items()},
           "candidate_rows": S * P * J, "logits_the_composition_writes_mib": round(S * P * J * K * 4 / 2 ** 20, 2)}
    res["fused_over_composition_after_stage_a"] = round(res["after_stage_a_ms"]["fused"] /
                                                        max(res["after_stage_a_ms"]["composition"], 1e-9), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
