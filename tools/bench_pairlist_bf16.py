#!/usr/bin/env python3
"""Time the bf16 pair-list stage against the pair grid of the same build at the cfg3 shape (one video: N = 64, T = 900,
D = 1024 -> C = 2048), HIP events, median of --iters launches after --warmup.

    python tools/bench_pairlist_bf16.py [--iters 20] [--warmup 3] [--n 64 --t 900 --c 2048]

Tables: the full canonical table as a list (what the plan and the chain walk cost), the 992 pairs among every other
tracklet (a proposal filter that keeps half the tracklets), 256 random pairs (a scattered top-k: almost every tile stays
occupied) and an empty table.  One JSON line per table; `plan_ms` is ops.pair_plan alone (its five allocations
included)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tspn_mi355x as tspn  # noqa: E402


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--t", type=int, default=900)
    ap.add_argument("--c", type=int, default=2048)
    args = ap.parse_args()
    N, T, C, H = args.n, args.t, args.c, 12
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn((N, T, 2 * C), generator=g, device=dev)
    hp = tspn.ops.pack_heads_bf16((0.1 * torch.randn((H, C), generator=g, device=dev)).contiguous())
    hb = torch.zeros(H, device=dev)
    canon = tspn.ops.pair_index(N, dev)
    half = torch.arange(0, N, 2, device=dev)
    keep = torch.isin(canon[:, 0], half) & torch.isin(canon[:, 1], half)
    rs = np.random.RandomState(0)
    tables = {"full_table_as_list": canon,
              "among_every_other_tracklet": canon[keep].contiguous(),
              "random_256": canon[torch.from_numpy(rs.permutation(N * (N - 1))[:256]).to(dev)].contiguous(),
              "empty": canon[:0].contiguous()}
    grid_ms = median_ms(lambda: tspn.ops.heads_pairgrid_bf16(y, 1, N, hp, hb, H), args.warmup, args.iters)
    print(json.dumps({"table": "grid (canonical, heads_pairgrid_bf16)", "P": N * (N - 1), "ms": round(grid_ms, 4)}), flush=True)
    for name, tab in tables.items():
        out = torch.empty((tab.shape[0], H, T), device=dev)
        ms = median_ms(lambda: tspn.ops.heads_pairlist_bf16(y, tab, 1, N, hp, hb, H, check_pairs=False, out=out),
                       args.warmup, args.iters)
        plan = median_ms(lambda: tspn.ops.pair_plan(tab, 1, N), args.warmup, args.iters)
        print(json.dumps({"table": name, "P": int(tab.shape[0]), "ms": round(ms, 4), "plan_ms": round(plan, 4),
                          "of_grid": round(ms / grid_ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
