#!/usr/bin/env python
"""Isolated timing of the canonical pair stage at one shape (default: config 2, 16 videos): the split-fp16 MFMA form
(tspn_heads_pairgrid_f16x3, with its two pack kernels) against heads_pairgrid4_kernel (with its pack kernel), both in one
process, taking turns, HIP events around each launch.  The split-fp16 form is timed with its diagonal-tile skip
(ops.heads_pair_f16x3_set_diag_skip) on, the default, and off, the walk of all eight objects in every tile.

heads_pairgrid4_kernel has no entry of its own: it is reached through the fused pass with direct-tap conv weights, and
timed from the pass's `conv end` event to an event recorded behind the pass, so the interval holds the pair stage and
nothing else.  Prints one JSON line.

    python tools/bench_pair_stage_f16x3.py [--B 16 --N 32 --T 150 --D 2048 --iters 10 --rounds 3 --no-fp32]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--T", type=int, default=150)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--A", type=int, default=4)
    ap.add_argument("--K", type=int, default=132)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-fp32", action="store_true", help="time the split-fp16 form only (a counter pass over it alone)")
    a = ap.parse_args()
    import tspn_mi355x as tspn
    ops = tspn.ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, N, T, D = a.B, a.N, a.T, a.D
    C, H = 2 * D, 3 * a.A
    ldt = (T + 3) // 4 * 4
    rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(dev)
    feats = rnd(B * N, T, D)
    conv_packed = rnd(3, D, 2 * C, std=0.01)
    conv_bias = rnd(C, std=0.1)
    head_w, head_b = rnd(H, C, std=0.02), rnd(H, std=0.1)
    cls_w, cls_b = rnd(a.K, C, std=0.02), rnd(a.K, std=0.1)
    pairs = torch.cat([torch.tensor([[s, o] for s in range(N) for o in range(N) if s != o]) + b * N
                       for b in range(B)]).to(dev)
    y = (torch.rand(B * N, 2 * C, ldt, generator=g) * 2 - 1).to(dev)
    split = torch.empty(ops.heads_pairgrid_f16x3_split_bytes(C, H), dtype=torch.uint8, device=dev)
    out = torch.empty(B * N * (N - 1), H, T, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()

    def fp32_once():
        ops.forward_fused(feats, pairs, B, N, conv_packed, conv_bias, head_w, head_b, cls_w, cls_b,
                          out_heads=out, check_pairs=False, conv_events=(ev[0], ev[1]), canonical_pairs=True)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[1].elapsed_time(ev[2])

    def f16_once(skip=1):
        prev = ops.heads_pair_f16x3_set_diag_skip(skip)
        ev[2].record()
        ops.heads_pairgrid_f16x3(y, B, N, head_w, head_b, T=T, split_buf=split, out=out)
        ev[3].record()
        torch.cuda.synchronize()
        ops.heads_pair_f16x3_set_diag_skip(prev)
        return ev[2].elapsed_time(ev[3])

    if not a.no_fp32:
        fp32_once()                   # warm-up (module load, LDS limits)
    f16_once(1), f16_once(0)
    t32, t16, t16_off = [], [], []
    for _ in range(a.rounds):
        if not a.no_fp32:
            t32 += [fp32_once() for _ in range(a.iters)]
        t16 += [f16_once(1) for _ in range(a.iters)]
        t16_off += [f16_once(0) for _ in range(a.iters)]
    summ = lambda v: {"mean_ms": statistics.mean(v), "median_ms": statistics.median(v), "sigma_ms": statistics.pstdev(v),
                      "min_ms": min(v), "max_ms": max(v)}
    res = {"shape": {"B": B, "N": N, "T": T, "D": D, "C": C, "H": H}, "launches_each": len(t16),
           "heads_pair_f16x3": summ(t16), "heads_pair_f16x3_diag_skip_off": summ(t16_off)}
    if t32:
        res["heads_pairgrid4"] = summ(t32)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
