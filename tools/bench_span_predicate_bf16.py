#!/usr/bin/env python3
"""Time span pooling + predicate head and the span relation decode on a bf16 segment at the cfg3 shape (one video:
N = 64, T = 900, D = 1024, K = 132; all 4032 pairs x J = 4 spans), HIP events, median of --iters launches after --warmup,
the two ways interleaved in one process:

  bf16    ops.span_predicate_bf16 / ops.decode_span_relations_bf16 (csrc/spanbf16/): float64 prefix sums of the bf16
          features, pooled bf16 rows, the predicate head on the bf16 MFMAs;
  upcast  what classify_spans / decode_span_relations did with a bf16 segment before: the features cast to fp32, then
          ops.span_predicate / ops.decode_span_relations with the fp32 classifier (the cast is timed with it: every call
          paid it).

    python tools/bench_span_predicate_bf16.py [--iters 10] [--warmup 2] [--n 64 --t 900 --d 1024 --k 132 --j 4]

One JSON line per measurement, with the workspace bytes of both ways and the shader clock while it ran (`clock_mhz`, the
hwmon node bench.py samples; null where it is not readable)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tspn_mi355x as tspn  # noqa: E402
from bench import ClockSampler  # noqa: E402


def interleaved_ms(fns, warmup, iters):
    """(median milliseconds of each of `fns`, their launches taking turns; the clock while they ran)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    props = torch.cuda.get_device_properties(0)
    clock = ClockSampler("%04x:%02x:%02x.0" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0),
                                               getattr(props, "pci_device_id", 0)))
    clock.start()
    evs = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    mhz = clock.stop()
    return [float(np.median([a.elapsed_time(b) for a, b in e])) for e in evs], mhz and {k: mhz[k] for k in ("mean", "min", "max")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--t", type=int, default=900)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=132)
    ap.add_argument("--j", type=int, default=4)
    args = ap.parse_args()
    N, T, D, K, J = args.n, args.t, args.d, args.k, args.j
    ops, lib = tspn.ops, tspn._abi.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    f16 = (torch.rand((N, T, D), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    w = (0.05 * torch.randn((K, 2 * D), generator=g, device=dev)).contiguous()
    b = (0.1 * torch.randn((K,), generator=g, device=dev)).contiguous()
    packed = ops.pack_span_cls_bf16(w)
    pairs = ops.pair_index(N, dev)
    P = pairs.shape[0]
    rs = np.random.RandomState(0)
    a = rs.randint(0, T, size=(P, J))
    e = np.minimum(a + 1 + rs.randint(0, T, size=(P, J)), T)
    spans = torch.from_numpy(np.stack([a, e], axis=2).astype(np.int64)).to(dev)             # [P, J, 2]
    rows_p = pairs.repeat_interleave(J, dim=0).contiguous()
    rows_s = spans.reshape(-1, 2).contiguous()
    R = P * J
    shape = {"N": N, "T": T, "D": D, "K": K, "pairs": P, "J": J, "rows": R}

    out = torch.empty((R, K), device=dev)
    ws_bf16 = lib.tspn_span_predicate_bf16_workspace_bytes(N, T, D, K, R)
    ws_f32 = lib.tspn_span_predicate_workspace_bytes(N, T, D, K)
    ws = torch.empty(ws_bf16, dtype=torch.uint8, device=dev)
    ms, mhz = interleaved_ms([lambda: ops.span_predicate_bf16(f16, rows_p, rows_s, packed, b, K, out=out, workspace=ws),
                              lambda: ops.span_predicate(f16.float(), rows_p, rows_s, w, b)], args.warmup, args.iters)
    print(json.dumps(dict(shape, what="span_predicate", bf16_ms=round(ms[0], 4), upcast_ms=round(ms[1], 4),
                          upcast_over_bf16=round(ms[1] / ms[0], 3), bf16_workspace_bytes=int(ws_bf16),
                          upcast_workspace_bytes=int(ws_f32), upcast_fp32_copy_bytes=N * T * D * 4, clock_mhz=mhz)), flush=True)
    del ws, out

    score = torch.rand((P, J), generator=g, device=dev)
    count = torch.full((P,), J, dtype=torch.int64, device=dev)
    clog = torch.randn((1, N, 35), generator=g, device=dev)
    p3 = pairs.view(1, P, 2).contiguous()
    ms, mhz = interleaved_ms([lambda: ops.decode_span_relations_bf16(f16, p3, spans, score, count, packed, b, K, clog,
                                                                check_pairs=False),
                              lambda: ops.decode_span_relations(f16.float(), p3, spans, score, count, w, b, clog,
                                                                check_pairs=False)], args.warmup, args.iters)
    print(json.dumps(dict(shape, what="decode_span_relations", bf16_ms=round(ms[0], 4), upcast_ms=round(ms[1], 4),
                          upcast_over_bf16=round(ms[1] / ms[0], 3),
                          bf16_workspace_bytes=int(lib.tspn_decode_span_relations_bf16_workspace_bytes(1, N, T, D, P, J, K, 20)),
                          upcast_workspace_bytes=int(lib.tspn_decode_span_relations_workspace_bytes(1, N, T, D, P, J, K, 20)),
                          clock_mhz=mhz)),
          flush=True)


if __name__ == "__main__":
    main()
