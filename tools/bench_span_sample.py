#!/usr/bin/env python3
"""Time the span anchor sampler (`ops.span_anchor_sample`: tspn_span_anchor_sample) against the torch composition of
sampler.py (`nonzero` + `randperm` + scatter per class) on the same device labels, and one training step of the span-loss
model test's shape with sampling on against the same step with sampling off.  Prints one JSON line.

Default shape: one cfg2 segment, P = 992 pairs, A = 4, T = 150 (n = 595 200 anchors), labels from `ops.span_anchor_labels`
on the ground truth of tests/span_loss_reference.make_gt, batch 256, half positive, 32-bit keys.  Before anything is timed
the entry's mask is compared with the numpy restatement (tests/span_sample_reference.py) and the composition's class counts
with the quota rule.  The two paths alternate inside one process, --repeat rounds after --warmup unmeasured ones; a round
of a path is --inner calls between two HIP events, and the figures are per call: median [min, max] in ms.  `host_ms` is the
wall time the host spends issuing those calls without waiting for the device: a path that synchronises cannot issue faster
than the device runs.  `torch_syncs` counts the synchronising torch calls of one call of each path
(torch.cuda.set_sync_debug_mode).  The training steps (forward, backward, no optimiser) alternate the same way.

    python tools/bench_span_sample.py [--P 992 --A 4 --T 150 --G 3] [--batch 256] [--repeat 20] [--warmup 3] [--inner 20]
    python tools/bench_span_sample.py --entry-only 50        (50 calls of the entry and nothing else: for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, inner):
    """(device ms per call, host ms per call spent issuing)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, host / inner


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _alternate(paths, warmup, repeat, inner):
    dev, host = {k: [] for k in paths}, {k: [] for k in paths}
    for r in range(warmup + repeat):
        for k, fn in paths.items():                     # alternating: one round of each path per repeat
            d, h = _timed(fn, inner)
            if r >= warmup:
                dev[k].append(d)
                host[k].append(h)
    return {k: {"device_ms": _stats(dev[k]), "host_ms": _stats(host[k])} for k in paths}


def _torch_syncs(fn):
    """Synchronising torch calls of one fn()."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def train_steps(tspn, dev, batch):
    """(step with sampling on, step with sampling off): the two segments of the span-loss model test (N = 5 and 6 tracklets,
    T = 30, D = 16, G = 3), forward + backward."""
    import oracle  # noqa: F401  (the tests' helpers import it)
    import span_loss_reference as loss_ref

    def build(batch_size):
        cfg = tspn.default_cfg()
        cfg.RELPN.USE_PPN = False
        cfg.RELPN.DPN.IN_CHANNELS = 32
        cfg.PREDICT.FEATURE_DIM = 32
        cfg.RELPN.DPN.SPAN_LOSS.BATCH_SIZE_PER_SEGMENT = batch_size
        torch.manual_seed(3)
        return tspn.BaseModel(cfg).to(dev).train()

    plists, tlists = [], []
    for i, N in enumerate((5, 6)):
        v = tspn.synth.make_video(95 + i, N, 30, 16)
        P = N * (N - 1)
        plists.append(tspn.PairList.from_tracklets(torch.from_numpy(v["tracklet_feats"])).to(dev))
        tl = tspn.TargetList(torch.from_numpy((tspn.hashrng.uniform(96 + i, "tg", (P, 132)) < 0.05).astype(np.float32)))
        tl.add_field("spans", torch.from_numpy(loss_ref.make_gt(70 + i, P, 3, 30)))
        tlists.append(tl.to(dev))

    def step(model):
        def run():
            model.zero_grad(set_to_none=True)
            sum(model(plists, tlists).values()).backward()
        return run
    return step(build(batch)), step(build(0))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("P", 992), ("A", 4), ("T", 150), ("G", 3), ("batch", 256), ("key-bits", 32), ("repeat", 20),
                          ("warmup", 3), ("inner", 20), ("train-repeat", 20), ("entry-only", 0)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import span_loss_reference as loss_ref
    import span_sample_reference as ref
    import tspn_mi355x as tspn
    from tspn_mi355x.sampler import BalancedPositiveNegativePairSampler
    if not torch.cuda.is_available():
        raise SystemExit("bench_span_sample: needs a HIP device (there is nothing to time on a CPU)")
    ops, dev = tspn.ops, torch.device("cuda", 0)
    P, A, T, G = a.P, a.A, a.T, a.G
    sizes = [(i + 1) * float(T) / A for i in range(A)]
    gt = torch.from_numpy(loss_ref.make_gt(11, P, G, T)).to(dev)
    label, _ = ops.span_anchor_labels(gt, sizes, T, loss_ref.POS_IOU, loss_ref.NEG_IOU)
    seed, tag = 0, "span_sample/0"
    key = tspn.hashrng.stream_key(seed, tag)

    def entry():
        return ops.span_anchor_sample(label, a.batch, 0.5, key, a.key_bits)

    if a.entry_only:
        for _ in range(a.entry_only):
            entry()
        torch.cuda.synchronize()
        print(json.dumps({"entry_calls": a.entry_only, "n": label.numel(), "key_bits": a.key_bits}))
        return

    host_sampler = BalancedPositiveNegativePairSampler(a.batch, 0.5)
    flat = label.reshape(-1)

    def composition():
        pos, neg = host_sampler([flat])
        return pos[0] | neg[0]

    mask, counts = entry()
    want_mask, want_counts, _ = ref.sample_ref(label.cpu().numpy(), seed, tag, a.key_bits, a.batch, a.batch // 2)
    assert np.array_equal(mask.cpu().numpy(), want_mask) and counts.cpu().tolist() == want_counts.tolist(), "the entry is wrong"
    m = composition()
    assert int(m[flat >= 1].sum()) == want_counts[2] and int(m[flat == 0].sum()) == want_counts[3], "the composition is wrong"
    res = {"shape": {"P": P, "A": A, "T": T, "G": G, "n": label.numel()}, "batch": a.batch, "key_bits": a.key_bits,
           "counts": want_counts.tolist(), "launches_per_call": 2 * ref.rounds_of(a.key_bits) + 2,
           "repeat": a.repeat, "warmup": a.warmup, "inner": a.inner,
           "per_call": _alternate({"entry": entry, "composition": composition}, a.warmup, a.repeat, a.inner),
           "torch_syncs_per_call": {"entry": _torch_syncs(entry), "composition": _torch_syncs(composition)}}
    res["composition_over_entry"] = round(res["per_call"]["composition"]["device_ms"]["median"] /
                                          res["per_call"]["entry"]["device_ms"]["median"], 2)
    if a.train_repeat > 0:
        on, off = train_steps(tspn, dev, 64)
        on(), off()
        res["train_step"] = {"segments": "N = 5 and 6, T = 30, D = 16, G = 3", "batch": 64, "repeat": a.train_repeat,
                             "per_step": _alternate({"sampling_on": on, "sampling_off": off}, 3, a.train_repeat, 1),
                             "torch_syncs_per_step": {"sampling_on": _torch_syncs(on), "sampling_off": _torch_syncs(off)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
