#!/usr/bin/env python3
"""Time the per-frame detector's stages behind the backbone on a 720p-sized res4 map and print one JSON line.

The input is a seeded random res4 map [frames, 45, 80, 1024] (a 720 x 1280 frame at stride 16), bf16 unless --fp32, and a
`FasterRCNNC4` with seeded random head weights: nothing is loaded, so the boxes are random ones -- NMS suppresses few of
them, which is the long case for its scan.  Per stage, HIP events around --repeat runs after one warm-up, reported in ms
per frame:
    rpn_head_ms        the RPN head's 3x3 conv + ReLU and the fused 1x1 heads (ops.conv2d_nhwc / conv2d_nhwc_bf16)
    rpn_proposals_ms   ops.rpn_proposals at --pre / --post (6000 / 1000): selection, decode, NMS, gather
    res5_predictor_ms  Res5RoIHead on the proposals and the box predictor's GEMM
    box_detections_ms  ops.box_detections: softmax + class boxes, NMS per (frame, class), the final top-k
The events bracket device work only; the host prepares nothing between them but the launches.  The job may use 16 CPUs;
the host side is single-threaded Python.

    python tools/bench_detector.py [--frames 8] [--repeat 3] [--fp32] [--pre 6000] [--post 1000] [--depth 101]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tspn_mi355x as tspn  # noqa: E402


def clocks():
    """The card's clock state as rocm-smi prints it (read only), or None where the tool is missing."""
    try:
        res = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--json"], stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL, text=True, timeout=60)
        return json.loads(res.stdout).get("card0") if res.returncode == 0 else None
    except (OSError, ValueError, subprocess.TimeoutExpired):
        return None


def main():
    ap = argparse.ArgumentParser(description="Time the detector's post-backbone stages on a 45 x 80 x 1024 res4 map; the job "
                                             "may use 16 CPUs (the host side is single-threaded).")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--pre", type=int, default=6000)
    ap.add_argument("--post", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=101)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector needs a HIP device: the numbers are kernel times")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = tspn.FasterRCNNC4(depth=args.depth, pre_nms_topk=args.pre, post_nms_topk=args.post, frame_chunk=args.frames)
    # seeded heads with some spread: logits of O(1), deltas of a few tenths, class scores that pass the 0.05 threshold
    head, pred = model.proposal_generator.rpn_head, model.roi_heads.box_predictor
    with torch.no_grad():
        head.objectness_logits.weight.normal_(std=0.03)
        head.anchor_deltas.weight.normal_(std=0.01)
        pred.cls_score.weight.normal_(std=0.05)
        pred.bbox_pred.weight.normal_(std=0.02)
    model = model.to(dev).eval()
    T, H, W, C = args.frames, 45, 80, 1024
    maps = torch.rand((T, H, W, C), device=dev)
    maps = maps if args.fp32 else maps.to(torch.bfloat16)
    sizes = torch.tensor([[720.0, 1280.0]] * T, device=dev)
    cell = model.cell_anchors.to(dev)
    roi = model.roi_heads
    state = {}

    def rpn_head():
        state["logits"], state["deltas"] = head(maps)

    def rpn_proposals():
        state["props"], _, state["count"] = tspn.ops.rpn_proposals(state["logits"], state["deltas"], cell, 16, sizes, args.pre,
                                                                   args.post, model.rpn_nms_thresh, model.min_box_size)

    def res5_predictor():
        feats = roi(maps, state["props"].permute(1, 0, 2).contiguous()).permute(1, 0, 2).float().contiguous()
        both = [pred(feats[i]) for i in range(T)]
        state["cls"], state["dl"] = torch.cat([b[0] for b in both]), torch.cat([b[1] for b in both])

    def box_detections():
        state["out"] = tspn.ops.box_detections(state["cls"], state["dl"], state["props"], state["count"], sizes,
                                               model.score_thresh, model.nms_thresh, model.detections_per_image)

    out = {"workload": "detector", "frames": T, "map": [H, W, C], "dtype": "fp32" if args.fp32 else "bf16",
           "pre_nms_topk": args.pre, "post_nms_topk": args.post, "classes": pred.num_classes, "repeat": args.repeat,
           "cpu_count": os.cpu_count(), "omp_threads": os.environ.get("OMP_NUM_THREADS"), "clocks_before": clocks()}
    total = 0.0
    for name, fn in (("rpn_head_ms", rpn_head), ("rpn_proposals_ms", rpn_proposals), ("res5_predictor_ms", res5_predictor),
                     ("box_detections_ms", box_detections)):
        fn()                                     # warm-up: code objects, packed weights, the allocator
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / T)
        out[name] = round(min(times), 4)
        out[name[:-3] + "_runs_ms"] = [round(t, 4) for t in times]
        total += min(times)
    out["post_backbone_ms_per_frame"] = round(total, 4)
    out["proposals_per_frame"] = [int(v) for v in state["count"].tolist()]
    out["detections_per_frame"] = [int(v) for v in state["out"][3].tolist()]
    out["clocks_after"] = clocks()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
