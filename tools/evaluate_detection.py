#!/usr/bin/env python3
"""Video object detection or action detection evaluation of a prediction JSON against VidVRD / VidOR annotation files,
on the GPU: what the reference's evaluate.py --task object / --task action computes.

Prints one line per ground-truth category (sorted) and the mean AP.

    python tools/evaluate_detection.py --task object --prediction PRED.json --annotations DIR_OR_FILES... [--device cuda:0]
    python tools/evaluate_detection.py --task action --prediction PRED.json --annotations DIR_OR_FILES...
                                       --action-predicates FILE [--device cuda:0]
Annotation arguments are JSON files or directories searched recursively for *.json (one video per file).  The prediction
file is {"version": ..., "results": {video id: [...]}}.  --action-predicates names a file with the predicates that count
as actions: a JSON list, or one predicate per line.  --thresh-t / --viou-threshold and --voc (the non-07 AP for objects)
change the reference's defaults.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tspn_mi355x as tspn  # noqa: E402
from evaluate_relations import load_annotations  # noqa: E402


def load_predicates(path):
    text = open(path).read()
    try:
        names = json.loads(text)
    except ValueError:
        names = [line.strip() for line in text.splitlines()]
    if not isinstance(names, list) or not all(isinstance(n, str) for n in names):
        raise SystemExit(f"{path}: expected a JSON list of predicate names, or one name per line")
    return [n for n in names if n]


def report(mean_ap, ap_items):
    for i, (category, ap) in enumerate(ap_items):
        print("{:>2}{:>20}\t{:.4f}".format(i + 1, str(category), ap))
    print("{:>22}\t{:.4f}".format("mean AP", mean_ap))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--task", choices=("object", "action"), required=True)
    ap.add_argument("--prediction", required=True)
    ap.add_argument("--annotations", nargs="+", required=True)
    ap.add_argument("--action-predicates", default=None, help="file with the action predicates (--task action)")
    ap.add_argument("--thresh-t", type=float, default=0.5, help="tIoU threshold of a true positive (--task object)")
    ap.add_argument("--voc", action="store_true", help="the non-07 VOC AP for objects (the reference uses the 11-point form)")
    ap.add_argument("--viou-threshold", type=float, default=0.5, help="vIoU threshold of a hit (--task action)")
    ap.add_argument("--device", default=None)
    args = ap.parse_args()
    E = tspn.evaluation
    annos = load_annotations(args.annotations)
    prediction = E.load_prediction(args.prediction)
    if args.task == "object":
        groundtruth = {a["video_id"]: E.object_instances(a) for a in annos}
    else:
        if args.action_predicates is None:
            raise SystemExit("--task action needs --action-predicates FILE")
        predicates = load_predicates(args.action_predicates)
        groundtruth = {a["video_id"]: E.action_instances(a, predicates) for a in annos}
    print("Number of videos in ground truth: {}".format(len(groundtruth)))
    print("Number of videos in prediction: {}".format(len(prediction)))
    if args.task == "object":
        mean_ap, ap_class = E.evaluate_objects(groundtruth, prediction, use_07_metric=not args.voc,
                                               thresh_t=args.thresh_t, device=args.device)
        report(mean_ap, ap_class)
    else:
        mean_ap, ap_class = E.evaluate_actions(groundtruth, prediction, viou_threshold=args.viou_threshold,
                                               device=args.device)
        report(mean_ap, sorted(ap_class.items(), key=lambda kv: kv[0]))


if __name__ == "__main__":
    main()
