#!/usr/bin/env python3
"""Relation detection evaluation of a prediction JSON against VidVRD / VidOR annotation files, on the GPU.

Prints the seven lines of the reference's evaluate.py --task relation (mAP, Recall@50/100/1000, tagging
Precision@1/5/10), then the same for its zero-shot setting when --train annotations are given.

    python tools/evaluate_relations.py --prediction PRED.json --annotations DIR_OR_FILES... [--train DIR_OR_FILES...]
                                       [--old-zeroshot] [--device cuda:0]
Annotation arguments are JSON files or directories searched recursively for *.json (one video per file).
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tspn_mi355x as tspn  # noqa: E402


def annotation_files(args):
    out = []
    for a in args:
        out.extend(sorted(glob.glob(os.path.join(a, "**", "*.json"), recursive=True)) if os.path.isdir(a) else [a])
    return out


def load_annotations(args):
    annos = []
    for path in annotation_files(args):
        with open(path) as fh:
            annos.append(json.load(fh))
    return annos


def report(res):
    mean_ap, rec_at_n, mprec_at_n = res
    print("detection mean AP (used in challenge): {}".format(mean_ap))
    for n in (50, 100, 1000):
        print("detection recall@{}: {}".format(n, rec_at_n[n]))
    for n in (1, 5, 10):
        print("tagging precision@{}: {}".format(n, mprec_at_n[n]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--prediction", required=True)
    ap.add_argument("--annotations", nargs="+", required=True)
    ap.add_argument("--train", nargs="*", default=None, help="training annotations (zero-shot triplets)")
    ap.add_argument("--old-zeroshot", action="store_true")
    ap.add_argument("--device", default=None)
    args = ap.parse_args()
    E = tspn.evaluation
    annos = load_annotations(args.annotations)
    groundtruth = {a["video_id"]: E.relation_instances(a) for a in annos}
    prediction = E.load_prediction(args.prediction)
    print("Number of videos in ground truth: {}".format(len(groundtruth)))
    print("Number of videos in prediction: {}".format(len(prediction)))
    report(E.evaluate(groundtruth, prediction, device=args.device))
    if args.train is not None:
        print("-- zero-shot setting ({})".format("old" if args.old_zeroshot else "new"))
        train = E.triplets(load_annotations(args.train))
        report(E.evaluate_zeroshot(groundtruth, prediction, train, old=args.old_zeroshot, device=args.device))


if __name__ == "__main__":
    main()
