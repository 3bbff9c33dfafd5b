#!/usr/bin/env python3
"""Generate tests/golden/g13_detection_eval.npz from the REFERENCE's own object and action detection evaluation.

Runs only on a host that has the reference checkout (TSPN_REFERENCE, default /root/reference); the GPU side never
reads it.  Inputs come from tests/golden/cases_detection_eval.py (hash RNG), so only the reference's OUTPUTS are stored.

What is run from the reference:
    lib.evaluation.video_object_detection   evaluate, trajectory_overlap
    lib.evaluation.action_detection         evaluate, compute_detection_scores_per_class
    lib/dataset/dataset.py                  Dataset.get_object_insts, Dataset.get_action_insts (loaded from its file, on
                                            an object that only supplies get_anno and the action predicate list)
IPython, imported but unused by the package's relation module, gets an empty stand-in module.

Stored per configuration: mean_ap and the class APs in sorted category order, each with a flag that tells a numpy scalar
from a Python float (the reference returns either); for the object set, (max_overlap, max_index) of every prediction of
a ground-truth class in `prediction` order; for the action set, (prec, rec, hit_scores) of every predicted class.

Usage:  python tests/golden/make_golden_detection_eval.py
"""
import contextlib
import importlib.util
import io
import itertools
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TSPN_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import cases_detection_eval as cde  # noqa: E402

if "IPython" not in sys.modules:
    _m = types.ModuleType("IPython")
    _m.embed = lambda *a, **k: None
    sys.modules["IPython"] = _m

from lib.evaluation import action_detection as act  # noqa: E402
from lib.evaluation import video_object_detection as vod  # noqa: E402

OBJECT_CONFIGS = [(True, 0.5), (True, 0.3), (False, 0.5), (False, 0.3)]
ACTION_THRESHOLDS = (0.5, 0.7)


def _ref_dataset_module():
    spec = importlib.util.spec_from_file_location("_ref_dataset", os.path.join(REF, "lib", "dataset", "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def store_ap(prefix, mean_ap, ap_items, out):
    out[prefix + "mean_ap"] = np.asarray(mean_ap, dtype=np.float64)
    out[prefix + "mean_ap_is_np"] = np.asarray(isinstance(mean_ap, np.floating))
    out[prefix + "categories"] = np.array([c for c, _ in ap_items])
    out[prefix + "ap"] = np.array([ap for _, ap in ap_items], dtype=np.float64)
    out[prefix + "ap_is_np"] = np.array([isinstance(ap, np.floating) for _, ap in ap_items])


def main():
    out = {}
    gt, pred = cde.g13_object_case()
    gt_classes = set(t["category"] for tracks in gt.values() for t in tracks)
    with contextlib.redirect_stdout(io.StringIO()):
        for m07, thr in OBJECT_CONFIGS:
            mean_ap, ap_class = vod.evaluate(gt, pred, use_07_metric=m07, thresh_t=thr)
            store_ap(f"obj/{'07' if m07 else 'voc'}_{thr}/", mean_ap, ap_class, out)
    overlap, index = [], []
    for vid, tracks in pred.items():
        for t in tracks:
            if t["category"] in gt_classes:
                trajs = [g["trajectory"] for g in gt[vid] if g["category"] == t["category"]]
                mo, mi = vod.trajectory_overlap(trajs, t["trajectory"])
                overlap.append(float(mo))
                index.append(mi)
    out["obj/max_overlap"] = np.array(overlap, dtype=np.float64)
    out["obj/max_index"] = np.array(index, dtype=np.int64)

    gt, pred = cde.g13_action_case()
    for thr in ACTION_THRESHOLDS:
        with contextlib.redirect_stdout(io.StringIO()):
            mean_ap, ap_class = act.evaluate(gt, pred, viou_threshold=thr)
        # the reference averages the class APs in the iteration order of a set of strings, which changes from process
        # to process: the case must not depend on it
        means = set(float(np.mean(list(p))) for p in itertools.permutations(ap_class.values()))
        assert len(means) == 1, f"the action mean AP depends on the order of the classes: {sorted(means)}"
        store_ap(f"act/{thr}/", mean_ap, sorted(ap_class.items()), out)
        for c in sorted(ap_class):
            preds = [dict(id=vid, score=t["score"], duration=t["duration"], trajectory=t["trajectory"])
                     for vid, tracks in pred.items() for t in tracks if t["category"] == c]
            if not preds:
                continue
            gts = [dict(id=vid, duration=t["duration"], trajectory=t["trajectory"])
                   for vid, tracks in gt.items() for t in tracks if t["category"] == c]
            prec, rec, hit_scores = act.compute_detection_scores_per_class(gts, preds, thr)
            out[f"act/{thr}/{c}/prec"], out[f"act/{thr}/{c}/rec"], out[f"act/{thr}/{c}/hit_scores"] = prec, rec, hit_scores

    mod = _ref_dataset_module()
    ds = mod.Dataset.__new__(mod.Dataset)
    anno = cde.g13_annotation()
    ds.get_anno = lambda vid: anno
    ds._get_action_predicates = lambda: list(cde.ACTION_PREDICATES)
    out["anno/object_insts_json"] = np.array(json.dumps(ds.get_object_insts(anno["video_id"])))
    out["anno/action_insts_json"] = np.array(json.dumps(ds.get_action_insts(anno["video_id"])))

    path = os.path.join(HERE, "g13_detection_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
