#!/usr/bin/env python3
"""Generate tests/golden/g12_evaluation.npz from the REFERENCE's own relation evaluation.

Runs only on a host that has the reference checkout (TSPN_REFERENCE, default /root/reference); the GPU side never
reads it.  Inputs come from tests/golden/cases_eval.py (hash RNG), so only the reference's OUTPUTS are stored.

What is run from the reference:
    lib.evaluation.visual_relation_detection   eval_detection_scores, eval_tagging_scores, evaluate
    lib/dataset/dataset.py                     Dataset.get_relation_insts, Dataset.get_triplets (loaded from its file,
                                               on an object that only supplies get_anno / get_index)
and the zero-shot filtering of evaluate.py:24-55, restated around the reference's `evaluate` (that function is tied
to a loaded dataset).  IPython, imported but unused by visual_relation_detection.py, gets an empty stand-in module.

Usage:  python tests/golden/make_golden_eval.py
"""
import contextlib
import importlib.util
import io
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

import cases_eval  # noqa: E402

if "IPython" not in sys.modules:
    _m = types.ModuleType("IPython")
    _m.embed = lambda *a, **k: None
    sys.modules["IPython"] = _m

from lib.evaluation import visual_relation_detection as vrd  # noqa: E402


def _ref_dataset_module():
    spec = importlib.util.spec_from_file_location("_ref_dataset", os.path.join(REF, "lib", "dataset", "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def zeroshot(gt, pred, train, old):
    """evaluate.py:30-55 with the split's triplets taken from `gt` (= dataset.get_triplets(split))."""
    split = set(tuple(r["triplet"]) for rels in gt.values() for r in rels)
    zs_triplets = split.difference(set(tuple(t) for t in train))
    zgt, zpred = dict(), dict()
    for vid, rels in gt.items():
        zs = [r for r in rels if tuple(r["triplet"]) in zs_triplets]
        if len(zs) > 0:
            zgt[vid] = zs
            zpred[vid] = pred[vid] if old else [r for r in pred[vid] if tuple(r["triplet"]) in zs_triplets]
    return vrd.evaluate(zgt, zpred)


def aggregates(prefix, res, out):
    mean_ap, rec_at_n, mprec_at_n = res
    out[prefix + "mean_ap"] = np.asarray(mean_ap)
    for k, v in rec_at_n.items():
        out[f"{prefix}rec_at_{k}"] = np.asarray(v)
    for k, v in mprec_at_n.items():
        out[f"{prefix}mprec_at_{k}"] = np.asarray(v)


def main():
    gt, pred, train = cases_eval.g12_case()
    out = {"vids": np.array([v for v, r in gt.items() if len(r) > 0])}
    for vid, rels in gt.items():
        if len(rels) == 0:
            continue
        prec, rec, hit_scores = vrd.eval_detection_scores(rels, pred[vid], 0.5)
        out[f"{vid}/prec"], out[f"{vid}/rec"], out[f"{vid}/hit_scores"] = prec, rec, hit_scores
        out[f"{vid}/ap"] = np.asarray(vrd.voc_ap(rec, prec))
        tprec, _, _ = vrd.eval_tagging_scores(rels, pred[vid])
        out[f"{vid}/tag_prec"] = tprec
    with contextlib.redirect_stdout(io.StringIO()):
        aggregates("", vrd.evaluate(gt, pred), out)
        aggregates("thr07/", vrd.evaluate(gt, pred, viou_threshold=0.7), out)
        aggregates("zs_new/", zeroshot(gt, pred, train, old=False), out)
        aggregates("zs_old/", zeroshot(gt, pred, train, old=True), out)

    ds = _ref_dataset_module().Dataset.__new__(_ref_dataset_module().Dataset)
    anno = cases_eval.g12_annotation()
    ds.get_anno = lambda vid: anno
    ds.split_index = {"val": [anno["video_id"]]}
    insts = ds.get_relation_insts(anno["video_id"])
    out["anno/relation_insts_json"] = np.array(json.dumps(insts))
    out["anno/triplets_json"] = np.array(json.dumps(sorted(ds.get_triplets("val"))))

    path = os.path.join(HERE, "g12_evaluation.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
