"""Relation detection evaluation, the parts that need no GPU: the host metric stage against the reference's own
numbers (golden g12), validation and exception types, the annotation reader, the packing layout the kernels read,
and the discipline of csrc/eval/ (kernel variant table, ISA store lint, no probe blocks, no environment reads)."""
import ast
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import cases_eval
import eval_kernel_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_EVAL = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc", "eval")


def _evaluation():
    import tspn_mi355x
    return tspn_mi355x.evaluation


def assert_same(got, want):
    assert type(got) is type(want) and got == want, (got, type(got), want, type(want))


def test_host_metrics_from_golden_hits_equal_the_reference():
    """_prepare's score order + the golden hit flags -> prec / rec / hit_scores / AP per video, tagging precision, and
    mAP / Recall@N / Precision@N, each equal to the reference's to the bit and with its dtype."""
    E = _evaluation()
    g = cases.load("g12_evaluation.npz")
    gt, pred, _ = cases_eval.g12_case()
    videos = E._prepare(gt, pred)
    assert [v["vid"] for v in videos] == list(g["vids"])
    for v in videos:
        hs = g[f"{v['vid']}/hit_scores"]
        v["hit"] = np.isfinite(hs)
        prec, rec, hit_scores = E._detection_scores(v["n_gt"], v["scores"], v["hit"])
        for got, want in ((prec, g[f"{v['vid']}/prec"]), (rec, g[f"{v['vid']}/rec"]), (hit_scores, hs)):
            assert got.dtype == want.dtype and np.array_equal(got, want), v["vid"]
        assert_same(E.voc_ap(rec, prec), g[f"{v['vid']}/ap"][()])
        tp = E._tagging_prec(v["gt_keys"], v["pred_keys"])
        assert tp.dtype == g[f"{v['vid']}/tag_prec"].dtype and np.array_equal(tp, g[f"{v['vid']}/tag_prec"])
    mean_ap, rec_at_n, mprec_at_n, _ = E._aggregate(videos, (50, 100, 1000), (1, 5, 10))
    assert_same(mean_ap, g["mean_ap"][()])
    for k in (50, 100, 1000):
        assert_same(rec_at_n[k], g[f"rec_at_{k}"][()])
    for k in (1, 5, 10):
        assert_same(mprec_at_n[k], g[f"mprec_at_{k}"][()])


def test_score_order_is_the_stable_descending_sort():
    E = _evaluation()
    gt, pred, _ = cases_eval.g12_case()
    for v in E._prepare(gt, pred):
        scores = [r["score"] for r in pred[v["vid"]]]
        assert v["order"].tolist() == sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)


def test_packing_layout():
    """Every packed trajectory lies inside `boxes` with end - begin rows; groups, candidate offsets and the
    prediction / ground-truth ranges tile the chunk; chunks split by video and respect max_candidates."""
    E = _evaluation()
    gt, pred, _ = cases_eval.g12_case()
    videos = E._prepare(gt, pred)
    pk = E._pack(videos)
    traj, groups, boxes = pk["traj"], pk["groups"], pk["boxes"]
    n_rel = traj.shape[0] // 2
    assert boxes.dtype == np.float64 and boxes.shape[1] == 4 and traj.shape[0] % 2 == 0
    assert (traj[:, 0] + traj[:, 2] - traj[:, 1] <= boxes.shape[0]).all() and (traj[:, 2] >= traj[:, 1]).all()
    assert np.array_equal(traj[1:, 0], traj[:-1, 0] + traj[:-1, 2] - traj[:-1, 1])
    assert np.array_equal(groups[:, 0], np.concatenate(([0], np.cumsum(groups[:-1, 1]))))
    assert np.array_equal(groups[:, 2], pk["n_pred"] + np.concatenate(([0], np.cumsum(groups[:-1, 3]))))
    assert np.array_equal(groups[:, 4], np.concatenate(([0], np.cumsum(groups[:-1, 1] * groups[:-1, 3]))))
    assert groups[:, 1].sum() == pk["n_pred"] and pk["n_pred"] + groups[:, 3].sum() == n_rel
    assert pk["candidates"] == int((groups[:, 1] * groups[:, 3]).sum()) and pk["max_group_gt"] == groups[:, 3].max()
    assert np.array_equal(pk["pred_group"], np.repeat(np.arange(len(groups)), groups[:, 1]))
    assert pk["max_group_gt"] > 64
    runs = list(E._chunks(videos, 50))
    assert [v["vid"] for r in runs for v in r] == [v["vid"] for v in videos] and len(runs) >= 4
    assert all(len(r) == 1 or sum(v["candidates"] for v in r) <= 50 for r in runs)


def test_chunks_stay_within_the_byte_budget():
    """The per-video cost _prepare predicts is what _pack produces (boxes included), and every chunk of more than one
    video stays within max_bytes, however loose max_candidates is; the results do not depend on the chunking."""
    E = _evaluation()
    gt, pred, _ = cases_eval.g12_case()
    videos = E._prepare(gt, pred)
    for v in videos:
        if v["groups"]:
            pk = E._pack([v])
            assert E._packed_bytes(pk) == v["bytes"] and pk["boxes"].nbytes == 32 * pk["rows"]
    sizes = sorted(v["bytes"] for v in videos if v["groups"])
    budget = sizes[-1] + sizes[0]                   # room for the largest video, or for a few small ones together
    runs = list(E._chunks(videos, 1 << 40, budget))
    assert [v["vid"] for r in runs for v in r] == [v["vid"] for v in videos]
    assert any(len(r) > 1 for r in runs) and len(runs) > 1
    for r in runs:
        pk = E._pack(r)
        assert len(r) == 1 or E._packed_bytes(pk) <= budget
        assert pk["boxes"].nbytes <= budget or len(r) == 1
    # one video over the budget still forms a chunk of its own
    assert [len(r) for r in E._chunks(videos, 1 << 40, 1)] == [1] * len(videos)
    assert E.DEFAULT_MAX_BYTES == 1 << 30


def test_validation_errors_and_exception_types():
    E = _evaluation()
    gt, pred, _ = cases_eval.g12_case()
    with pytest.raises(KeyError):                       # as the reference's prediction[vid]
        E.evaluate(gt, {k: v for k, v in pred.items() if k != "v_int"})
    with pytest.raises(IndexError):                     # as the reference's rec[-1]: no prediction anywhere
        E.evaluate(gt, {vid: [] for vid in gt})
    bad = json.loads(json.dumps(pred))
    bad["v_str"][5]["score"] = float("inf")
    with pytest.raises(ValueError, match="'v_str', prediction 5: non-finite score"):
        E.evaluate(gt, bad)
    bad = json.loads(json.dumps(pred))
    bad["v_edges"][0]["obj_traj"][1][2] = float("nan")
    with pytest.raises(ValueError, match="'v_edges', prediction 0: non-finite box in its obj_traj"):
        E.evaluate(gt, bad)
    bad = json.loads(json.dumps(pred))
    bad["v_edges"][1]["sub_traj"].pop()
    with pytest.raises(ValueError, match="'v_edges', prediction 1: sub_traj has 2 boxes for the duration"):
        E.evaluate(gt, bad)
    bad_gt = json.loads(json.dumps(gt))
    bad_gt["v_edges"][2]["obj_traj"][0] = [1, 2, 3]
    with pytest.raises(ValueError, match="'v_edges', ground truth 2: obj_traj must be a list of 4-coordinate"):
        E.evaluate(bad_gt, pred)
    with pytest.raises(ValueError, match="max_candidates and max_bytes"):
        E.evaluate(gt, pred, max_candidates=0)
    with pytest.raises(ValueError, match="max_candidates and max_bytes"):
        E.evaluate(gt, pred, max_bytes=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.evaluate(gt, pred, device="cpu")


def test_ops_refuse_cpu_tensors():
    import torch
    import tspn_mi355x
    boxes = torch.zeros((4, 4), dtype=torch.float64)
    traj = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn_mi355x.ops.eval_traj_volume(boxes, traj)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn_mi355x.ops.eval_greedy_match(torch.zeros(1, dtype=torch.float64), torch.zeros((1, 5), dtype=torch.int64),
                                          1, 0.5, 1)


def test_annotation_reader_equals_the_reference():
    E = _evaluation()
    g = cases.load("g12_evaluation.npz")
    anno = cases_eval.g12_annotation()
    assert json.dumps(E.relation_instances(anno)) == str(g["anno/relation_insts_json"])
    assert json.dumps(sorted(E.triplets([anno]))) == str(g["anno/triplets_json"])
    assert E.triplets({"anno0": anno}) == E.triplets([anno])


def test_load_prediction(tmp_path):
    E = _evaluation()
    _, pred, _ = cases_eval.g12_case()
    path = tmp_path / "pred.json"
    path.write_text(json.dumps({"version": "VERSION 1.0", "results": pred}))
    assert E.load_prediction(str(path)) == json.loads(json.dumps(pred))


# ---------------------------------------------------------------------------------------------------- csrc/eval/
def eval_global_kernels():
    """Names of every `__global__` function defined in csrc/eval/*.hip (the parse of test_kernel_variant_table.py)."""
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC_EVAL, "*.hip"))):
        src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b__global__\b", src):
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_eval_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = eval_global_kernels()
    assert in_source == {r["kernel"] for r in eval_kernel_variants.VARIANTS} and len(in_source) == 3
    seen = set()
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    for r in eval_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"


def test_eval_sources_pass_the_store_lint_and_carry_no_probe_blocks():
    import shutil
    files = sorted(glob.glob(os.path.join(CSRC_EVAL, "*.hip")) + glob.glob(os.path.join(CSRC_EVAL, "*.h")))
    assert files
    for f in files:
        assert "getenv" not in open(f).read(), f"{f} reads the environment"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + files,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available: nothing to compile to ISA")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] +
                         [f for f in files if f.endswith(".hip")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert "tspn_eval.hip" in res.stdout
