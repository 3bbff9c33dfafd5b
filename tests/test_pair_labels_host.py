"""Pair labels from ground-truth relation instances, the parts that need no GPU: the numpy restatement
(tests/pair_labels_reference.py) against an independent triple loop and against the reference's own statements once their
three crashing lines are given ints and tensors; the conditions the shared cases have to meet; the host helper
`dataset.segment_relation_instances`; the refusals of the C entry; and the discipline of csrc/pairlabels/ (kernel variant
table, built sources, no probe blocks, no memset, no environment reads, no spills)."""
import ast
import ctypes
import glob
import os
import re
import subprocess
import sys
from itertools import product

import numpy as np
import pytest
import torch

import oracle
import pair_labels_reference as ref
import pairlabels_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_PL = os.path.join(PKG, "csrc", "pairlabels")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_PL, "*.hip")) + glob.glob(os.path.join(CSRC_PL, "*.h")))
ENTRY = "tspn_pair_labels_f32"


# ------------------------------------------------------------------------------------------- the restatement
def brute_force(seg, K, G, thr, merge):
    """The frozen semantics as DESIGN.md §2 words them, pair by pair and instance by instance: no dict, no product."""
    trackid, iou, pairs, insts = seg["trackid"], seg["iou"], seg["pairs"], seg["insts"]
    fstart, fend = seg["frames"]
    M, P, R = len(trackid), len(pairs), len(insts)
    t = np.float32(thr)
    cols = np.full((R, 2), -1, np.int32)
    for r in range(R):
        if not 0 <= insts[r, 2] < K:
            cols[r] = -2
            continue
        for c in range(2):
            for j in range(M):
                if trackid[j] >= 0 and trackid[j] == insts[r, c]:
                    cols[r, c] = j
    labels = np.zeros((P, K), np.float32)
    spans = np.zeros((P, G, 2), np.int64)
    count = np.zeros(P, np.int32)
    for p in range(P):
        s, o = pairs[p]
        if not (0 <= s < M and 0 <= o < M):
            count[p] = -1
            continue
        if s == o or trackid[s] >= 0 or trackid[o] >= 0:
            continue
        for r in range(R):
            if cols[r, 0] < 0 or cols[r, 1] < 0:
                continue
            if not (iou[s, cols[r, 0]] >= t and iou[o, cols[r, 1]] >= t):
                continue
            if merge == "last":
                labels[p] = 0.0
            labels[p, insts[r, 2]] = 1.0
            lo, hi = max(insts[r, 3], fstart) - fstart, min(insts[r, 4], fend) - fstart
            if hi <= lo or any((spans[p, g] == (lo, hi)).all() for g in range(min(count[p], G))):
                continue
            if count[p] < G:
                spans[p, count[p]] = (lo, hi)
            count[p] = min(count[p] + 1, G + 1)
    if G == 0:
        count[:] = 0                                          # no span outputs: nothing to count
    return labels, spans, count, cols


@pytest.mark.parametrize("cid", ref.case_ids())
def test_restatement_equals_an_independent_triple_loop(cid):
    case = next(c for c in ref.cases() if c["id"] == cid)
    for seg in case["segments"]:
        got = ref.segment_ref(seg, case["K"], case["G"], case["thr"], case["merge"])
        want = brute_force(seg, case["K"], case["G"], case["thr"], case["merge"])
        for name, g, w in zip(("labels", "spans", "span_count", "inst_cols"), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (cid, name)


def reference_statements(pairs, iou, trackid, insts, K, iou_thres):
    """`_get_proposals_rel_feature` (vrdataset.py:85-138) in its own statement order, with the three lines that cannot run
    given what they need: `iou` as a float32 tensor (torch.where refuses numpy), the 0-d tensors of `product(...)` turned
    into ints before they key `pair_to_find`, and every label row a float32 tensor.  Returns the stacked rows in the
    reference's order (dict insertion: positives first) and that order as pair indices."""
    iou = torch.from_numpy(iou)
    pair_to_find = dict([((int(a), int(b)), find) for find, (a, b) in enumerate(pairs)])
    gt_tid_to_idx = dict([(int(tid), ind) for ind, tid in enumerate(trackid) if tid >= 0])
    pos_idx, pred_labels = [], {}
    for sub_tid, obj_tid, pred_idx in insts[:, :3].tolist():
        if sub_tid in gt_tid_to_idx and obj_tid in gt_tid_to_idx:
            overlap_tids1 = torch.where(iou[:, gt_tid_to_idx[sub_tid]] >= iou_thres)[0]
            overlap_tids2 = torch.where(iou[:, gt_tid_to_idx[obj_tid]] >= iou_thres)[0]
            for traj_idx1, traj_idx2 in product(overlap_tids1, overlap_tids2):
                traj_idx1, traj_idx2 = int(traj_idx1), int(traj_idx2)
                if traj_idx1 != traj_idx2 and trackid[traj_idx1] < 0 and trackid[traj_idx2] < 0:
                    pos_idx.append(pair_to_find[(traj_idx1, traj_idx2)])
                    row = torch.zeros(K)
                    row[pred_idx] = 1.0
                    pred_labels[pair_to_find[(traj_idx1, traj_idx2)]] = row
    neg_idx = [idx for idx in range(len(pairs)) if idx not in set(pos_idx)]
    pred_labels.update(dict([(i, torch.zeros(K)) for i in neg_idx]))
    return torch.stack(list(pred_labels.values())).numpy(), list(pred_labels.keys())


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_last_merge_in_insertion_order_equals_the_references_statements(thr):
    """The row-order decision: the restatement's "last" labels, permuted into the dict's insertion order, are what the
    reference's statements stack; in pair order they are not (the positives come first there)."""
    K = 132
    seg = ref.make_segment(11, 20, ref.GT4, 10, 40, K, thr)
    M = len(seg["trackid"])
    seg["pairs"] = np.array([(a, b) for a in range(M) for b in range(M) if a != b], np.int64)
    seg["insts"] = seg["insts"][(seg["insts"][:, 2] >= 0) & (seg["insts"][:, 2] < K)]      # to_multi_onehot has no range check
    rows, order = reference_statements(seg["pairs"], seg["iou"], seg["trackid"], seg["insts"], K, thr)
    labels = ref.segment_ref(seg, K, 0, thr, "last")[0]
    assert sorted(order) == list(range(len(seg["pairs"]))) and order != sorted(order)
    assert np.array_equal(labels[order], rows) and not np.array_equal(labels, rows)
    assert 0 < int(labels.sum()) < len(labels)


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_threshold_edges_by_hand(thr):
    """One instance 0 -> 1 (predicate 5): subject rows at fp32 thr and one ulp above are covered, one ulp below and NaN are
    not; the Python-float threshold is rounded to float32 first (0.7 rounds down: the double 0.7 is above float32(0.7))."""
    seg = ref.edge_segment(thr)
    col = seg["iou"][:4, 5]
    assert col[0] == np.float32(thr) and col[1] < col[0] < col[2] and np.isnan(col[3])
    assert np.nextafter(col[1], np.float32(1)) == col[0] and np.nextafter(col[0], np.float32(1)) == col[2]
    if thr == 0.7:
        assert float(col[0]) < 0.7                                  # a float64 comparison would refuse the edge row
    labels, spans, count, cols = ref.segment_ref(seg, 8, 2, thr, "last")
    assert cols.tolist() == [[5, 6]]
    for p, (s, o) in enumerate(seg["pairs"].tolist()):
        want = s in (0, 2) and o < 5 and o != s and seg["iou"][o, 6] >= np.float32(thr)
        assert labels[p].tolist() == [float(want and k == 5) for k in range(8)], (s, o)
        assert count[p] == int(want) and spans[p].tolist() == ([[0, 30], [0, 0]] if want else [[0, 0], [0, 0]])
    assert labels[:, 5].sum() >= 4


def test_shared_cases_meet_the_conditions_the_gpu_tests_rely_on():
    cs = ref.cases()
    assert len({c["id"] for c in cs}) == len(cs) and set(ref.SMALL_IDS) <= set(ref.case_ids())
    total = lambda c, key: sum(len(s[key]) for s in c["segments"])  # noqa: E731
    assert {1, 255, 256, 257, 2 * 256 + 3} <= {total(c, "pairs") for c in cs if c["single"]}
    assert {1, 63, 64, 65, 132, 512} <= {c["K"] for c in cs} and {0, 1, 70} <= {total(c, "insts") for c in cs}
    assert {1, 4, 16} <= {c["G"] for c in cs} and {1, 3} <= {len(c["segments"]) for c in cs}
    assert {0.5, 0.7} <= {c["thr"] for c in cs} and {"last", "or"} == {c["merge"] for c in cs}
    assert any(not c["single"] and len(c["segments"]) == 1 for c in cs)
    s3 = next(c for c in cs if c["id"] == "S3-last")
    assert [len(s["pairs"]) for s in s3["segments"]] == [300, 0, 100] and len(s3["segments"][2]["insts"]) == 0
    seen = set()
    for c in cs:
        labels, spans, count, cols = ref.case_ref(c)
        assert set(np.unique(labels).tolist()) <= {0.0, 1.0}
        if c["merge"] == "last":
            assert labels.sum(axis=1).max(initial=0) <= 1
        elif labels.size and labels.sum(axis=1).max() > 1:
            seen.add("multi-hot")
        if c["G"]:
            if (count == c["G"] + 1).any():
                seen.add(f"overflow G={c['G']}")
            if (count == -1).any():
                seen.add("out of range")
            if ((count > 0) & (count <= c["G"])).any():
                seen.add("spans")
        if (cols == -2).any():
            seen.add("pred out of range")
        if (cols == -1).any():
            seen.add("missing column")
        for s in c["segments"]:
            tid, ins = s["trackid"], s["insts"]
            dup = [t for t in set(tid[tid >= 0].tolist()) if (tid == t).sum() > 1]
            r = ref.segment_ref(s, c["K"], c["G"], c["thr"], c["merge"])
            for t in dup:                                           # the last column of a repeated id
                rows = np.flatnonzero((ins[:, 0] == t) & (r[3][:, 0] >= 0))
                if len(rows):
                    assert (r[3][rows, 0] == np.flatnonzero(tid == t)[-1]).all()
                    seen.add("duplicate id")
            live = (r[3] >= 0).all(axis=1)
            if (live & (ins[:, 0] == ins[:, 1])).any():
                seen.add("sub == obj")
            if (ins[:, :2] < 0).any():
                seen.add("negative id")
            if len(s["pairs"]) and (s["pairs"][:, 0] == s["pairs"][:, 1]).any():
                seen.add("s == o")
            if len(s["pairs"]) and len(tid) and (tid[np.clip(s["pairs"], 0, len(tid) - 1)] >= 0).any():
                seen.add("ground-truth pair")
            if np.isnan(s["iou"]).any():
                seen.add("nan")
            f0, f1 = s["frames"]
            b, e = ins[live, 3], ins[live, 4]
            seen |= {name for name, hit in (("clip start", (b < f0) & (e > f0) & (e < f1)), ("clip end", (b > f0) & (b < f1) & (e > f1)),
                                            ("clip both", (b < f0) & (e > f1)), ("empty", (e <= f0) | (b >= f1) | (e <= b)))
                     if hit.any()}
    want = {"multi-hot", "overflow G=1", "overflow G=4", "overflow G=16", "out of range", "spans", "pred out of range",
            "missing column", "duplicate id", "sub == obj", "negative id", "s == o", "ground-truth pair", "nan", "clip start",
            "clip end", "clip both", "empty"}
    assert seen == want, want ^ seen
    # a duplicated span is met by a pair and stored once
    dense = next(c for c in cs if c["id"] == "G16-dense-last")
    spans, count = ref.case_ref(dense)[1:3]
    full = np.flatnonzero(count == 17)[0]
    assert len({tuple(x) for x in spans[full].tolist()}) == 16


# ------------------------------------------------------------------------------------------- the host helper
def test_segment_relation_instances_in_its_three_modes():
    import tspn_mi355x
    sri, seg_video = tspn_mi355x.dataset.segment_relation_instances, tspn_mi355x.dataset.segment_video
    for a, b in ((0, 30), (0, 29), (10, 70), (0, 100), (7, 38), (5, 5)):
        assert seg_video(a, b) == oracle.segment_video(a, b)
    insts = np.array([[0, 1, 3, 10, 70], [1, 0, 7, 0, 31], [2, 2, 9, 50, 60], [0, 2, 1, 80, 120]], np.int64)
    train = sri(insts, "train")
    want = {}
    for row in insts:
        for seg in oracle.segment_video(int(row[3]), int(row[4])):
            want.setdefault(seg, []).append(row)
    assert set(train) == set(want) == {(10, 40), (25, 55), (40, 70), (0, 30), (80, 110)}
    assert all(v.dtype == np.int64 and v.shape[1] == 5 and np.array_equal(v, np.stack(want[k])) for k, v in train.items())
    assert list(train) == list(want)                                  # the reference's index order: first met, first listed
    test = sri(insts, "test", frame_count=100)
    assert list(test) == oracle.segment_video(0, 100) and all(np.array_equal(v, insts) for v in test.values())
    clip = sri(insts, "clip", frame_count=100)
    for seg in oracle.segment_video(0, 100):
        rows = insts[(insts[:, 3] < seg[1]) & (insts[:, 4] > seg[0])]
        assert np.array_equal(clip[seg], rows) and len(rows)
    assert clip[(0, 30)][:, 2].tolist() == [3, 7] and clip[(45, 75)][:, 2].tolist() == [3, 9]
    # has_segment stands for the feature-file check; an empty list gives no segment
    odd = sri(insts, "test", frame_count=100, has_segment=lambda a, b: a % 2 == 1)
    assert list(odd) == [(15, 45), (45, 75)]
    assert sri(np.zeros((0, 5), np.int64), "test", frame_count=100) == {} and sri(insts, "clip", frame_count=20) == {}
    with pytest.raises(ValueError, match="mode"):
        sri(insts, "val")
    with pytest.raises(ValueError, match="frame_count"):
        sri(insts, "clip")


# ------------------------------------------------------------------------------------------- the entry
def test_entry_point_is_declared_bound_exported_and_takes_no_workspace():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRY in abi.header_symbols() and ENTRY in abi.PROTOTYPES and hasattr(ctypes.CDLL(abi.LIB_PATH), ENTRY)
    assert "pair_labels" in tspn_mi355x.ops.__all__ and abi.lib().tspn_version() == 7
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\btspn_pair_labels_f32\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    assert "workspace" not in params and len(params.split(",")) == len(abi.PROTOTYPES[ENTRY][1]) == 22
    assert {"segment_relation_instances", "segment_video"} <= set(tspn_mi355x.dataset.__all__)


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any device work: the pointers are made-up addresses.  Return
    code and the whole message."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    vp = ctypes.c_void_p
    ok, odd4, odd2, null = vp(0x10000), vp(0x10004), vp(0x10002), vp(0)
    names = ("pairs", "pair_off", "trackid", "track_off", "iou", "iou_off", "insts", "inst_off", "seg_frames")

    def call(S=2, P=10, M=5, R=3, K=132, G=4, thr=0.5, merge=0, labels=ok, spans=ok, span_count=ok, inst_cols=ok, **ptr):
        args = [ptr.get(n, ok) for n in names]
        rc = lib.tspn_pair_labels_f32(*args, S, P, M, R, K, G, thr, merge, labels, spans, span_count, inst_cols, null)
        return rc, lib.tspn_last_error().decode()

    w = "tspn_pair_labels_f32: "
    assert call(P=-1) == (A_.TSPN_EINVAL, w + "bad sizes S=2 P=-1 M=5 R=3")
    assert call(S=-1)[0] == call(M=-1)[0] == call(R=-1)[0] == A_.TSPN_EINVAL
    assert call(P=2 ** 31) == (A_.TSPN_EUNSUPPORTED, w + "S=2 P=2147483648 M=5 R=3 (each needs < 2^31)")
    assert call(K=0) == (A_.TSPN_EINVAL, w + "K=0 predicates (needs K >= 1)")
    assert call(K=513) == (A_.TSPN_EUNSUPPORTED, w + "K=513 predicates (needs K <= 512)")
    assert call(G=-1) == (A_.TSPN_EINVAL, w + "G=-1 span rows (needs 0 <= G)")
    assert call(G=17) == (A_.TSPN_EUNSUPPORTED, w + "G=17 span rows (needs G <= 16)")
    assert call(spans=null) == call(span_count=null) == (A_.TSPN_EINVAL, w + "G=4 with a null spans or span_count")
    assert call(merge=2) == (A_.TSPN_EINVAL, w + "unknown merge=2 (0 = last, 1 = or)")
    assert call(merge=-1)[0] == A_.TSPN_EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(thr=bad) == (A_.TSPN_EINVAL, w + "iou_thres is not finite")
    msg = w + "S=2 needs pair_off, track_off, iou_off and inst_off (all null: one segment)"
    for n in ("pair_off", "track_off", "iou_off", "inst_off"):
        assert call(**{n: null}) == (A_.TSPN_EINVAL, msg)
    assert call(pair_off=null, track_off=null, iou_off=null, inst_off=null) == (A_.TSPN_EINVAL, msg)
    assert call(S=1, pair_off=null, track_off=null, iou_off=null) == (A_.TSPN_EINVAL, msg.replace("S=2", "S=1"))
    assert call(S=0) == (A_.TSPN_EINVAL, w + "S=0 with P=10 pairs and R=3 instances")
    for n in ("pairs", "trackid", "iou", "insts", "seg_frames"):
        assert call(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert call(labels=null) == call(inst_cols=null) == (A_.TSPN_EINVAL, w + "null pointer")
    msg = w + "unaligned pointer (int64 operands need 8 bytes, fp32 and int32 ones 4)"
    for n in ("pairs", "pair_off", "trackid", "track_off", "iou_off", "insts", "inst_off", "seg_frames"):
        assert call(**{n: odd4}) == (A_.TSPN_EUNSUPPORTED, msg), n
    assert call(spans=odd4) == call(iou=odd2) == call(labels=odd2) == call(span_count=odd2) == call(inst_cols=odd2) \
        == (A_.TSPN_EUNSUPPORTED, msg)
    # the order: sizes, K, G, merge, threshold, offsets, null pointers
    assert "bad sizes" in call(P=-1, K=0)[1] and "K=0" in call(K=0, G=17)[1] and "G=17" in call(G=17, merge=5)[1]
    assert "merge=5" in call(merge=5, thr=float("nan"))[1] and "not finite" in call(thr=float("nan"), pair_off=null)[1]
    # nothing to do is served without a device and without any pointer: no pairs and no instances
    nothing = {n: null for n in names}
    assert call(S=0, P=0, M=0, R=0, G=0, labels=null, spans=null, span_count=null, inst_cols=null, **nothing)[0] == A_.TSPN_OK
    assert call(S=1, P=0, M=7, R=0, G=0, labels=null, spans=null, span_count=null, inst_cols=null, **nothing)[0] == A_.TSPN_OK
    assert call(S=3, P=0, M=0, R=0)[0] == A_.TSPN_OK


def test_op_and_dataset_layer_refuse_cpu_tensors_and_wrong_operands():
    import tspn_mi355x
    ops, ds = tspn_mi355x.ops, tspn_mi355x.dataset
    pairs, tid = torch.zeros((3, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    iou, insts = torch.zeros((4, 4)), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_labels(pairs, tid, iou, insts, 132)
    with pytest.raises(TypeError):
        ops.pair_labels(pairs.numpy(), tid, iou, insts, 132)
    with pytest.raises(ValueError, match="not both"):
        ds._relation_instances(insts, None, 0, torch.zeros((3, 132)))
    with pytest.raises(ValueError, match=r"\[R,3\] or \[R,5\]"):
        ds._relation_instances(np.zeros((2, 4), np.int64), None, 0, None)
    with pytest.raises(ValueError, match="max_spans > 0 needs"):
        ds._relation_instances(np.zeros((2, 3), np.int64), (0, 30), 4, None)
    with pytest.raises(ValueError, match="max_spans > 0 needs"):
        ds._relation_instances(insts, None, 4, None)
    a, frames = ds._relation_instances(np.array([[0, 1, 5]]), None, 0, None)
    assert a.tolist() == [[0, 1, 5, 0, 0]] and a.dtype == np.int64 and frames.tolist() == [[0, 0]]
    assert ds._relation_instances(None, None, 0, None) == (None, None)


# ------------------------------------------------------------------------------------------- the sources
def test_pairlabels_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_PL, "*.hip"))))
    assert in_source == {r["kernel"] for r in pairlabels_kernel_variants.VARIANTS} and len(in_source) == 2
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in pairlabels_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] == ENTRY and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_PL]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "pairlabels_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    # the granularities the table and the case list speak of are the kernels'
    text = open(os.path.join(CSRC_PL, "tspn_pair_labels.hip")).read()
    consts = {m.group(1): m.group(2).strip() for m in re.finditer(r"constexpr int (\w+) = ([^;,]+)[;,]", text)}
    assert (consts["TILE"], consts["MAX_K"], consts["MAX_WORDS"], consts["MAX_G"]) == ("256", "512", "MAX_K / 64", "16")
    assert (ref.TILE, ref.MAX_K, ref.MAX_G) == (256, 512, 16)


def test_pairlabels_sources_are_built_and_carry_no_probe_blocks_memsets_atomics_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "getenv" not in text, f"{f} reads the environment"
        assert "hipMemset" not in text, f"{f}: the kernels write every output themselves"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert "asm" not in code and not re.search(r"[aA]tomic", code), f"{f}: neither inline assembly nor atomics"
        assert "workspace" not in code
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in pairlabels_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k + "(" in n for k in names)}
    assert len(found) == len(names)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
