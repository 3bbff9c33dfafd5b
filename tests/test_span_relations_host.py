"""Relations decoded with their temporal spans, the parts that need no GPU: the discipline of csrc/relations/ (kernel
variant table, no probe blocks, no environment reads), the composition helper against a brute-force float64
restatement, and span-bounded association (`greedy_relational_association` with 4-tuple predictions)."""
import ast
import copy
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import relations_kernel_variants
import span_relations_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc", "relations")


def _association():
    import tspn_mi355x
    return tspn_mi355x.association


# ------------------------------------------------------------------------------------------------ csrc/relations/
def relations_global_kernels():
    """Names of every `__global__` function defined in csrc/relations/*.hip (the parse of test_kernel_variant_table.py)."""
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC_REL, "*.hip"))):
        src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b__global__\b", src):
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_relations_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = relations_global_kernels()
    assert in_source == {r["kernel"] for r in relations_kernel_variants.VARIANTS} and len(in_source) == 2
    seen, defined = set(), {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    for r in relations_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"


def test_relations_sources_are_built_and_carry_no_probe_blocks():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tspn_build_rel", os.path.join(os.path.dirname(os.path.dirname(CSRC_REL)), "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    files = sorted(glob.glob(os.path.join(CSRC_REL, "*.hip")) + glob.glob(os.path.join(CSRC_REL, "*.h")))
    assert files and set(f for f in files if f.endswith(".hip")) <= set(build.sources())
    for f in files:
        assert "getenv" not in open(f).read(), f"{f} reads the environment"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + files,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_entry_points_are_declared_and_bound():
    import tspn_mi355x
    names = {"tspn_decode_span_relations_workspace_bytes", "tspn_decode_span_relations_f32"}
    assert names <= set(tspn_mi355x._abi.header_symbols()) and names <= set(tspn_mi355x._abi.PROTOTYPES)
    assert "decode_span_relations" in tspn_mi355x.ops.__all__


def test_ops_refuse_cpu_tensors():
    import tspn_mi355x
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn_mi355x.ops.decode_span_relations(z(2, 3, 4), z((1, 2, 2), dtype=torch.int64), z((2, 1, 2), dtype=torch.int64),
                                              z(2, 1), z(2, dtype=torch.int64), z(3, 8), None, z(1, 2, 5))


# --------------------------------------------------------------------------------------- the composition helper
def test_composition_equals_a_brute_force_per_frame_mean():
    """`compose` on q built in float64 from per-frame means + sigmoid, against a candidate-by-candidate Python loop:
    N=3, T=5, D=4, K=3, J=2, with an unused row, a (-1, -1) row inside the count, and an exact tie."""
    N, T, D, K, J, R, M = 3, 5, 4, 3, 2, 2, 7
    rng = np.random.RandomState(11)
    f = rng.uniform(-1, 1, (N, T, D))
    f[2] = f[0]                                                   # tracklets 0 and 2 alike: pairs (0,1) and (2,1) tie
    w, b = rng.uniform(-1, 1, (K, 2 * D)), rng.uniform(-0.2, 0.2, K)
    pairs = np.array([[0, 1], [1, 2], [2, 1], [1, 0]], dtype=np.int64)
    P = len(pairs)
    spans = np.array([[[0, 3], [2, 5]], [[1, 2], [-1, -1]], [[0, 3], [2, 5]], [[-1, -1], [4, 9]]], dtype=np.int64)
    score = np.array([[0.9, 0.5], [0.7, 0.0], [0.9, 0.5], [0.25, 0.75]], dtype=np.float32)
    count = np.array([2, 1, 2, 2], dtype=np.int64)
    cls = rng.uniform(-1, 1, (1, N, 6)).astype(np.float32)
    q = np.zeros((P, J, K), dtype=np.float32)
    for p in range(P):
        for j in range(J):
            a, e = oracle.span_frames(spans[p, j, 0], spans[p, j, 1], T)
            x = np.concatenate([f[pairs[p, 0], a:e].mean(axis=0), f[pairs[p, 1], a:e].mean(axis=0)])
            q[p, j] = (1.0 / (1.0 + np.exp(-(w @ x + b)))).astype(np.float32)
    t = torch.from_numpy
    got = ref.compose(t(q.reshape(P * J, K)), t(pairs[None]), t(spans), t(score), t(count), t(cls), R, M)[0]
    # brute force: every candidate, sorted by (-product, flat index)
    cands = []
    for p in range(P):
        for j in range(count[p]):
            ks = sorted(range(K), key=lambda k: (-q[p, j, k], k))[:R]
            for r, k in enumerate(ks):
                cands.append((-(q[p, j, k] * score[p, j]), (p * J + j) * R + r, p, j, k))
    cands.sort()
    assert len(cands) == 14 and got["valid"] == M
    labels = cls[0].argmax(axis=1)
    for m, (neg, _, p, j, k) in enumerate(cands[:M]):
        assert got["scores"][m] == -neg and got["scores"].dtype == np.float32
        assert got["triplets"][m].tolist() == [labels[pairs[p, 0]], k, labels[pairs[p, 1]]]
        assert got["pair_tids"][m].tolist() == pairs[p].tolist() and got["span_rank"][m] == j
        assert got["spans"][m].tolist() == spans[p, j].tolist()
    tie = [m for m in range(M) if got["pair_tids"][m].tolist() in ([0, 1], [2, 1])]
    assert len(tie) >= 2                                          # the tie is among the winners: lower flat index first
    few = ref.compose(t(q.reshape(P * J, K)), t(pairs[None]), t(spans), t(score), t(count), t(cls), R, 200)[0]
    assert few["valid"] == 14 and len(few["scores"]) == 14


# ------------------------------------------------------------------------------------------ span-bounded association
def _boxes(n, length, shift=0.0):
    """[n, length, 4]: tracklet i sits at x = 100 i (+ shift), the same box in every frame."""
    b = np.zeros((n, length, 4))
    for i in range(n):
        b[i] = (100.0 * i + shift, 10.0, 100.0 * i + 60.0 + shift, 80.0)
    return b


TRIP = (3, 7, 5)
SEG1, SEG2 = ("v", 0, 30), ("v", 15, 45)


def _case(preds1, preds2, shift2=0.0):
    rels = [(SEG1, (list(preds1), None, None)), (SEG2, (list(preds2), None, None))]
    return rels, {SEG1: _boxes(2, 30), SEG2: _boxes(2, 30, shift2)}


def _run(rels, trajs, **kw):
    return _association().greedy_relational_association(None, copy.deepcopy(rels), trajectories=trajs, **kw)


def _check_lengths(out):
    for r in out:
        n = r["duration"][1] - r["duration"][0]
        assert n > 0 and len(r["sub_traj"]) == n and len(r["obj_traj"]) == n, r["duration"]


def test_span_reaching_the_segment_end_continues_into_the_next_segment():
    rels, trajs = _case([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 1), (0, 20))], shift2=2.0)
    out = _run(rels, trajs)
    assert out == ref.associate(rels, trajs)
    assert len(out) == 1 and out[0]["duration"] == [10, 35] and out[0]["score"] == pytest.approx(0.85)
    _check_lengths(out)
    assert out[0]["sub_traj"][0] == (0.0, 10.0, 60.0, 80.0)          # frames [10, 15): segment 1 alone
    assert out[0]["sub_traj"][5] == (1.0, 10.0, 61.0, 80.0)          # [15, 30): the average
    assert out[0]["sub_traj"][-1] == (2.0, 10.0, 62.0, 80.0)         # [30, 35): segment 2 alone


def test_span_ending_early_is_not_continued():
    """Span [0, 12) of segment 1 stops before segment 2 begins (frame 15): the same triplet on the same tracklets in
    segment 2 is a new relation (confidence 1, the constructor default of the reference)."""
    rels, trajs = _case([(0.9, TRIP, (0, 1), (0, 12))], [(0.8, TRIP, (0, 1), (0, 20))])
    out = _run(rels, trajs)
    assert out == ref.associate(rels, trajs)
    assert [r["duration"] for r in out] == [[0, 12], [15, 35]] and [r["score"] for r in out] == [0.9, 1.0]
    _check_lengths(out)


def test_later_span_that_starts_before_or_ends_inside_opens_a_new_relation():
    """Segment 2's spans against the relation [20, 30): one that ends inside it ([15, 28)), and - through a third segment
    visited later but starting earlier in time than the relation it meets - one that starts before it."""
    rels, trajs = _case([(0.9, TRIP, (0, 1), (20, 30))], [(0.8, TRIP, (0, 1), (0, 13)), (0.7, TRIP, (0, 1), (5, 12))])
    out = _run(rels, trajs)                                          # [15, 28) and [20, 27): neither reaches frame 30
    assert out == ref.associate(rels, trajs)
    assert [r["duration"] for r in out] == [[20, 30], [15, 28], [20, 27]]
    _check_lengths(out)
    # starts before the relation: relation [25, 30) of segment 1, span [15, 40) of segment 2
    rels, trajs = _case([(0.9, TRIP, (0, 1), (25, 30))], [(0.8, TRIP, (0, 1), (0, 25))])
    out = _run(rels, trajs)
    assert out == ref.associate(rels, trajs)
    assert [r["duration"] for r in out] == [[25, 30], [15, 40]]
    _check_lengths(out)


def test_two_predictions_on_one_tracklet_do_not_alias():
    """Both relations of segment 1 use tracklets (0, 1); only the first is extended: the second keeps its own boxes."""
    other = (3, 8, 5)
    rels, trajs = _case([(0.9, TRIP, (0, 1), (10, 30)), (0.6, other, (0, 1), (10, 30))],
                        [(0.8, TRIP, (0, 1), (0, 20))], shift2=2.0)
    out = _run(rels, trajs)
    assert out == ref.associate(rels, trajs)
    assert [r["duration"] for r in out] == [[10, 35], [10, 30]]
    assert out[1]["sub_traj"] == [(0.0, 10.0, 60.0, 80.0)] * 20 and out[1]["obj_traj"] == [(100.0, 10.0, 160.0, 80.0)] * 20
    _check_lengths(out)


def test_three_tuples_are_unchanged_and_alias_as_in_the_reference():
    """The same data as 3-tuples: whole-segment relations, shared Track objects (the second relation's trajectory grows
    with the first one's merge) - the result recorded from the code before span mode existed."""
    other = (3, 8, 5)
    rels, trajs = _case([(0.9, TRIP, (0, 1)), (0.6, other, (0, 1))], [(0.8, TRIP, (0, 1))], shift2=2.0)
    out = _run(rels, trajs)
    assert [r["duration"] for r in out] == [[0, 45], [0, 30]]
    assert [r["score"] for r in out] == [pytest.approx(0.85), 0.6]
    assert len(out[0]["sub_traj"]) == 45 and len(out[1]["sub_traj"]) == 45      # aliased: the reference's behaviour
    assert out[0]["sub_traj"][:15] == [(0.0, 10.0, 60.0, 80.0)] * 15
    assert out[0]["sub_traj"][15:30] == [(1.0, 10.0, 61.0, 80.0)] * 15
    assert out[0]["sub_traj"][30:] == [(2.0, 10.0, 62.0, 80.0)] * 15


def test_device_with_span_predictions_raises_and_bad_spans_are_refused():
    rels, trajs = _case([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 1), (0, 20))])
    with pytest.raises(ValueError, match="device=None"):
        _run(rels, trajs, device="cuda:0")
    for bad in ((5, 5), (-1, 4), (3, 31)):
        rels, trajs = _case([(0.9, TRIP, (0, 1), bad)], [])
        with pytest.raises(ValueError, match="does not lie inside"):
            _run(rels, trajs)


def test_short_term_relations_from_arrays_takes_spans():
    A = _association()
    sc = [np.array([0.9], np.float32), np.array([0.8], np.float32)]
    tr = [np.array([TRIP]), np.array([TRIP])]
    pr = [np.array([[0, 1]]), np.array([[0, 1]])]
    sp = [np.array([[10, 30]]), np.array([[0, 20]])]
    boxes = [_boxes(2, 30), _boxes(2, 30)]
    rels, trajs = A.short_term_relations_from_arrays([SEG1, SEG2], sc, tr, pr, boxes, spans=sp)
    assert all(len(p) == 4 for _, (preds, _, _) in rels for p in preds)
    out = A.greedy_relational_association(None, rels, trajectories=trajs)
    assert len(out) == 1 and out[0]["duration"] == [10, 35]
    rels3, _ = A.short_term_relations_from_arrays([SEG1, SEG2], sc, tr, pr, boxes)
    assert all(len(p) == 3 for _, (preds, _, _) in rels3 for p in preds)
    with pytest.raises(ValueError, match="spans"):
        A.short_term_relations_from_arrays([SEG1, SEG2], sc, tr, pr, boxes, spans=[sp[0][:0], sp[1]])
