"""Span-bounded association matched in one call per segment, the parts that need no GPU: the numpy restatement
(tests/span_match_reference.py) and the association that only applies its answer against the host path and against the
reference-order restatement; the package's own packing of a segment, with the restatement standing in for the kernels;
the refusals of the C entry, of `ops.span_match` and of the `device_spans` keyword; and the discipline of csrc/spanmatch/
(kernel variant table, built sources, no probe blocks, no memset, no environment reads, no spills)."""
import ast
import copy
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import span_association_cases as sac
import span_match_reference as ref
import span_relations_reference
import spanmatch_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_SM = os.path.join(PKG, "csrc", "spanmatch")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_SM, "*.hip")) + glob.glob(os.path.join(CSRC_SM, "*.h")))
ENTRY = "tspn_span_match_f64"
_HOST = {}


def _association():
    import tspn_mi355x
    return tspn_mi355x.association


def host_result(scenario, cap=100):
    """`greedy_relational_association(device=None)` of a scenario, computed once and shared (never modified)."""
    if (scenario, cap) not in _HOST:
        rels, trajs = sac.spanned(*scenario)
        _HOST[(scenario, cap)] = _association().greedy_relational_association(None, rels, max_traj_num_in_clip=cap,
                                                                              trajectories=trajs)
    return _HOST[(scenario, cap)]


def restatement_as_op(*tensors, iou_thr=0.5):
    """`ops.span_match` answered by the restatement: torch tensors in, torch tensors out."""
    match, iou = ref.span_match(*[t.cpu().numpy() for t in tensors], iou_thr=iou_thr)
    return torch.from_numpy(match), torch.from_numpy(iou)


# --------------------------------------------------------------------------------- the restatement and the association
@pytest.mark.parametrize("scenario", sorted(sac.SCENARIOS))
def test_match_once_per_segment_equals_the_host_path_and_the_reference_order(scenario):
    rels, trajs = sac.spanned(*scenario)
    host = host_result(scenario)
    stats = {}
    assert ref.associate(copy.deepcopy(rels), trajs, stats=stats) == host
    assert span_relations_reference.associate(copy.deepcopy(rels), trajs) == host
    assert 1 <= stats["calls"] <= scenario[1] - 1 and stats["pairs"] >= stats["calls"]
    # the scenario does what the feature is about: relations that outlast a segment, spans off the 15-frame grid
    assert sum(r["duration"][1] - r["duration"][0] > 30 for r in host) >= 10
    assert sum(r["duration"][0] % 15 != 0 for r in host) >= 1


@pytest.mark.parametrize("cap", [100, 25])
def test_package_packing_with_the_restatement_as_the_op_equals_the_host_path(monkeypatch, cap):
    """`greedy_relational_association(device_spans=True)` with `ops.span_match` answered by the restatement (on the CPU):
    the package's own upload arrays, candidate rows and apply-the-match loop give the host path's relations."""
    import tspn_mi355x
    monkeypatch.setattr(tspn_mi355x.ops, "span_match", restatement_as_op)
    scenario = (11, 5, 7, 40)
    rels, trajs = sac.spanned(*scenario)
    stats = {}
    got = _association().greedy_relational_association(None, rels, max_traj_num_in_clip=cap, trajectories=trajs,
                                                       device="cpu", device_spans=True, stats=stats)
    assert got == host_result(scenario, cap)
    assert 1 <= stats["iou_launches"] <= 4 and stats["iou_host_rows"] == 0 and stats["segments"] == 5
    assert stats["iou_lookups"] >= stats["iou_launches"]


def test_restatement_by_hand():
    """Two relations, three predictions, L = 4: the gates, the window, first-free-candidate."""
    box = np.array([0.0, 0.0, 9.0, 9.0])
    rel_boxes = np.tile(box, (2, 2, 4, 1))
    trk = np.tile(box, (2, 4, 1))
    trk[1, :, 2] = 4.0                                           # tracklet 1: half as wide -> IoU 0.5 exactly
    rng = np.array([[[0, 3], [0, 3]], [[0, 4], [0, 4]]], dtype=np.int32)
    fend = np.array([3, 4], dtype=np.int32)
    trip = np.array([[1, 2, 3], [1, 2, 3]], dtype=np.int64)
    ptrip = np.array([[1, 2, 3]] * 3 + [[1, 2, 4]], dtype=np.int64)
    pair = np.array([[0, 1], [0, 0], [0, 0], [0, 0]], dtype=np.int32)
    span = np.array([[1, 4], [2, 4], [3, 4], [0, 4]], dtype=np.int32)
    match, iou = ref.span_match(rel_boxes, rng, fend, trip, trk, ptrip, pair, span)
    assert match.tolist() == [0, 1, -1, -1] and match.dtype == np.int32 and iou.dtype == np.float32
    assert iou[0, 0].tolist() == [1.0, 0.5] and iou[1, 0].tolist() == [1.0, 0.5]
    assert iou[0, 2].tolist() == [-1.0, -1.0]                    # a = 3 == rel_fend = end of relation 0
    assert iou[1, 2].tolist() == [1.0, 1.0] and iou[:, 3].tolist() == [[-1.0, -1.0]] * 2
    assert ref.span_match(rel_boxes, rng, fend, trip, trk, ptrip, pair, span, iou_thr=0.51)[0].tolist() == [-1, 0, 1, -1]


# ------------------------------------------------------------------------------------------- the entry
def test_entry_point_is_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRY in abi.header_symbols() and ENTRY in abi.PROTOTYPES and hasattr(ctypes.CDLL(abi.LIB_PATH), ENTRY)
    assert "span_match" in tspn_mi355x.ops.__all__ and abi.lib().tspn_version() == 7
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\btspn_span_match_f64\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    assert "workspace" not in params and len(params.split(",")) == len(abi.PROTOTYPES[ENTRY][1]) == 16


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any launch: the pointers are made-up addresses.  Return code
    and the whole message."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    vp = ctypes.c_void_p
    ok, null = vp(0x10000), vp(0)
    names = ("rel_boxes", "rel_range", "rel_fend", "rel_triplet", "trk_boxes", "pred_triplet", "pred_pair", "pred_span")

    def call(U=3, P=4, N=5, L=30, thr=0.5, iou=ok, match=ok, **ptr):
        rc = lib.tspn_span_match_f64(*[ptr.get(n, ok) for n in names], U, P, N, L, thr, iou, match, null)
        return rc, lib.tspn_last_error().decode()

    w = ENTRY + ": "
    assert call(U=-1) == (A_.TSPN_EINVAL, w + "bad sizes U=-1 P=4 N=5 L=30")
    assert call(P=-1)[0] == call(N=-1)[0] == call(L=-1)[0] == A_.TSPN_EINVAL
    for n in names:
        assert call(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert call(iou=null) == call(match=null) == (A_.TSPN_EINVAL, w + "null pointer")
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(thr=bad) == (A_.TSPN_EINVAL, w + "iou_thr is not finite")
    assert call(U=65537) == (A_.TSPN_EUNSUPPORTED,
                             w + "U=65537 relations (needs U <= 65536: the taken flags live in LDS)")
    assert call(U=65536, P=32768) == (A_.TSPN_EUNSUPPORTED, w + "U=65536 x P=32768 pairs (needs U * P < 2^31)")
    assert call(U=3, P=2 ** 62)[0] == A_.TSPN_EUNSUPPORTED          # no overflow in the product
    assert call(L=2 ** 31) == (A_.TSPN_EUNSUPPORTED, w + "N=5 L=2147483648 (each needs < 2^31)")
    assert call(N=2 ** 31)[0] == A_.TSPN_EUNSUPPORTED
    # the order: sizes, null pointers, threshold, U, U * P
    assert "bad sizes" in call(U=-1, match=null)[1] and "null pointer" in call(match=null, thr=float("nan"))[1]
    assert "not finite" in call(thr=float("nan"), U=65537)[1] and "U=65537 relations" in call(U=65537, P=2 ** 40)[1]
    # no predictions: served without a launch and without any pointer, whatever U says
    nothing = {n: null for n in names}
    assert call(P=0, iou=null, match=null, **nothing)[0] == A_.TSPN_OK
    assert call(U=0, P=0, N=0, L=0, iou=null, match=null, **nothing)[0] == A_.TSPN_OK
    # operands without elements may be null: no relations; no tracklets or no frames (nothing can be a candidate)
    rels = {n: null for n in names if n.startswith("rel_")}
    assert "null pointer" not in call(U=0, iou=null, trk_boxes=null, **rels, thr=float("nan"))[1]
    assert "null pointer" not in call(N=0, rel_boxes=null, trk_boxes=null, thr=float("nan"))[1]
    assert "null pointer" not in call(L=0, rel_boxes=null, trk_boxes=null, thr=float("nan"))[1]


def test_op_refuses_cpu_tensors_and_foreign_objects():
    import tspn_mi355x
    z = torch.zeros
    args = [z((1, 2, 3, 4), dtype=torch.float64), z((1, 2, 2), dtype=torch.int32), z(1, dtype=torch.int32),
            z((1, 3), dtype=torch.int64), z((2, 3, 4), dtype=torch.float64), z((1, 3), dtype=torch.int64),
            z((1, 2), dtype=torch.int32), z((1, 2), dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn_mi355x.ops.span_match(*args)
    with pytest.raises(TypeError):
        tspn_mi355x.ops.span_match(args[0].numpy(), *args[1:])


# ------------------------------------------------------------------------------------------- the keyword
TRIP = (1, 2, 3)


def _two_segments(preds1, preds2, n=2, L=30):
    boxes = np.tile(np.array([0.0, 0.0, 50.0, 60.0]), (n, L, 1))
    mk = lambda preds: [(np.array(p[0]), np.array(p[1]), np.array(p[2])) + ((np.array(p[3]),) if len(p) == 4 else ())  # noqa: E731
                        for p in preds]
    rels = [(("v", 0, L), (mk(preds1), None, None)), (("v", 15, 15 + L), (mk(preds2), None, None))]
    return rels, {("v", 0, L): boxes, ("v", 15, 15 + L): boxes.copy()}


def test_keyword_refusals(monkeypatch):
    import tspn_mi355x
    A = _association()
    run = lambda rels, trajs, **kw: A.greedy_relational_association(None, copy.deepcopy(rels), trajectories=trajs, **kw)  # noqa: E731
    spanned = _two_segments([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 1), (0, 20))])
    with pytest.raises(ValueError, match="device_spans=True needs a device"):
        run(*spanned, device_spans=True)
    # the default keeps the refusal of 4-tuples with a device, word for word
    with pytest.raises(ValueError, match=r"span-bounded predictions \(4-tuples\) need device=None: the batched IoU table is per "
                                         "whole tracklet"):
        run(*spanned, device="cuda:0")
    with pytest.raises(ValueError, match="device=None"):
        run(*spanned, device="cuda:0", device_spans=False)
    mixed = _two_segments([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 1))])
    called = []
    monkeypatch.setattr(tspn_mi355x.ops, "span_match", lambda *a, **k: called.append(1) or restatement_as_op(*a, **k))
    with pytest.raises(ValueError, match="mixes whole-segment"):
        run(*mixed, device="cpu", device_spans=True)
    assert not called
    # bad spans and pair indices: the host path's errors, before the device is asked
    for bad in ((5, 5), (-1, 4), (3, 31)):
        case = _two_segments([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 1), bad)])
        with pytest.raises(ValueError, match="does not lie inside") as host:
            run(*case)
        with pytest.raises(ValueError, match="does not lie inside") as dev:
            run(*case, device="cpu", device_spans=True)
        assert str(host.value) == str(dev.value)
    case = _two_segments([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, 2), (0, 20))])
    with pytest.raises(IndexError) as host:
        run(*case)
    with pytest.raises(IndexError) as dev:
        run(*case, device="cpu", device_spans=True)
    assert str(host.value) == str(dev.value) and not called
    # a good video reaches the op once per later segment; a negative pair index counts from the end, as on the host
    case = _two_segments([(0.9, TRIP, (0, 1), (10, 30))], [(0.8, TRIP, (0, -1), (0, 20))])
    assert run(*case, device="cpu", device_spans=True) == run(*case) and called == [1]
    assert run(*case)[0]["duration"] == [10, 35]


def test_worker_takes_the_keyword():
    import inspect
    A = _association()
    assert inspect.signature(A.AssociationWorker.__init__).parameters["device_spans"].default is False
    assert inspect.signature(A.greedy_relational_association).parameters["device_spans"].default is False
    assert "device=None only" not in inspect.getsource(A.AssociationWorker.submit_arrays)


# ------------------------------------------------------------------------------------------- the sources
def test_spanmatch_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_SM, "*.hip"))))
    assert in_source == {r["kernel"] for r in spanmatch_kernel_variants.VARIANTS} and len(in_source) == 2
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in spanmatch_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] == ENTRY and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_SM]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "spanmatch_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    text = open(os.path.join(CSRC_SM, "tspn_span_match.hip")).read()
    consts = {m.group(1): m.group(2).strip() for m in re.finditer(r"constexpr int (\w+) = ([^;,]+)[;,]", text)}
    assert (consts["TILE"], consts["MAX_U"], consts["TAKEN_WORDS"]) == ("256", "65536", "MAX_U / 32")


def test_pairwise_sum_has_one_copy_that_both_iou_sources_include():
    hits = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*"), recursive=True)
            if os.path.isfile(f) and re.search(r"double\s+np_(block|pairwise)_sum\s*\(", open(f).read())]
    assert hits == [os.path.join(PKG, "csrc", "tspn_np_sum.h")]
    for f in (os.path.join(PKG, "csrc", "tspn_iou.hip"), os.path.join(CSRC_SM, "tspn_span_match.hip")):
        assert '#include "tspn_np_sum.h"' in open(f).read()
    assert hits[0] in _build_module()._headers()


def test_spanmatch_sources_are_built_and_carry_no_probe_blocks_memsets_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "getenv" not in text, f"{f} reads the environment"
        assert "hipMemset" not in text and "hipMalloc" not in text and "Synchronize" not in text, f"{f}: launch contract"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert not re.search(r"[aA]tomic", code), f"{f}: no atomics"
        assert "workspace" not in code and code.count("hipLaunchKernelGGL") == 2
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_new_kernels_do_not_spill():
    """No register spills and no scratch memory, in the two new kernels and in traj_iou_tail_f64_kernel, which shares
    `np_pairwise_sum`: its parked sums live in an LDS column per thread (kNpSumLevels x 256 doubles)."""
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in spanmatch_kernel_variants.VARIANTS} | {"traj_iou_tail_f64_kernel"}
    found = {n.split("::")[-1].split("(")[0]: r for n, r in res.items() if any(k + "(" in n for k in names)}
    assert set(found) == names
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
    assert found["span_match_iou_kernel"]["lds_bytes"] == found["traj_iou_tail_f64_kernel"]["lds_bytes"] == 26 * 256 * 8
    assert 8192 <= found["span_match_greedy_kernel"]["lds_bytes"] <= 8192 + 64
