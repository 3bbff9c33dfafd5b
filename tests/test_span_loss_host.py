"""Span anchor targets and losses, the parts that need no GPU: the discipline of csrc/spanloss/ (kernel variant table,
built sources, no probe blocks, the store-hazard lint), the three entry points in header / binding / library and their
refusals, the float64 restatement (tests/span_loss_reference.py) on the hand-made threshold edges, and the conditions the
GPU tests' generated inputs have to meet."""
import ast
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import span_loss_reference as ref
import spanloss_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_SL = os.path.join(PKG, "csrc", "spanloss")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_SL, "*.hip")) + glob.glob(os.path.join(CSRC_SL, "*.h")))
ENTRIES = {"tspn_span_anchor_labels", "tspn_span_loss_f32", "tspn_span_loss_finish"}

# (P, G, A, T) of tests/test_gpu_span_loss.py: A*T of 60, 64, 68 around one wave's width, idle waves in the last workgroup
# (P % 4 != 0), several strides per lane (480, 195 anchors), G at its limit, G = 0, more pairs than the finish kernel has threads
SHAPES = [(1, 1, 1, 1), (5, 3, 4, 15), (5, 3, 4, 16), (5, 3, 4, 17), (3, 8, 16, 30), (257, 2, 4, 30), (4, 0, 4, 7), (6, 3, 3, 65)]
# the shapes that have room for the three special pairs of ref.make_gt and for a random pair besides
FULL_SHAPES = [s for s in SHAPES if s[0] >= 5 and s[1] >= 2]


def case(shape, seed=0):
    """(gt, sizes, heads) of one shape; the seed depends on the shape only, so every test sees the same inputs."""
    P, G, A, T = shape
    sizes = ref.make_sizes(A, T)
    gt = ref.make_gt(1000 + seed + 7 * P + 3 * T + G, P, G, T)
    return gt, sizes, ref.make_heads(2000 + seed + P + T, gt, sizes, T)


def test_spanloss_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_SL, "*.hip"))))
    assert in_source == {r["kernel"] for r in spanloss_kernel_variants.VARIANTS} and len(in_source) == 4
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in spanloss_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] in ENTRIES and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    # no kernel of the new directory is also defined in an older one: the older tables stay complete
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_SL]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    tool = open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    assert "spanloss_kernel_variants.VARIANTS" in tool


def test_spanloss_sources_are_built_and_carry_no_probe_blocks_memsets_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert "hipMemsetAsync" not in text and "atomic" not in text.lower(), f"{f}: the kernels write every output themselves"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_store_hazard_lint_passes_on_the_spanloss_sources():
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] + hips,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert all(os.path.basename(f) in res.stdout for f in hips)


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in spanloss_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k in n for k in names)}
    assert len(found) == len(names)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)


def test_entry_points_are_declared_bound_and_exported_without_scratch_parameters():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert {"span_anchor_labels", "span_loss"} <= set(tspn_mi355x.ops.__all__)
    assert abi.lib().tspn_version() == 7                                # the entries only add symbols
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    for name in ENTRIES:
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)
        assert "workspace" not in params and name + "_workspace_bytes" not in header
    cfg = tspn_mi355x.default_cfg().RELPN.DPN.SPAN_LOSS
    assert (cfg.POS_IOU, cfg.NEG_IOU, cfg.SMOOTH_L1_BETA) == (0.7, 0.3, 1.0 / 9.0)


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    import tspn_mi355x
    ops = tspn_mi355x.ops
    z = torch.zeros
    gt, heads = z((3, 2, 2), dtype=torch.int64), z(3, 12, 5)
    lab = z((3, 4, 5), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_anchor_labels(gt, [1.0, 2.0, 3.0, 4.0], 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_loss(heads, gt, [1.0, 2.0, 3.0, 4.0], lab, lab)
    with pytest.raises(TypeError):
        ops.span_anchor_labels([[0, 1]], [1.0], 5)


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any device work: the pointers are made-up addresses."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    p = ctypes.c_void_p
    ok, odd, null = p(0x10000), p(0x10004), p(0)
    sizes = (ctypes.c_float * 16)(*[float(i + 1) for i in range(16)])
    bad_sizes = (ctypes.c_float * 4)(1.0, 0.0, 2.0, 3.0)

    def labels(gt=ok, sz=sizes, P=3, G=2, A=4, T=5, pos=0.7, neg=0.3, label=ok, matched=ok):
        return lib.tspn_span_anchor_labels(gt, sz, P, G, A, T, pos, neg, label, matched, null), lib.tspn_last_error().decode()

    def loss(heads=ok, gt=ok, sz=sizes, label=ok, matched=ok, mask=null, P=3, G=2, A=4, T=5, beta=0.1, partials=ok, dheads=ok):
        return (lib.tspn_span_loss_f32(heads, gt, sz, label, matched, mask, P, G, A, T, beta, partials, dheads, null),
                lib.tspn_last_error().decode())

    def finish(partials=ok, P=3, A=4, T=5, out=ok, dheads=ok):
        return lib.tspn_span_loss_finish(partials, P, A, T, out, dheads, null), lib.tspn_last_error().decode()

    for call in (labels, loss):
        rc, msg = call(G=9)
        assert rc == A_.TSPN_EUNSUPPORTED and "G=9" in msg
        rc, msg = call(G=-1)
        assert rc == A_.TSPN_EINVAL and "G=-1" in msg
        rc, msg = call(gt=null)
        assert rc == A_.TSPN_EINVAL and "null pointer" in msg
        rc, msg = call(sz=None)
        assert rc == A_.TSPN_EINVAL and "null pointer" in msg
        rc, msg = call(sz=bad_sizes)
        assert rc == A_.TSPN_EINVAL and "anchor size 1" in msg
        rc, msg = call(gt=odd)
        assert rc == A_.TSPN_EUNSUPPORTED and "unaligned" in msg
        assert call(P=0, gt=null, label=null, matched=null)[0] == A_.TSPN_OK       # nothing to launch
    for call in (labels, loss, finish):
        rc, msg = call(A=17)
        assert rc == A_.TSPN_EUNSUPPORTED and "A=17" in msg
        assert call(A=0)[0] == A_.TSPN_EINVAL and call(T=0)[0] == A_.TSPN_EINVAL and call(P=-1)[0] == A_.TSPN_EINVAL
        rc, msg = call(A=16, T=2 ** 27)
        assert rc == A_.TSPN_EUNSUPPORTED and "anchors per pair" in msg
        assert call(A=1, T=2 ** 31)[0] == A_.TSPN_EUNSUPPORTED
    for pos, neg in ((0.3, 0.7), (1.5, 0.3), (0.7, -0.1), (float("nan"), 0.3), (0.7, float("nan"))):
        rc, msg = labels(pos=pos, neg=neg)
        assert rc == A_.TSPN_EINVAL and "thresholds" in msg, (pos, neg)
    assert labels(label=null)[0] == A_.TSPN_EINVAL and labels(matched=null)[0] == A_.TSPN_EINVAL
    for kw in ("heads", "label", "matched", "partials", "dheads"):
        rc, msg = loss(**{kw: null})
        assert rc == A_.TSPN_EINVAL and "null pointer" in msg, kw
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert loss(beta=beta)[0] == A_.TSPN_EINVAL
    for kw in ("partials", "out", "dheads"):
        rc, msg = finish(**{kw: null})
        assert rc == A_.TSPN_EINVAL and "null pointer" in msg, kw
    assert finish(P=0, out=null)[0] == A_.TSPN_EINVAL                    # P = 0 still writes `out`
    assert finish(out=odd)[0] == A_.TSPN_EUNSUPPORTED


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_labels_on_the_hand_made_edges():
    assert (7.0 / 10.0 >= ref.POS_IOU) and not (3.0 / 10.0 < ref.NEG_IOU)       # the two divisions round onto the literals
    for name, gt, sizes, T, expect in ref.edge_cases():
        label, matched, info = ref.labels_ref(np.array(gt), sizes, T)
        for (a, t), want in expect.items():
            assert label[0, a, t] == want, (name, a, t, label[0, a, t], info["iou"][0, 0, a, t])
        assert (matched == 0).all()
    name, gt, sizes, T, _ = ref.edge_cases()[0]
    iou = ref.labels_ref(np.array(gt), sizes, T)[2]["iou"]
    assert iou[0, 0, 0, 10] == 0.7 and iou[0, 0, 1, 8] == 6.5 / 7.5 == iou.max()
    iou = ref.labels_ref(np.array(ref.edge_cases()[1][1]), [10.0, 3.0], 21)[2]["iou"]
    assert iou[0, 0, 0, 10] == 0.3 and iou.max() == 2.5 / 3.5
    assert ref.labels_ref(np.array(ref.edge_cases()[2][1]), [10.0], 21)[2]["iou"][0, 0, 0, 10] == 1.0
    # the plateau: positives by the low-quality rule alone
    name, gt, sizes, T, _ = ref.edge_cases()[3]
    label, _, info = ref.labels_ref(np.array(gt), sizes, T)
    assert info["lowq"][0, 0, :6].all() and not info["thr"].any() and label.sum() == 6
    assert (info["iou"][0, 0, 0, :6] == 0.1).all()


def test_restatement_losses_by_hand():
    """One pair, one anchor width 4, T = 3, one span [0, 2): the anchors [-2, 2), [-1, 3), [0, 4) all have inter 2, union 4,
    so all three are positive by the low-quality rule alone; the losses and the gradient written out in numpy."""
    gt, sizes, T = np.array([[[0, 2]]]), [4.0], 3
    label, matched, info = ref.labels_ref(gt, sizes, T)
    assert info["iou"][0, 0, 0].tolist() == [0.5, 0.5, 0.5] and label[0, 0].tolist() == [1, 1, 1]    # all tied: low quality
    heads = np.array([[[0.5, -1.0, 2.0], [0.0, -0.25, -0.5], [np.log(0.5), np.log(0.5) + 0.05, 1.0]]], np.float32)
    out, dh, _, _ = ref.span_loss_ref(heads, gt, sizes)
    x = heads[0, 0].astype(np.float64)
    bce = np.maximum(x, 0) - x + np.log1p(np.exp(-np.abs(x)))
    assert out[2] == 3 and out[3] == 3 and abs(out[0] - bce.sum() / 3) < 1e-15
    tc = (1.0 - np.arange(3)) / 4.0                                    # ((0 + 2) / 2 - t) / 4
    d = np.concatenate([heads[0, 1].astype(np.float64) - tc, heads[0, 2].astype(np.float64) - np.log(0.5)])
    b = ref.BETA
    sl1 = np.where(np.abs(d) < b, 0.5 * d * d / b, np.abs(d) - 0.5 * b)
    assert (np.abs(d) < b).any() and (np.abs(d) > b).any() and abs(out[1] - sl1.sum() / 3) < 1e-15
    np.testing.assert_allclose(dh[0, 0], (1 / (1 + np.exp(-x)) - 1) / 3, rtol=1e-12)
    np.testing.assert_allclose(dh[0, 1:].reshape(-1), np.where(np.abs(d) < b, d / b, np.sign(d)) / 3, rtol=1e-12, atol=1e-18)


def test_generated_inputs_meet_the_conditions_the_gpu_tests_rely_on():
    for shape in SHAPES:
        P, G, A, T = shape
        gt, sizes, heads = case(shape)
        assert gt.dtype == np.int64 and all(float(s) * 4 == int(s * 4) and s > 0 for s in sizes)
        assert np.array_equal(ref.sizes64(sizes), np.asarray(sizes, np.float64))
        if shape in FULL_SHAPES:
            cond = ref.input_conditions(gt, sizes, T, heads)
            assert all(cond.values()), (shape, cond)
            assert (gt[0, :, 1] <= gt[0, :, 0]).all() and np.array_equal(gt[1, 0], gt[1, G - 1])
            if G >= 3:          # padding between two ground-truth rows
                valid = gt[:, :, 1] > gt[:, :, 0]
                assert any(valid[p, 0] and not valid[p, 1:-1].all() and valid[p, -1] for p in range(P))
    assert len(FULL_SHAPES) >= 5
    # the segment without a positive anchor
    gt, sizes, heads = case((4, 0, 4, 7))
    out, dh, label, matched = ref.span_loss_ref(heads, gt, sizes)
    assert out[3] == 0 and out[1] == 0 and out[2] == 4 * 4 * 7 and not dh[:, 4:].any() and (matched == -1).all()


def test_torch_composition_equals_the_numpy_labels():
    """tools/bench_span_loss.py times this composition on the GPU: here it is held to the restatement on the CPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_span_loss
    for shape in ((5, 3, 4, 17), (6, 3, 3, 65)):
        gt, sizes, heads = case(shape)
        T = shape[3]
        label, matched, _ = ref.labels_ref(gt, sizes, T)
        l2, m2 = bench_span_loss.labels_torch(torch.from_numpy(gt), sizes, T, ref.POS_IOU, ref.NEG_IOU)
        assert np.array_equal(l2.numpy(), label) and np.array_equal(m2.numpy(), matched)


def test_decode_round_trip_on_the_oracle():
    """What tests/test_gpu_span_loss.py::test_decode_round_trip asks of ops.decode_spans, on oracle.decode_spans first: heads
    that hold the regression targets (rounded to fp32) and +10 / -10 logits decode, top_k = 1, to the ground-truth row of
    every pair with ground truth whose positives all match one row -- all 156 such pairs of these shapes, none left out
    (the decode stores start and end as fp32, which takes the targets' fp32 rounding back onto the integer frames)."""
    for shape in FULL_SHAPES:
        P, G, A, T = shape
        gt, sizes, _ = case(shape)
        heads, pairs = round_trip_heads(gt, sizes, T)
        h = torch.from_numpy(heads)
        got = oracle.decode_spans(h[:, :A], h[:, A:], sizes, top_k=1)["span"][:, 0].numpy()
        assert len(pairs) >= 2, (shape, pairs)
        for p, g in pairs:                      # every one of them: no pair is left out
            assert got[p].tolist() == gt[p, g].tolist(), (shape, p, got[p], gt[p, g])


def round_trip_heads(gt, sizes, T):
    """(heads fp32 [P, 3A, T], [(pair, row)]): the regression channels hold the float64 targets rounded to fp32, the logits
    are +10 at positives and -10 elsewhere.  The pairs listed are those with ground truth whose positives all match one
    row, the ones the round trip is stated for: where the positives match several rows, the best-ranked one (the lowest
    candidate index among equal logits) may belong to any of them."""
    P, A = len(gt), len(sizes)
    label, matched, _ = ref.labels_ref(gt, sizes, T)
    tc, tw = ref.targets_ref(gt, sizes, T, matched)
    heads = np.zeros((P, 3 * A, T), np.float32)
    heads[:, :A] = np.where(label == 1, 10.0, -10.0)
    heads[:, A::2], heads[:, A + 1::2] = tc, tw
    pairs = []
    for p in range(P):
        rows = set(matched[p][label[p] == 1].tolist())
        if len(rows) == 1:
            pairs.append((p, rows.pop()))
    return heads, pairs
