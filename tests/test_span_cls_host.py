"""Training the predicate head on ground-truth-span-pooled features, the parts that need no GPU: the invariants of the
numpy restatement (tests/span_cls_reference.py) against the pair labels, the refusals of the four C entries, and the
discipline of csrc/spancls/ (kernel variant table, built sources, no switches, no memset, no atomics, no environment
reads, no `workspace` parameter or size export, no spills)."""
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

import pair_labels_reference as plr
import span_cls_reference as ref
import spancls_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_SC = os.path.join(PKG, "csrc", "spancls")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_SC, "*.hip")) + glob.glob(os.path.join(CSRC_SC, "*.h")))
CASES = ref.label_cases()


def empty_clip_covers(seg, K, thr):
    """Pairs of the segment that a live instance covers whose clipped span is empty."""
    trackid, iou, pairs, insts = seg["trackid"], seg["iou"], seg["pairs"], seg["insts"]
    fstart, fend = seg["frames"]
    cols = plr.segment_ref(seg, K, 0, thr, "or")[3]
    hit = np.zeros(len(pairs), bool)
    M = len(trackid)
    for r in range(len(insts)):
        if cols[r, 0] < 0 or cols[r, 1] < 0 or min(insts[r, 4], fend) > max(insts[r, 3], fstart):
            continue
        for p, (s, o) in enumerate(pairs):
            if 0 <= s < M and 0 <= o < M and s != o and trackid[s] < 0 and trackid[o] < 0 \
                    and iou[s, cols[r, 0]] >= np.float32(thr) and iou[o, cols[r, 1]] >= np.float32(thr):
                hit[p] = True
    return hit


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["merge"] == "or"])
def test_or_rows_stay_below_the_pair_labels_and_reach_them_where_no_span_is_lost(cid):
    case = next(c for c in CASES if c["id"] == cid)
    K, G = case["K"], case["G"]
    seen = set()
    for seg in case["segments"]:
        labels, spans, count, _ = plr.segment_ref(seg, K, G, case["thr"], "or")
        rows = ref.span_labels_segment(seg, K, G, case["thr"], "or", spans, count)
        assert rows.dtype == np.float32 and rows.shape == (len(labels), G, K) and set(np.unique(rows).tolist()) <= {0.0, 1.0}
        top = rows.max(axis=1, initial=0.0)
        assert (top <= labels).all()
        kept = (count >= 0) & (count <= G) & ~empty_clip_covers(seg, K, case["thr"])
        assert np.array_equal(top[kept], labels[kept])
        for p in range(len(labels)):
            assert not rows[p, max(int(count[p]), 0):].any()                     # rows past the count, count <= 0
            assert all(rows[p, g].any() for g in range(min(max(int(count[p]), 0), G)))   # a stored span has an instance
        seen |= {"lost span" for _ in [0] if (top < labels).any()} | {"saturated" for _ in [0] if (count == G + 1).any()}
        seen |= {"negative count" for _ in [0] if (count == -1).any()} | {"rows" for _ in [0] if rows.any()}
    if cid.startswith(("G1-dense", "G4-dense", "G16-dense")):
        assert {"lost span", "saturated", "rows"} <= seen
    if cid.startswith("P257"):
        assert {"negative count", "rows"} <= seen


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["merge"] == "last"])
def test_last_rows_are_one_hot(cid):
    case = next(c for c in CASES if c["id"] == cid)
    K, G = case["K"], case["G"]
    for seg in case["segments"]:
        _, spans, count, _ = plr.segment_ref(seg, K, G, case["thr"], "last")
        rows = ref.span_labels_segment(seg, K, G, case["thr"], "last", spans, count)
        valid = np.arange(G)[None, :] < np.minimum(np.maximum(count, 0), G)[:, None]
        assert (rows.sum(axis=2)[valid] == 1.0).all() and not rows[~valid].any()
        either = ref.span_labels_segment(seg, K, G, case["thr"], "or", spans, count)
        assert (rows <= either).all()


def test_loss_restatement_by_hand_and_against_autograd():
    """One pair, two adjacent spans and a negative pair by hand; then the restatement's dW / db against float64 autograd
    of binary_cross_entropy_with_logits over explicitly pooled rows, two segments."""
    c = ref.loss_case(5, 5, 2, 6, 4, 3, 2, table="shuffled")
    r = ref.loss_ref(c["feats"], c["pairs"], c["spans"], c["span_count"], c["span_labels"], c["cls_w"], c["cls_b"], c["pair_off"])
    NT, T, D, K, G, S = c["dims"]
    valid, a, e = ref.row_table(c["pairs"], c["spans"], c["span_count"], NT, T, G)
    assert valid[0].tolist() == [True, True] and (a[0, 0], e[0, 0], a[0, 1], e[0, 1]) == (0, 3, 3, 6)
    assert not valid[2].any() and not valid[3].any() and r["seg_rows"].sum() == valid.sum()
    w, b = torch.tensor(c["cls_w"], dtype=torch.float64, requires_grad=True), torch.tensor(c["cls_b"], dtype=torch.float64, requires_grad=True)
    f = torch.tensor(c["feats"], dtype=torch.float64)
    total = 0
    for s in range(S):
        xs, ys = [], []
        for p in range(c["pair_off"][s], c["pair_off"][s + 1]):
            for g in range(G):
                if valid[p, g]:
                    i, j = c["pairs"][p]
                    xs.append(torch.cat([f[i, a[p, g]:e[p, g]].mean(0), f[j, a[p, g]:e[p, g]].mean(0)]))
                    ys.append(torch.tensor(c["span_labels"][p, g] if c["span_count"][p] >= 1 else np.zeros(K), dtype=torch.float64))
        total = total + torch.nn.functional.binary_cross_entropy_with_logits(torch.stack(xs) @ w.t() + b, torch.stack(ys))
    total.backward()
    np.testing.assert_allclose(r["loss"], float(total.detach()), rtol=1e-12)
    np.testing.assert_allclose(r["dW"], w.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["db"], b.grad.numpy(), rtol=0, atol=1e-12)
    assert not r["dG"][NT - 1].any() and not r["dv"][~r["valid"]].any() and not r["q"][~r["valid"]].any()


# ------------------------------------------------------------------------------------------- the entries
def test_entry_points_are_declared_bound_exported_and_take_named_scratch():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    handle = ctypes.CDLL(abi.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    for entry, count in zip(spancls_kernel_variants.ENTRIES, (22, 22, 9, 14)):
        assert entry in abi.header_symbols() and entry in abi.PROTOTYPES and hasattr(handle, entry)
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % entry, header, re.S).group(1)
        assert not re.search(r"\bworkspace\b", params) and len(params.split(",")) == len(abi.PROTOTYPES[entry][1]) == count
    assert not [n for n in abi.header_symbols() if n.endswith("_workspace_bytes") and "span_predicate_loss" in n]
    assert {"span_labels", "span_predicate_loss", "span_predicate_grad"} <= set(tspn_mi355x.ops.__all__)
    assert abi.lib().tspn_version() == 7


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any device work: the pointers are made-up addresses.  Return
    code and the whole message."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    vp = ctypes.c_void_p
    ok, odd4, odd2, null = vp(0x10000), vp(0x10004), vp(0x10002), vp(0)
    names = ("pairs", "pair_off", "trackid", "track_off", "iou", "iou_off", "insts", "inst_off", "seg_frames")

    def labels(S=2, P=10, M=5, R=3, K=132, G=4, thr=0.5, merge=0, spans=ok, span_count=ok, inst_cols=ok, out=ok, **ptr):
        args = [ptr.get(n, ok) for n in names]
        rc = lib.tspn_span_labels_f32(*args, S, P, M, R, K, G, thr, merge, spans, span_count, inst_cols, out, null)
        return rc, lib.tspn_last_error().decode()

    w = "tspn_span_labels_f32: "
    assert labels(P=-1) == (A_.TSPN_EINVAL, w + "bad sizes S=2 P=-1 M=5 R=3")
    assert labels(P=2 ** 31) == (A_.TSPN_EUNSUPPORTED, w + "S=2 P=2147483648 M=5 R=3 (each needs < 2^31)")
    assert labels(K=0) == (A_.TSPN_EINVAL, w + "K=0 predicates (needs K >= 1)")
    assert labels(K=513) == (A_.TSPN_EUNSUPPORTED, w + "K=513 predicates (needs K <= 512)")
    assert labels(G=0) == (A_.TSPN_EINVAL, w + "G=0 span rows (needs 1 <= G)")
    assert labels(G=17) == (A_.TSPN_EUNSUPPORTED, w + "G=17 span rows (needs G <= 16)")
    assert labels(merge=2) == (A_.TSPN_EINVAL, w + "unknown merge=2 (0 = last, 1 = or)")
    for bad in (float("nan"), float("inf")):
        assert labels(thr=bad) == (A_.TSPN_EINVAL, w + "iou_thres is not finite")
    msg = w + "S=2 needs pair_off, track_off, iou_off and inst_off (all null: one segment)"
    for n in ("pair_off", "track_off", "iou_off", "inst_off"):
        assert labels(**{n: null}) == (A_.TSPN_EINVAL, msg)
    assert labels(S=0) == (A_.TSPN_EINVAL, w + "S=0 with P=10 pairs and R=3 instances")
    for n in ("pairs", "trackid", "iou", "insts", "seg_frames"):
        assert labels(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert labels(spans=null) == labels(span_count=null) == labels(inst_cols=null) == labels(out=null) \
        == (A_.TSPN_EINVAL, w + "null pointer")
    msg = w + "unaligned pointer (int64 operands need 8 bytes, fp32 and int32 ones 4)"
    for n in ("pairs", "pair_off", "trackid", "track_off", "iou_off", "insts", "inst_off", "seg_frames"):
        assert labels(**{n: odd4}) == (A_.TSPN_EUNSUPPORTED, msg), n
    assert labels(spans=odd4) == labels(iou=odd2) == labels(out=odd2) == labels(span_count=odd2) == labels(inst_cols=odd2) \
        == (A_.TSPN_EUNSUPPORTED, msg)
    assert "bad sizes" in labels(P=-1, K=0)[1] and "K=0" in labels(K=0, G=17)[1] and "G=17" in labels(G=17, merge=5)[1]
    nothing = {n: null for n in names}
    assert labels(S=1, P=0, M=7, R=0, spans=null, span_count=null, inst_cols=null, out=null, **nothing)[0] == A_.TSPN_OK

    def loss(NT=5, T=3, D=4, S=1, P=6, G=2, K=7, pair_off=null, scratch=ok, nbytes=1 << 30, **ptr):
        g = lambda n: ptr.get(n, ok)   # noqa: E731
        rc = lib.tspn_span_predicate_loss_f32(g("feats"), NT, T, D, g("pairs"), pair_off, S, P, g("spans"), g("span_count"),
                                              g("span_labels"), G, g("cls_w"), g("cls_b"), K, g("q"), g("dv"), g("partials"),
                                              g("seg_rows"), scratch, nbytes, null)
        return rc, lib.tspn_last_error().decode()

    w = "tspn_span_predicate_loss_f32: "
    assert loss(T=0) == (A_.TSPN_EINVAL, w + "bad sizes NT=5 T=0 K=7 P=6 S=1")
    assert loss(P=-1)[0] == loss(NT=-1)[0] == loss(K=0)[0] == loss(S=-1)[0] == A_.TSPN_EINVAL
    assert loss(G=0) == (A_.TSPN_EINVAL, w + "G=0 span rows (needs 1 <= G)")
    assert loss(G=17) == (A_.TSPN_EUNSUPPORTED, w + "G=17 span rows (needs G <= 16)")
    assert loss(P=2 ** 30) == (A_.TSPN_EUNSUPPORTED,
                               w + "NT=5 T=3 K=7 P=1073741824 S=1 (needs T < 2^30, K < 2^20, S < 2^31, P*G < 2^31)")
    assert loss(T=2 ** 30)[0] == loss(K=2 ** 20)[0] == A_.TSPN_EUNSUPPORTED
    assert loss(S=2) == (A_.TSPN_EINVAL, w + "S=2 needs pair_off (null: one segment)")
    assert loss(S=0) == (A_.TSPN_EINVAL, w + "S=0 with P=6 pairs")
    assert loss(D=0) == (A_.TSPN_EINVAL, w + "D=0 features (needs D >= 1)")
    for n in ("feats", "pairs", "spans", "span_count", "span_labels", "cls_w", "q", "dv", "partials", "seg_rows"):
        assert loss(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    msg = w + "unaligned pointer (int64 and float64 operands need 8 bytes, fp32 and int32 ones 4)"
    for n in ("pairs", "spans", "partials", "seg_rows"):
        assert loss(**{n: odd4}) == (A_.TSPN_EUNSUPPORTED, msg), n
    for n in ("feats", "span_count", "span_labels", "cls_w", "cls_b", "q", "dv"):
        assert loss(**{n: odd2}) == (A_.TSPN_EUNSUPPORTED, msg), n
    assert loss(pair_off=odd4, S=2)[0] == loss(scratch=odd4)[0] == A_.TSPN_EUNSUPPORTED
    need = lib.tspn_span_predicate_workspace_bytes(5, 3, 4, 7)
    assert need > 0 and loss(nbytes=need - 1) == (A_.TSPN_EWORKSPACE, w + f"workspace {need - 1} < {need} bytes")
    assert loss(scratch=null)[0] == A_.TSPN_EWORKSPACE
    assert loss(S=0, P=0, **{n: null for n in ("pairs", "spans", "span_count", "span_labels", "q", "dv", "partials", "seg_rows")})[0] \
        == A_.TSPN_OK

    def finish(S=1, P=6, G=2, K=7, pair_off=null, partials=ok, seg_rows=ok, out=ok):
        rc = lib.tspn_span_predicate_loss_finish(partials, seg_rows, pair_off, S, P, G, K, out, null)
        return rc, lib.tspn_last_error().decode()

    w = "tspn_span_predicate_loss_finish: "
    assert finish(G=17) == (A_.TSPN_EUNSUPPORTED, w + "G=17 span rows (needs G <= 16)")
    assert finish(S=3) == (A_.TSPN_EINVAL, w + "S=3 needs pair_off (null: one segment)")
    assert finish(out=null) == finish(partials=null) == finish(seg_rows=null) == (A_.TSPN_EINVAL, w + "null pointer")
    assert finish(out=odd4) == finish(partials=odd4) == (A_.TSPN_EUNSUPPORTED,
                                                         w + "unaligned pointer (int64 and float64 operands need 8 bytes)")

    def grad(NT=5, T=3, P=6, G=2, K=7, scratch=ok, nbytes=1 << 30, **ptr):
        g = lambda n: ptr.get(n, ok)   # noqa: E731
        rc = lib.tspn_span_predicate_grad_f32(g("dv"), g("pairs"), g("spans"), g("span_count"), NT, T, P, G, K, g("db"), g("dG"),
                                              scratch, nbytes, null)
        return rc, lib.tspn_last_error().decode()

    w = "tspn_span_predicate_grad_f32: "
    assert grad(K=0) == (A_.TSPN_EINVAL, w + "bad sizes NT=5 T=3 K=0 P=6 S=1")
    assert grad(G=0) == (A_.TSPN_EINVAL, w + "G=0 span rows (needs 1 <= G)")
    for n in ("dv", "pairs", "spans", "span_count", "db", "dG"):
        assert grad(**{n: null}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    msg = w + "unaligned pointer (int64 and float64 operands need 8 bytes, fp32 and int32 ones 4)"
    assert grad(pairs=odd4) == grad(spans=odd4) == grad(scratch=odd4) == grad(dv=odd2) == grad(db=odd2) == grad(dG=odd2) \
        == grad(span_count=odd2) == (A_.TSPN_EUNSUPPORTED, msg)
    need = 5 * 4 * 14 * 8
    assert grad(nbytes=need - 1) == (A_.TSPN_EWORKSPACE, w + f"prefix_scratch {need - 1} < {need} bytes")
    assert grad(scratch=null) == (A_.TSPN_EWORKSPACE, w + f"prefix_scratch {1 << 30} < {need} bytes")


def test_op_model_and_dataset_layer_refuse_cpu_tensors_and_wrong_operands():
    import tspn_mi355x
    ops, ds = tspn_mi355x.ops, tspn_mi355x.dataset
    pairs, tid = torch.zeros((3, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    iou, insts = torch.zeros((4, 4)), torch.zeros((2, 5), dtype=torch.int64)
    spans, count, cols = torch.zeros((3, 2, 2), dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_labels(pairs, tid, iou, insts, 132, spans, count, cols, torch.zeros((1, 2), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_predicate_loss(torch.zeros((4, 3, 2)), pairs, spans, count, torch.zeros((3, 2, 5)), torch.zeros((5, 4)), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_predicate_grad(torch.zeros((6, 5)), pairs, spans, count, 4, 3)
    with pytest.raises(ValueError, match="span_labels=True needs"):
        ds._span_labels_wanted(True, 0, True)
    with pytest.raises(ValueError, match="span_labels=True needs"):
        ds._span_labels_wanted(True, 4, False)
    assert ds._span_labels_wanted(False, 0, False) is None and ds._span_labels_wanted(True, 4, True) is None
    assert tspn_mi355x.config.default_cfg().RELPN.DPN.POOL_GT_SPAN is False


# ------------------------------------------------------------------------------------------- the sources
def test_spancls_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_SC, "*.hip"))))
    assert in_source == {r["kernel"] for r in spancls_kernel_variants.VARIANTS} and len(in_source) == 6
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in spancls_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] in spancls_kernel_variants.ENTRIES and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_SC]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "spancls_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    text = open(os.path.join(CSRC_SC, "tspn_span_cls.hip")).read()
    consts = {m.group(1): m.group(2).strip() for m in re.finditer(r"constexpr int (\w+) = ([^;,]+)[;,]", text)}
    assert (consts["TILE"], consts["MAX_K"], consts["MAX_G"], consts["WAVES"]) == ("256", "512", "16", "4")
    assert (ref.TILE, ref.MAX_K, ref.MAX_G, ref.WAVES) == (256, 512, 16, 4)


def test_spancls_sources_are_built_and_carry_no_switches_memsets_atomics_or_environment_reads():
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
        assert not re.search(r"\bworkspace\b", code) and "_workspace_bytes" not in code
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in spancls_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k + "(" in n for k in names)}
    assert len(found) == len(names)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
