"""Span pooling and span relations on bf16 segments, the parts that need no GPU: the discipline of csrc/spanbf16/ (kernel
variant table, built sources, no probe blocks, no environment reads, the store-hazard lint), the new entry points in
header / binding / library, their refusals, and the float64 restatement (tests/span_bf16_reference.py) against the
committed oracle composition."""
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
import span_bf16_reference as ref
import spanbf16_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_SB = os.path.join(PKG, "csrc", "spanbf16")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_SB, "*.hip")) + glob.glob(os.path.join(CSRC_SB, "*.h")))
ENTRIES = {"tspn_pack_span_cls_bf16", "tspn_span_predicate_bf16", "tspn_span_predicate_bf16_workspace_bytes",
           "tspn_decode_span_relations_bf16", "tspn_decode_span_relations_bf16_workspace_bytes"}


def test_spanbf16_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_SB, "*.hip"))))
    assert in_source == {r["kernel"] for r in spanbf16_kernel_variants.VARIANTS} and len(in_source) == 5
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in spanbf16_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    # no new kernel outside the new directory: the two older tables stay complete
    older = global_kernels(sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) +
                                  glob.glob(os.path.join(PKG, "csrc", "relations", "*.hip"))))
    assert not (older & in_source)


def test_spanbf16_sources_are_built_and_carry_no_probe_blocks_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    assert os.path.join(PKG, "csrc", "tspn_span_pool.h") in build._headers()
    for f in NEW_SOURCES:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    # the clamp has one home, shared with the fp32 kernels
    assert "span_frames(" in open(os.path.join(PKG, "csrc", "tspn_span_pool.h")).read()
    assert all("tspn::span_frames(" in open(f).read() for f in hips)


def test_store_hazard_lint_passes_on_the_spanbf16_sources():
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] + hips,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert all(os.path.basename(f) in res.stdout for f in hips)


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in spanbf16_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k in n for k in names)}
    assert len(found) >= len(names)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)


def test_entry_points_are_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert {"pack_span_cls_bf16", "span_predicate_bf16", "decode_span_relations_bf16"} <= set(tspn_mi355x.ops.__all__)
    lib = abi.lib()
    # the cfg3 workspace as DESIGN.md 4c states it: float64 prefix sums [64, 901, 1024] + pooled rows [16128, 2048] bf16
    assert lib.tspn_span_predicate_bf16_workspace_bytes(64, 900, 1024, 132, 16128) == 64 * 901 * 1024 * 8 + 16128 * 2048 * 2
    assert lib.tspn_span_predicate_bf16_workspace_bytes(4, 9, 24, 5, 3) == 0             # D % 16
    small = lib.tspn_span_predicate_bf16_workspace_bytes(2, 3, 16, 5, 3)
    assert small >= 2 * 4 * 16 * 8 + 3 * 32 * 2 and small % 256 == 0
    rel = lib.tspn_decode_span_relations_bf16_workspace_bytes(2, 3, 5, 16, 6, 2, 9, 4)
    assert rel >= 6 * 6 * 16 * 8 + 24 * 32 * 2 + 24 * 9 * 4 + 3 * 24 * 4 * 4 and rel % 256 == 0
    assert lib.tspn_decode_span_relations_bf16_workspace_bytes(2, 3, 5, 16, 6, 17, 9, 4) == 0   # J > 16


def test_ops_refuse_cpu_tensors():
    import tspn_mi355x
    ops = tspn_mi355x.ops
    z = torch.zeros
    pairs, spans = z((3, 2), dtype=torch.int64), z((3, 2), dtype=torch.int64)
    f16, packed = z((4, 5, 16), dtype=torch.bfloat16), z((1, 1, 64, 8), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_span_cls_bf16(z(9, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_predicate_bf16(f16, pairs, spans, packed, z(9), 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_span_relations_bf16(f16, pairs.view(1, 3, 2), z((3, 2, 2), dtype=torch.int64), z(3, 2),
                                       z(3, dtype=torch.int64), packed, z(9), 9, z(1, 4, 35))


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any device work: the pointers are made-up addresses."""
    import tspn_mi355x
    A = tspn_mi355x._abi
    lib = A.lib()
    p = ctypes.c_void_p
    ok, odd, null = p(0x10000), p(0x10004), p(0)

    def pred(feats=ok, D=16, packed=ok, ws=ok, ws_bytes=1 << 30, pairs=ok, P=3, NT=4):
        rc = lib.tspn_span_predicate_bf16(feats, NT, 5, D, pairs, ok, P, packed, ok, 9, ok, ws, ws_bytes, null)
        return rc, lib.tspn_last_error().decode()

    rc, msg = pred(D=24)
    assert rc == A.TSPN_EUNSUPPORTED and "D % 16" in msg
    rc, msg = pred(feats=null)
    assert rc == A.TSPN_EINVAL and "null pointer" in msg
    rc, msg = pred(pairs=null)
    assert rc == A.TSPN_EINVAL and "null pointer" in msg
    rc, msg = pred(feats=odd)
    assert rc == A.TSPN_EUNSUPPORTED and "unaligned" in msg
    rc, msg = pred(packed=odd)
    assert rc == A.TSPN_EUNSUPPORTED and "unaligned" in msg
    need = lib.tspn_span_predicate_bf16_workspace_bytes(4, 5, 16, 9, 3)
    rc, msg = pred(ws_bytes=need - 1)
    assert rc == A.TSPN_EWORKSPACE and "workspace" in msg
    rc, msg = pred(ws=null)
    assert rc == A.TSPN_EWORKSPACE
    rc, msg = pred(ws=p(0x10010))
    assert rc == A.TSPN_EUNSUPPORTED and "unaligned" in msg
    assert pred(P=0, feats=null)[0] == A.TSPN_OK and pred(NT=0, feats=null)[0] == A.TSPN_OK     # nothing to launch

    def rel(feats=ok, D=16, K=9, J=2, M=16, R=4, P=6, ws_bytes=1 << 30, S=1):
        rc = lib.tspn_decode_span_relations_bf16(feats, S, 3, 5, D, ok, P, ok, ok, ok, J, ok, ok, K, ok, 35, R, M,
                                                 ok, ok, ok, ok, ok, ok, ok, ws_bytes, null)
        return rc, lib.tspn_last_error().decode()

    rc, msg = rel(D=8)
    assert rc == A.TSPN_EUNSUPPORTED and "D % 16" in msg
    rc, msg = rel(K=257)
    assert rc == A.TSPN_EUNSUPPORTED and "K=257" in msg
    rc, msg = rel(M=1025)
    assert rc == A.TSPN_EUNSUPPORTED and "topk_per_seg=1025" in msg
    rc, msg = rel(J=17)
    assert rc == A.TSPN_EUNSUPPORTED and "J=17" in msg
    rc, msg = rel(P=2 ** 24, J=16, R=8, K=8)
    assert rc == A.TSPN_EUNSUPPORTED and "candidates per segment" in msg
    rc, msg = rel(feats=null)
    assert rc == A.TSPN_EINVAL and "null pointer" in msg
    rc, msg = rel(feats=odd)
    assert rc == A.TSPN_EUNSUPPORTED and "unaligned" in msg
    need = lib.tspn_decode_span_relations_bf16_workspace_bytes(1, 3, 5, 16, 6, 2, 9, 4)
    rc, msg = rel(ws_bytes=need - 1)
    assert rc == A.TSPN_EWORKSPACE and "workspace" in msg
    assert rel(S=0, feats=null)[0] == A.TSPN_OK and rel(P=0, feats=null)[0] == A.TSPN_OK


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_the_committed_oracle_composition():
    """oracle.pair_gather -> oracle.rel_oi_pool(spans) on float64 -> oracle.bf16_round -> oracle.predicate_head_bf16, on a
    small case with every rule row: the pooled operand to the bit, the logits to one fp32 rounding (the oracle rounds
    its float64 sigmoid to fp32; its matrix product sums in another order)."""
    NT, T, D, K = 4, 9, 16, 5
    rs, f, w, b = ref.make_operands(11, NT, T, D, K)
    pairs = np.array([(s, o) for s in range(NT) for o in range(NT)] * 2, dtype=np.int64)
    spans = ref.draw_spans(rs, len(pairs), T)
    assert [tuple(r) for r in spans[:11]] == ref.rule_rows(T)
    pf, _ = oracle.pair_gather(torch.from_numpy(f), torch.zeros(NT, T, 4), torch.from_numpy(pairs))
    pooled = oracle.bf16_round(oracle.rel_oi_pool(pf.double(), torch.from_numpy(spans)).float())
    assert np.array_equal(pooled.numpy().view(np.uint32), ref.pooled_rows(f, pairs, spans).view(np.uint32))
    want = oracle.predicate_head_bf16(pooled, torch.from_numpy(w), torch.from_numpy(b)).numpy()
    got, z, S, frames = ref.span_predicate_ref(f, pairs, spans, w, b)
    assert np.abs(got - want.astype(np.float64)).max() <= 2.0 ** -24
    assert frames[0].tolist() == [0, T] and (frames[:, 0] < frames[:, 1]).all() and frames.min() >= 0 and frames.max() <= T
    assert (S > 0).all() and np.isfinite(z).all()


def test_float64_span_sums_of_the_generated_features_do_not_depend_on_the_order():
    """What contract (2) rests on: on the generator's features (bf16 values of magnitude 0 or >= 2^-12, |.| <= 1: whole
    multiples of 2^-19) every float64 prefix sum over T = 900 frames is exact, so forward prefix differences, reversed
    direct sums and integer arithmetic agree to the bit -- and so do the pooled bf16 operands."""
    NT, T, D = 3, 900, 32
    rs, f, _, _ = ref.make_operands(12, NT, T, D, 1)
    units = f.astype(np.float64) * 2.0 ** 19
    assert np.array_equal(units, np.round(units))
    exact = np.concatenate([np.zeros((NT, 1, D), np.int64), np.cumsum(units.astype(np.int64), axis=1)], axis=1)
    prefix = np.concatenate([np.zeros((NT, 1, D)), np.cumsum(f.astype(np.float64), axis=1)], axis=1)   # in frame order
    assert np.array_equal(prefix * 2.0 ** 19, exact.astype(np.float64))                   # 0 inexact prefix values
    a = rs.randint(0, T, size=400)
    e = np.minimum(a + 1 + rs.randint(0, T, size=400), T)
    trk = rs.randint(0, NT, size=400)
    bad = 0
    for i in range(400):
        fwd = prefix[trk[i], e[i]] - prefix[trk[i], a[i]]
        rev = np.cumsum(f[trk[i], a[i]:e[i]][::-1].astype(np.float64), axis=0)[-1]         # last frame first
        n = np.float64(e[i] - a[i])
        bad += int((ref.bf16((fwd / n).astype(np.float32)) != ref.bf16((rev / n).astype(np.float32))).sum())
        assert np.array_equal(fwd, rev)
    assert bad == 0
