"""The bf16 pair-list stage, the parts that need no GPU: the discipline of csrc/pairlist/ (kernel variant table, built
sources, no probe blocks, no environment reads, the store-hazard lint), the new entry points in header / binding /
library, and the numpy restatement of the plan on hand-written tables."""
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

import pairlist_kernel_variants
import pairlist_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_PL = os.path.join(PKG, "csrc", "pairlist")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_PL, "*.hip")) + glob.glob(os.path.join(CSRC_PL, "*.h"))) + \
    [os.path.join(PKG, "csrc", "tspn_heads_pair_bf16.h")]
ENTRIES = {"tspn_pair_plan_i32", "tspn_heads_pairlist_bf16", "tspn_heads_pairlist_bf16_workspace_bytes",
           "tspn_forward_fused_bf16_pairs", "tspn_forward_fused_bf16_pairs_workspace_bytes"}


def global_kernels(paths):
    """Names of every `__global__` function defined in the given sources (the parse of test_kernel_variant_table.py)."""
    names = set()
    for path in paths:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b__global__\b", src):
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_pairlist_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_PL, "*.hip"))))
    assert in_source == {r["kernel"] for r in pairlist_kernel_variants.VARIANTS} and len(in_source) == 3
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in pairlist_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    # both forms the launcher can pick are rows of the table
    assert {i for k, i in seen if k == "heads_pairlist_bf16_kernel"} == {"4, 8, 2", "8, 16, 2"}


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tspn_build_pl", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_pairlist_sources_are_built_and_carry_no_probe_blocks_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert all(os.path.exists(f) for f in NEW_SOURCES)
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert "heads_pairlist_bf16_kernel" in build.NO_SPILL_KERNELS


def test_store_hazard_lint_passes_on_the_pairlist_sources():
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] + hips,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert all(os.path.basename(f) in res.stdout for f in hips)


def test_entry_points_are_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    assert abi.ABI_VERSION == 7
    assert re.search(r"#define\s+TSPN_ABI_VERSION\s+7\b", open(abi.HEADER_PATH).read())
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert abi.lib().tspn_version() == 7
    assert {"pair_plan", "heads_pairlist_bf16", "forward_fused_bf16"} <= set(tspn_mi355x.ops.__all__)
    # limits answered without a device: no workspace for what the entry refuses
    lib = abi.lib()
    assert lib.tspn_heads_pairlist_bf16_workspace_bytes(1, 2049, 10) == 0
    assert lib.tspn_heads_pairlist_bf16_workspace_bytes(1, 16, 2 ** 31) == 0
    small = lib.tspn_heads_pairlist_bf16_workspace_bytes(2, 17, 5)
    assert small >= 2 * 32 * 32 * 4 + 2 * 2 * 32 * 4 + 5 * 4 and small % 256 == 0


def test_ops_refuse_cpu_tensors():
    import tspn_mi355x
    ops, abi = tspn_mi355x.ops, tspn_mi355x._abi
    z = torch.zeros
    pairs = z((3, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        ops.pair_plan(pairs, 1, 4)
    assert isinstance(e.value, abi.TspnError) and e.value.code == abi.TSPN_EUNSUPPORTED
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        ops.heads_pairlist_bf16(z(4, 5, 64), pairs, 1, 4, z((4, 16, 8), dtype=torch.bfloat16), z(12), 12)
    assert isinstance(e.value, abi.TspnError) and e.value.code == abi.TSPN_EUNSUPPORTED
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.forward_fused_bf16(z((4, 5, 16), dtype=torch.bfloat16), pairs, 1, 4, z((3, 2, 64, 8), dtype=torch.bfloat16),
                               z(32), z((4, 16, 8), dtype=torch.bfloat16), z(12), z(132, 32), z(132), canonical_pairs=False)


# ------------------------------------------------------------------------------------------- the numpy plan
def test_plan_restatement_on_hand_written_tables():
    # one video, N = 5: a duplicate, an (s, s) row, a subject-only and an object-only tracklet
    pairs = [[3, 1], [0, 1], [3, 1], [4, 4], [0, 4]]
    p = ref.plan_np(pairs, 1, 5)
    assert p["s_list"] == [[0, 3, 4]] and p["o_list"] == [[1, 4]] and p["counts"].tolist() == [[3, 2]]
    assert p["chains"] == {(0, 1, 0): {0, 2}, (0, 0, 0): {1}, (0, 2, 1): {3}, (0, 0, 1): {4}}
    # three videos of N = 4, none for the middle one; a cross-video row, a negative and a too-large id are in no chain
    pairs = [[9, 8], [1, 2], [1, 5], [-1, 2], [2, 12], [11, 8], [1, 2]]
    p = ref.plan_np(pairs, 3, 4)
    assert p["s_list"] == [[1], [], [1, 3]] and p["o_list"] == [[2], [], [0]]
    assert p["counts"].tolist() == [[1, 1], [0, 0], [2, 1]]
    assert p["chains"] == {(2, 0, 0): {0}, (0, 0, 0): {1, 6}, (2, 1, 0): {5}}
    assert ref.plan_np(np.zeros((0, 2), np.int64), 2, 3)["chains"] == {}


def test_check_plan_accepts_a_correct_plan_and_refuses_wrong_ones():
    """`check_plan` (what the GPU test holds the device plan to) on a plan written by hand, chains in either order."""
    pairs = np.array([[2, 0], [0, 2], [2, 0], [5, 1]], dtype=np.int64)          # N = 3, B = 1: row 3 is out of range
    Np = 16
    good = {"s_list": np.zeros((1, Np), np.int32), "o_list": np.zeros((1, Np), np.int32),
            "counts": np.array([[2, 2]], np.int32), "head": np.full((1, Np, Np), -1, np.int32),
            "next": np.array([-1, -1, 0, -1], np.int32)}
    good["s_list"][0, :2] = [0, 2]
    good["o_list"][0, :2] = [0, 2]
    good["head"][0, 1, 0] = 2          # chain of (2, 0): row 2 -> row 0
    good["head"][0, 0, 1] = 1          # chain of (0, 2): row 1
    ref.check_plan(good, pairs, 1, 3)
    other = {k: v.copy() for k, v in good.items()}
    other["head"][0, 1, 0], other["next"][0], other["next"][2] = 0, 2, -1         # the same chain, the other order
    ref.check_plan(other, pairs, 1, 3)
    for key, idx, val in (("head", (0, 1, 1), 3), ("next", (2,), -1), ("counts", (0, 0), 3), ("s_list", (0, 1), 1),
                          ("head", (0, 5, 5), 0)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][idx] = val
        with pytest.raises(AssertionError):
            ref.check_plan(bad, pairs, 1, 3)


def test_tables_of_the_reference_module():
    assert ref.canonical_table(2, 3).tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1],
                                                  [3, 4], [3, 5], [4, 3], [4, 5], [5, 3], [5, 4]]
    assert ref.among([4, 1], base=10).tolist() == [[14, 11], [11, 14]]
    y = torch.arange(2 * 1 * 4, dtype=torch.float32).reshape(2, 1, 4) - 3.0      # C = 2
    hw, hb = torch.tensor([[1.0, 2.0]]), torch.tensor([0.5])
    out = ref.heads_list_ref64(y, [[0, 1], [1, 1]], hw, hb)
    # (0, 1): relu([-3, -2] + [3, 4]) = [0, 2] -> 4.5; (1, 1): relu([1, 2] + [3, 4]) = [4, 6] -> 16.5
    assert out.shape == (2, 1, 1) and out.flatten().tolist() == [4.5, 16.5]
