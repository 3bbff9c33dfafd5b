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


# ------------------------------------------------------------------------------------------- the vectorised plan check
def _random_table(rs):
    """A small table with bad rows: B in 1..3, N in 1..20, repeated rows, ids below 0, past B*N and in two videos."""
    B, N = int(rs.randint(1, 4)), int(rs.randint(1, 21))
    P = int(rs.randint(0, 60))
    pool = rs.randint(0, N, size=(max(int(rs.randint(1, 8)), 1), 2))                 # few distinct pairs: real chains
    table = pool[rs.randint(0, len(pool), size=P)] + N * rs.randint(0, B, size=(P, 1))
    bad = rs.rand(P) < 0.2
    table[bad] = rs.randint(-3, B * N + 3, size=(int(bad.sum()), 2))
    return B, N, table.astype(np.int64)


def test_fast_plan_check_accepts_what_the_walk_accepts():
    """On plans written in numpy from plan_np, chains in sorted and in shuffled order: every table the GPU tests score,
    the cross-video table, and 300 random small tables with bad rows pass both checks; the slots agree with plan_np."""
    cases = [(B, N, tab) for B, N, _, _, tab in ref.TABLES.values()] + [ref.CROSS_VIDEO]
    rs = np.random.RandomState(11)
    cases += [_random_table(rs) for _ in range(300)]
    for B, N, table in cases:
        for order in (None, rs):
            plan = ref.plan_arrays(table, B, N, rs=order)
            want = ref.check_plan(plan, table, B, N)
            slot = ref.check_plan_fast(plan, table, B, N)
            Np = (N + 15) // 16 * 16
            by_slot = {}
            for p, k in enumerate(slot.tolist()):
                if k >= 0:
                    by_slot.setdefault((k // (Np * Np), k // Np % Np, k % Np), set()).add(p)
            assert by_slot == want["chains"]


def _mutation_base():
    """B = 2, N = 5: video 0 has pairs (0,1) x3 [rows 0, 3, 6], (0,4) [1], (2,1) x2 [2, 7]; video 1 has (7,5) [4];
    row 5 joins two videos, row 8 is out of range."""
    table = np.array([[0, 1], [0, 4], [2, 1], [0, 1], [7, 5], [1, 7], [0, 1], [2, 1], [10, 3]], dtype=np.int64)
    plan = ref.plan_arrays(table, 2, 5)
    assert plan["head"][0, 0, 0] == 0 and plan["next"].tolist() == [3, -1, 7, 6, -1, -1, -1, -1, -1]
    assert plan["head"][0, 1, 0] == 2 and plan["head"][0, 0, 1] == 1 and plan["head"][1, 0, 0] == 4
    return table, plan


def _swap_list_entries(p):
    p["s_list"][0, [0, 1]] = p["s_list"][0, [1, 0]]


def _count_off_by_one(p):
    p["counts"][0, 1] += 1


def _row_dropped_from_a_chain(p):
    p["next"][0] = 6                    # 0 -> 6: row 3 is on no chain


def _row_linked_into_the_neighbouring_chain(p):
    p["next"][0], p["next"][7] = 6, 3   # (0,1): 0 -> 6; row 3 of (0,1) hangs at the end of the chain of (2,1): 2 -> 7 -> 3
    p["next"][3] = -1                   # every row is still pointed at exactly once, each slot pair has one terminal row


def _two_row_cycle_off_no_head(p):
    p["head"][0, 0, 0] = 0
    p["next"][0] = -1                   # head -> 0 ends at once
    p["next"][3], p["next"][6] = 6, 3   # 3 <-> 6: in-degree one each, one terminal row (0) in the slot pair


def _skipped_row_given_a_next(p):
    p["next"][5] = -1
    p["next"][8] = 1


def _head_on_an_unnamed_slot_pair(p):
    p["head"][0, 1, 1] = 1              # (2, 4) is in no row


MUTATIONS = [_swap_list_entries, _count_off_by_one, _row_dropped_from_a_chain, _row_linked_into_the_neighbouring_chain,
             _two_row_cycle_off_no_head, _skipped_row_given_a_next, _head_on_an_unnamed_slot_pair]


def test_fast_plan_check_accepts_the_mutation_base():
    table, plan = _mutation_base()
    ref.check_plan(plan, table, 2, 5)
    ref.check_plan_fast(plan, table, 2, 5)


@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda f: f.__name__.strip("_"))
def test_fast_plan_check_refuses_a_mutated_plan(mutate):
    """Each hand-made defect alone, on a plan both checks accept: the vectorised check must raise."""
    table, plan = _mutation_base()
    mutate(plan)
    with pytest.raises(AssertionError):
        ref.check_plan_fast(plan, table, 2, 5)


def test_fast_plan_check_catches_a_cycle_by_pointer_doubling_alone():
    """The two-row cycle passes every local test (in-degrees, slots, one terminal row): only the doubling sees it."""
    table, plan = _mutation_base()
    _two_row_cycle_off_no_head(plan)
    with pytest.raises(AssertionError, match="a cycle"):
        ref.check_plan_fast(plan, table, 2, 5)


def test_fast_plan_check_is_fast_at_the_sizes_the_gpu_tests_use():
    """N = 2048 with every tracklet and a million-row table of 380 pairs: the shapes the walk cannot do."""
    N = 2048
    table = np.stack([np.arange(N), (np.arange(N) * 7 + 1) % N], axis=1)
    plan = {"s_list": np.arange(N, dtype=np.int32)[None], "o_list": np.arange(N, dtype=np.int32)[None],
            "counts": np.array([[N, N]], np.int32), "head": np.full((1, N, N), -1, np.int32),
            "next": np.full((N,), -1, np.int32)}
    plan["head"][0, table[:, 0], table[:, 1]] = np.arange(N)
    ref.check_plan_fast(plan, table, 1, N)
    table, plan = ref.long_chain_table(), None
    assert table.shape == (256 * 4096 + 300, 2)
    # chains written by a stable sort: row i of a pair points at row i + 1 of the same pair
    _, slot, _, _ = ref.row_slots(table, 1, 20)
    order = np.argsort(slot, kind="stable")
    same = slot[order][1:] == slot[order][:-1]
    nxt = np.full(len(table), -1, np.int32)
    nxt[order[:-1][same]] = order[1:][same]
    first = order[np.concatenate([[True], ~same])]
    head = np.full(32 * 32, -1, np.int32)
    head[slot[first]] = first
    lists = np.zeros((1, 32), np.int32)
    lists[0, :20] = np.arange(20)
    plan = {"s_list": lists, "o_list": lists.copy(), "counts": np.array([[20, 20]], np.int32),
            "head": head.reshape(1, 32, 32), "next": nxt}
    ref.check_plan_fast(plan, table, 1, 20)
    nxt[order[-1]] = order[-3]                                 # a cycle at the end of a 2760-row chain
    with pytest.raises(AssertionError):
        ref.check_plan_fast(plan, table, 1, 20)
