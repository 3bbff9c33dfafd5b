"""The split-fp16 pair stage, the parts that need no GPU: the kernel table of csrc/pairf16/ against its sources and the
tests it names, the build lists, and the new entry points in header / binding / library."""
import ast
import ctypes
import glob
import importlib.util
import os
import re

import pairf16_kernel_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_PF = os.path.join(PKG, "csrc", "pairf16")
ENTRIES = {"tspn_heads_pairgrid_f16x3", "tspn_heads_pairgrid_f16x3_split_bytes", "tspn_heads_pairgrid_f16x3_set_force_exact"}


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


def test_pairf16_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_PF, "*.hip"))))
    assert in_source == {r["kernel"] for r in pairf16_kernel_variants.VARIANTS} and len(in_source) == 3
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in pairf16_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"


def test_pairf16_sources_are_built_without_switches_and_must_not_spill():
    spec = importlib.util.spec_from_file_location("_tspn_build_pf", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    hips = sorted(glob.glob(os.path.join(CSRC_PF, "*.hip")))
    assert hips and set(hips) <= set(build.sources())
    assert set(glob.glob(os.path.join(CSRC_PF, "*.h"))) <= set(build._headers())
    for f in hips:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert "hipMemsetAsync" not in text
    assert "heads_pair_f16x3_kernel" in build.NO_SPILL_KERNELS


def test_pairf16_entry_points_are_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    assert abi.ABI_VERSION == 7 and abi.lib().tspn_version() == 7
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert {"heads_pairgrid_f16x3", "heads_pairgrid_f16x3_split_bytes",
            "heads_pairgrid_f16x3_set_force_exact"} <= set(tspn_mi355x.ops.__all__)
    # answered without a device: a header of 256 bytes + 64 bytes per channel, nothing for what the entry refuses
    ops = tspn_mi355x.ops
    assert ops.heads_pairgrid_f16x3_split_bytes(4096, 12) == 256 + 64 * 4096
    assert ops.heads_pairgrid_f16x3_split_bytes(48, 12) == 0 and ops.heads_pairgrid_f16x3_split_bytes(64, 17) == 0
    assert ops.heads_pairgrid_f16x3_set_force_exact(0) == 0
