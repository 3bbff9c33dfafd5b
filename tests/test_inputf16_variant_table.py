"""The fused input side of the split-fp16 F(6,3) conv, the parts that need no GPU: the kernel table of csrc/inputf16/
against its sources and the tests it names, the build lists, the shared header, the new entry points in header / binding /
library, and the form-selection function."""
import ast
import ctypes
import glob
import importlib.util
import os
import re

import inputf16_kernel_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_IN = os.path.join(PKG, "csrc", "inputf16")
ENTRIES = {"tspn_conv3_tc_wino63_f16x3_input", "tspn_conv3_tc_wino63_f16x3_input_form",
           "tspn_conv3_tc_wino63_f16x3_set_input_form"}
SHARED = ("wino63_load_sextet", "wino63_bt", "wino63_absmax_own_frames", "wino63_hot_publish", "split_exponent",
          "wino63_split_f16")


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


def test_inputf16_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_IN, "*.hip"))))
    assert in_source == {r["kernel"] for r in inputf16_kernel_variants.VARIANTS} and len(in_source) == 2
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in inputf16_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"


def test_inputf16_sources_are_built_without_switches():
    spec = importlib.util.spec_from_file_location("_tspn_build_in", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    hips = sorted(glob.glob(os.path.join(CSRC_IN, "*.hip")))
    assert hips and set(hips) <= set(build.sources())
    assert set(glob.glob(os.path.join(CSRC_IN, "*.h"))) <= set(build._headers())
    for f in hips:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert "hipMemsetAsync" not in text
    # one object per source base name: the new file must not shadow another directory's
    names = [os.path.basename(s) for s in build.sources()]
    assert len(names) == len(set(names))


def test_transform_pieces_have_one_definition_in_the_shared_header():
    """The fp32 transform, the two-pass split transform and the fused input kernels use ONE body of each piece."""
    header = open(os.path.join(PKG, "csrc", "tspn_wino63_input.h")).read()
    users = [os.path.join(PKG, "csrc", "tspn_wino63.hip")] + sorted(glob.glob(os.path.join(CSRC_IN, "*.hip")))
    for name in SHARED:
        define = re.compile(r"__device__\s+__forceinline__\s+\w+\s+" + name + r"\s*\(")
        assert len(define.findall(header)) == 1, name
        for path in users:
            text = open(path).read()
            assert '#include "tspn_wino63_input.h"' in text
            assert not define.search(text), f"{os.path.basename(path)} has its own {name}"
    for name in ("wino63_bt", "wino63_split_f16", "split_exponent", "wino63_hot_publish"):
        for path in users:
            assert re.search(r"\b" + name + r"\s*\(", open(path).read()), f"{os.path.basename(path)} does not use {name}"


def test_inputf16_entry_points_are_declared_bound_and_exported():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    assert abi.ABI_VERSION == 7 and abi.lib().tspn_version() == 7
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert {"wino63_f16x3_input", "wino63_f16x3_input_form", "wino63_f16x3_set_input_form"} <= set(tspn_mi355x.ops.__all__)
    ops = tspn_mi355x.ops
    assert ops.wino63_f16x3_set_input_form(0) == 0
    assert abi.lib().tspn_conv3_tc_wino63_f16x3_set_input_form(3) == abi.TSPN_EINVAL
    assert ops.wino63_f16x3_set_input_form(0) == 0                # a refused value changes nothing


def test_input_form_is_a_pure_function_of_the_shape_and_the_cu_count():
    """Fused where the scan workgroups (one per tracklet, Cin / 4 threads) are large and numerous enough: Cin in
    [1024, 2048] and at least one tracklet per two CUs.  No device is asked."""
    import tspn_mi355x
    form = tspn_mi355x.ops.wino63_f16x3_input_form
    assert form(512, 150, 2048, 256) == 1                         # the benchmark's shape: 16 videos of 32 tracklets
    assert form(128, 150, 2048, 256) == 1 and form(127, 150, 2048, 256) == 0
    assert form(32, 150, 2048, 256) == 0 and form(64, 150, 2048, 256) == 0          # one and two videos
    assert form(32, 150, 2048, 64) == 1                           # the same launch fills a smaller chip
    assert form(512, 150, 1024, 256) == 1 and form(512, 150, 992, 256) == 0
    assert form(512, 150, 2080, 256) == 0 and form(512, 150, 4096, 256) == 0       # beyond the register-resident limit
    assert form(512, 1, 2048, 256) == 1                           # T does not enter
    assert form(0, 150, 2048, 256) == 0 and form(512, 150, 2048, 0) == 0 and form(512, 0, 2048, 256) == 0
    assert form(512, 150, 2044, 256) == 0                         # Cin % 8
