"""The kernel variant table (tests/kernel_variants.py) stays equal to the HIP sources and points at tests that exist:
a new `__global__` kernel, a deleted one, or a deleted test named by the table fails here without a GPU."""
import ast
import glob
import os
import re

import kernel_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc")


def strip_comments(src):
    """C++ source without // and /* */ comments (string literals kept intact)."""
    pat = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\])*"|\'(?:\\.|[^\'\\])*\'', re.S)
    return pat.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", src)


def global_kernels():
    """Names of every `__global__` function defined in csrc/*.hip."""
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = strip_comments(open(path).read())
        for m in re.finditer(r"\b__global__\b", src):
            # `__global__ [__launch_bounds__(...)] [__attribute__((...))] void NAME(`
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_every_global_kernel_has_a_row_and_every_row_a_kernel():
    in_source = global_kernels()
    in_table = {r["kernel"] for r in kernel_variants.VARIANTS}
    assert len(in_source) > 50
    assert in_source - in_table == set(), "kernels without a row in tests/kernel_variants.py"
    assert in_table - in_source == set(), "rows naming a kernel that is not in csrc/*.hip"


def test_rows_are_complete_and_unique():
    seen = set()
    for r in kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen, f"duplicate row {key}"
        seen.add(key)
        assert r["entry"] and r["when"] and r["align"], key
        assert r["tests"], f"{key}: no test reaches it"


def test_every_named_test_exists():
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    missing = []
    for r in kernel_variants.VARIANTS:
        for node in r["tests"]:
            path, _, name = node.partition("::")
            if name.split("[")[0] not in defined.get(path, ()):
                missing.append(f"{r['kernel']}<{r['inst']}>: {node}")
    assert not missing, "table rows name tests that do not exist:\n" + "\n".join(missing)
