"""The kernel variant table (tests/kernel_variants.py) stays equal to the HIP sources and points at tests that exist:
a new `__global__` kernel, a deleted one, a further overload of an existing name, or a deleted test named by the table
fails here without a GPU."""
import ast
import collections
import glob
import os
import re

import kernel_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc")

Definition = collections.namedtuple("Definition", "name template params file")

# fixed-width typedefs as the demangled name of a gfx950 kernel spells them
TYPEDEFS = {"int64_t": "long", "int32_t": "int", "int16_t": "short", "int8_t": "signed char", "uint64_t": "unsigned long",
            "uint32_t": "unsigned int", "uint16_t": "unsigned short", "uint8_t": "unsigned char", "size_t": "unsigned long"}
BUILTIN = ("int", "long", "short", "char", "float", "double", "unsigned", "bool")


def strip_comments(src):
    """C++ source without // and /* */ comments (string literals kept intact)."""
    pat = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\])*"|\'(?:\\.|[^\'\\])*\'', re.S)
    return pat.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", src)


def demangled_type(param):
    """One parameter declaration as a demangled kernel name spells its type:
    `const float* __restrict__ W` -> `float const*`, `int64_t M` -> `long`, `unsigned long long* __restrict__ hot` ->
    `unsigned long long*`."""
    tok = [w for w in param.replace("*", " * ").replace("&", " & ").split() if w != "__restrict__"]
    if len(tok) > 1 and re.fullmatch(r"[A-Za-z_]\w*", tok[-1]) and tok[-1] not in BUILTIN:
        tok = tok[:-1]                                   # the parameter's name
    k = next((i for i, w in enumerate(tok) if w in "*&"), len(tok))
    base, rest = [TYPEDEFS.get(w, w) for w in tok[:k]], tok[k:]
    const = "const" in base
    base = " ".join(w for w in base if w != "const")
    return base + (" const" if const else "") + "".join(rest)


def parameter_list(src, open_paren):
    """The parameter declarations between the parenthesis at `open_paren` and its match."""
    depth, start, out = 0, open_paren + 1, []
    for i in range(open_paren, len(src)):
        c = src[i]
        if c in "(<[":
            depth += 1
        elif c in ")>]":
            depth -= 1
            if depth == 0:
                out.append(src[start:i])
                return [s.strip() for s in out if s.strip()]
        elif c == "," and depth == 1:
            out.append(src[start:i])
            start = i + 1
    raise AssertionError("unbalanced parameter list")


def global_kernels():
    """One Definition per `__global__` function DEFINITION in csrc/*.hip: its name, whether it is a template, and its
    parameter types as a demangled kernel name spells them.  Overloads of one name are separate entries."""
    defs = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = strip_comments(open(path).read())
        for m in re.finditer(r"\b__global__\b", src):
            # `[template <...>] __global__ [__launch_bounds__(...)] [__attribute__((...))] void NAME(`
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            template = re.search(r"\btemplate\s*<[^;{}]*>\s*$", src[:m.start()]) is not None
            params = tuple(demangled_type(p) for p in parameter_list(src, m.end() + d.end() - 1))
            defs.append(Definition(d.group(1), template, params, os.path.basename(path)))
    return defs


def signature(d):
    return "(" + ", ".join(d.params) + ")"


def test_demangled_type_spelling():
    assert demangled_type("const float* __restrict__ W") == "float const*"
    assert demangled_type("int64_t M") == "long"
    assert demangled_type("unsigned long long* __restrict__ hot") == "unsigned long long*"
    assert demangled_type("_Float16* __restrict__ Vh") == "_Float16*"
    assert demangled_type("const int16_t* __restrict__ Wp") == "short const*"
    assert demangled_type("int") == "int"


def test_every_global_kernel_has_a_row_and_every_row_a_kernel():
    in_source = {d.name for d in global_kernels()}
    in_table = {r["kernel"] for r in kernel_variants.VARIANTS}
    assert len(in_source) > 50
    assert in_source - in_table == set(), "kernels without a row in tests/kernel_variants.py"
    assert in_table - in_source == set(), "rows naming a kernel that is not in csrc/*.hip"


def test_every_overload_of_a_name_has_rows_of_its_own():
    """A name defined n times needs rows that tell all n apart: a non-template overload by `inst` = its parameter
    types in parentheses (what distinguishes the overloads in a demangled kernel name), a template by rows with
    template arguments.  No row of such a name may be left matching any overload (inst None)."""
    by_name = collections.defaultdict(list)
    for d in global_kernels():
        by_name[d.name].append(d)
    overloaded = {n: ds for n, ds in by_name.items() if len(ds) > 1}
    assert {"pack_wino63_frag_kernel", "wino63_input_transform_kernel", "conv3_wino63_kernel"} <= set(overloaded)
    problems = []
    for name, ds in sorted(overloaded.items()):
        insts = [r["inst"] for r in kernel_variants.VARIANTS if r["kernel"] == name]
        plain = {signature(d) for d in ds if not d.template}
        if len({(d.template, signature(d)) for d in ds}) != len(ds):
            problems.append(f"{name}: two definitions with one signature")
        for d in ds:
            if d.template:
                if not any(i is not None and not i.startswith("(") for i in insts):
                    problems.append(f"{name} (template, {d.file}): no row with template arguments")
            elif signature(d) not in insts:
                problems.append(f"{name}{signature(d)} ({d.file}): no row with this parameter list as inst")
        for i in insts:
            if i is None:
                problems.append(f"{name}: a row with inst None cannot tell its {len(ds)} definitions apart")
            elif i.startswith("(") and i not in plain:
                problems.append(f"{name}{i}: no such overload in csrc/*.hip")
    for r in kernel_variants.VARIANTS:           # a parameter list on a name that is defined once must be that definition's
        if r["inst"] is not None and r["inst"].startswith("(") and r["kernel"] not in overloaded:
            if [signature(d) for d in by_name.get(r["kernel"], ())] != [r["inst"]]:
                problems.append(f"{r['kernel']}{r['inst']}: not the signature in csrc/*.hip")
    assert not problems, "\n".join(problems)


def test_check_tool_tells_the_overloads_apart_in_a_kernel_trace(tmp_path, capsys):
    """tools/check_kernel_variants.py on a `*_kernel_stats.csv` with the names as rocprofv3 prints them (the kernels
    with a `_Float16` parameter stay mangled): complete -> 0; the split contraction filtered out -> 1 and named,
    although the fp32 contraction of the same identifier is in the trace."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_kernel_variants", os.path.join(ROOT, "tools", "check_kernel_variants.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    split_conv = "_ZN12_GLOBAL__N_119conv3_wino63_kernelEPKDF16_PKiPKsPKfPfS8_iiiilliiiiii"
    names = [
        split_conv,
        "_ZN12_GLOBAL__N_129wino63_input_transform_kernelEPKfPDF16_PiiiilllPy",
        "(anonymous namespace)::pack_wino63_frag_kernel(float const*, long, long, long, short*)",
        "(anonymous namespace)::pack_wino63_frag_kernel(float const*, long, long, long, float*)",
        "(anonymous namespace)::wino63_input_transform_kernel(float const*, float*, int, int, int, long, long, long, "
        "unsigned long long*)",
        "void (anonymous namespace)::conv3_wino63_kernel<true>(float const*, float const*, float const*, float*, int, int, "
        "int, int, long, long, int, int, int, int, int, int)",
        "void (anonymous namespace)::conv3_wino63_kernel<false>(float const*, float const*, float const*, float*, int, int, "
        "int, int, long, long, int, int, int, int, int, int)",
    ]
    by_name = collections.defaultdict(list)
    for d in global_kernels():
        by_name[d.name].append(d)
    split_sig = [signature(d) for d in by_name["conv3_wino63_kernel"] if not d.template]
    assert tool.demangle(split_conv) == "conv3_wino63_kernel" + split_sig[0]
    files = ["tests/test_gpu_wino63.py", "tests/test_gpu_wino63_f16x3_range.py"]

    def run(kernels):
        path = tmp_path / "run_kernel_stats.csv"
        with open(path, "w") as f:
            f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage"\n')
            for k in kernels:
                f.write(f'"{k}",3,300,100.0,1.0\n')
        rc = tool.main(["check", str(path)] + [os.path.join(ROOT, p) for p in files])
        return rc, capsys.readouterr().out

    rc, out = run(names)
    assert rc == 0, out
    rc, out = run([n for n in names if n != split_conv])
    assert rc == 1 and "NOT LAUNCHED conv3_wino63_kernel(_Float16 const*" in out and out.count("NOT LAUNCHED") == 1, out
    rc, out = run([n for n in names if "<false>" not in n])
    assert rc == 1 and "NOT LAUNCHED conv3_wino63_kernel<false>" in out and out.count("NOT LAUNCHED") == 1, out


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
