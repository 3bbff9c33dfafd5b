#!/usr/bin/env python3
"""Check a profiled test run against the kernel variant tables (tests/kernel_variants.py for csrc/*.hip,
tests/eval_kernel_variants.py for csrc/eval/*.hip, tests/relations_kernel_variants.py for csrc/relations/*.hip,
tests/pairlist_kernel_variants.py for csrc/pairlist/*.hip, tests/spanbf16_kernel_variants.py for csrc/spanbf16/*.hip,
tests/spanloss_kernel_variants.py for csrc/spanloss/*.hip, tests/spansample_kernel_variants.py for csrc/spansample/*.hip,
tests/pairlabels_kernel_variants.py for csrc/pairlabels/*.hip, tests/spanmatch_kernel_variants.py for csrc/spanmatch/*.hip,
tests/evalobj_kernel_variants.py for csrc/evalobj/*.hip, tests/spancls_kernel_variants.py for csrc/spancls/*.hip,
tests/detect_kernel_variants.py for csrc/detect/*.hip, tests/link_kernel_variants.py for csrc/link/*.hip).

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python -m pytest FILE... -q -m gpu
    python tools/check_kernel_variants.py OUT/.../run_kernel_stats.csv FILE...   (or OUT/.../run_results.db)

For every table row that names a test in one of the FILEs, the row's kernel instantiation must appear among the
launched kernels: the identifier, and the template arguments or (for an overloaded name) the parameter types of the
demangled kernel name.  rocprofv3 leaves names it cannot demangle (a `_Float16` parameter) mangled; those are decoded
here.  Lists every such row that never ran and exits 1 if there is one."""
import csv
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_kernel_variants  # noqa: E402
import eval_kernel_variants  # noqa: E402
import evalobj_kernel_variants  # noqa: E402
import kernel_variants  # noqa: E402
import link_kernel_variants  # noqa: E402
import pairlabels_kernel_variants  # noqa: E402
import pairlist_kernel_variants  # noqa: E402
import relations_kernel_variants  # noqa: E402
import spanbf16_kernel_variants  # noqa: E402
import spancls_kernel_variants  # noqa: E402
import spanloss_kernel_variants  # noqa: E402
import spanmatch_kernel_variants  # noqa: E402
import spansample_kernel_variants  # noqa: E402

BUILTIN = {"v": "void", "b": "bool", "c": "char", "a": "signed char", "h": "unsigned char", "s": "short",
           "t": "unsigned short", "i": "int", "j": "unsigned int", "l": "long", "m": "unsigned long", "x": "long long",
           "y": "unsigned long long", "f": "float", "d": "double", "DF16_": "_Float16", "DF16b": "__bf16", "Dh": "_Float16"}


def demangle_parameters(enc, subs):
    """Parameter types of an Itanium-mangled function whose parameters are builtin types, pointers and const:
    'PKDF16_PKiPfS3_l' -> ['_Float16 const*', 'int const*', 'float*', 'float*', 'long'].  None for anything else.
    `subs`: the substitution candidates the name itself made (its namespace)."""
    subs, out, i = list(subs), [], 0

    def one(i):
        """(type, next index); every compound type (pointer, const-qualified) becomes a substitution candidate."""
        if enc.startswith("P", i):
            t, i = one(i + 1)
            subs.append(t + "*")
            return t + "*", i
        if enc.startswith("K", i):
            t, i = one(i + 1)
            subs.append(t + " const")
            return t + " const", i
        if enc.startswith("S", i):
            m = re.match(r"S([0-9A-Z]*)_", enc[i:])
            k = 0 if m.group(1) == "" else int(m.group(1), 36) + 1
            return subs[k], i + m.end()
        for code in sorted(BUILTIN, key=len, reverse=True):
            if enc.startswith(code, i):
                return BUILTIN[code], i + len(code)
        raise ValueError(enc[i:])

    try:
        while i < len(enc):
            t, i = one(i)
            out.append(t)
    except (ValueError, IndexError, AttributeError):
        return None
    return out


def demangle(name):
    """`_ZN12_GLOBAL__N_1<len><identifier>E<parameters>` (a non-template kernel in the anonymous namespace) or
    `_Z<len><identifier><parameters>` as the demangler would print it; any other name unchanged."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name) or re.match(r"_Z(\d+)", name)
    if not m:
        return name
    n, rest = int(m.group(1)), name[m.end():]
    ident, enc = rest[:n], rest[n:]
    nested = name.startswith("_ZN")
    if nested and not enc.startswith("E"):
        return name
    enc = re.sub(r"\.kd$", "", enc[1:] if nested else enc)
    params = demangle_parameters(enc, ["(anonymous namespace)"] if nested else [])
    if params is None or not re.fullmatch(r"[A-Za-z_]\w*", ident):
        return name
    return f"{ident}({', '.join(params)})"


def parse(name):
    """Kernel name of a trace -> (identifier, template arguments or None, parameter types or None), without spaces:
    'void (anonymous namespace)::heads_kernel<0, true>(float const*, int)' -> ('heads_kernel', '0,true',
    '(floatconst*,int)')."""
    name = demangle(name)
    m = re.search(r"(?:\(anonymous namespace\)::)?([A-Za-z_][A-Za-z0-9_]*)(<(?:[^<>(]|<[^<>(]*>)*>)?(\(.*\))", name)
    if not m:
        return name[:60], None, None
    squeeze = lambda s: re.sub(r"\s+", "", s)   # noqa: E731
    return m.group(1), (squeeze(m.group(2)[1:-1]) if m.group(2) else None), squeeze(m.group(3))


def launched(stats):
    """{(kernel, template args, parameter types): calls} from a `*_kernel_stats.csv` or a rocpd `*_results.db`."""
    if stats.endswith(".db"):
        cur = sqlite3.connect(stats).cursor()
        rows = cur.execute("select name, count(*) from kernels group by name").fetchall()
    else:
        rows = [(r["Name"], int(r["Calls"])) for r in csv.DictReader(open(stats))]
    calls = {}
    for name, n in rows:
        key = parse(name)
        calls[key] = calls.get(key, 0) + n
    return calls


def row_calls(r, calls):
    """Launches of the kernel a table row means: by template arguments, by parameter types ("(...)"), or any (None)."""
    inst = None if r["inst"] is None else re.sub(r"\s+", "", r["inst"])
    n = 0
    for (base, args, params), c in calls.items():
        if base != r["kernel"]:
            continue
        if inst is None or (params == inst if inst.startswith("(") else args == inst):
            n += c
    return n


def rel(path):
    return os.path.relpath(os.path.abspath(path), ROOT).replace(os.sep, "/")


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    calls = launched(argv[1])
    files = {rel(f) for f in argv[2:]}
    checked, missing = 0, []
    for r in (kernel_variants.VARIANTS + eval_kernel_variants.VARIANTS + relations_kernel_variants.VARIANTS
              + pairlist_kernel_variants.VARIANTS + spanbf16_kernel_variants.VARIANTS
              + spanloss_kernel_variants.VARIANTS + spansample_kernel_variants.VARIANTS
              + pairlabels_kernel_variants.VARIANTS + spanmatch_kernel_variants.VARIANTS
              + evalobj_kernel_variants.VARIANTS + spancls_kernel_variants.VARIANTS
              + detect_kernel_variants.VARIANTS + link_kernel_variants.VARIANTS):
        if not any(node.partition("::")[0] in files for node in r["tests"]):
            continue
        checked += 1
        if row_calls(r, calls) == 0:
            missing.append(r)
    print(f"{checked} table rows name tests in {', '.join(sorted(files))}; {checked - len(missing)} launched, "
          f"{len(missing)} never ran")
    for r in missing:
        inst = r["inst"]
        name = r["kernel"] + ("" if inst is None else inst if inst.startswith("(") else f"<{inst}>")
        print(f"  NOT LAUNCHED {name}  (entry {r['entry']}; when {r['when']})")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
