#!/usr/bin/env python3
"""Check a profiled test run against the kernel variant tables (tests/kernel_variants.py for csrc/*.hip,
tests/eval_kernel_variants.py for csrc/eval/*.hip).

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python -m pytest FILE... -q -m gpu
    python tools/check_kernel_variants.py OUT/.../run_kernel_stats.csv FILE...   (or OUT/.../run_results.db)

For every table row that names a test in one of the FILEs, the row's kernel instantiation must appear among the
launched kernels (named the way tools/kernel_stats.py names them).  Lists every such row that never ran and exits
1 if there is one."""
import csv
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from kernel_stats import short  # noqa: E402

import eval_kernel_variants  # noqa: E402
import kernel_variants  # noqa: E402


def split(name):
    """'heads_kernel<0, true>' -> ('heads_kernel', '0,true'); 'pair_index_kernel' -> ('pair_index_kernel', None)."""
    base, _, args = name.partition("<")
    return base, (re.sub(r"\s+", "", args[:-1]) if args else None)


def launched(stats):
    """{(kernel, template args): calls} from a `*_kernel_stats.csv` or a rocpd `*_results.db` (as kernel_stats.py)."""
    if stats.endswith(".db"):
        cur = sqlite3.connect(stats).cursor()
        rows = cur.execute("select name, count(*) from kernels group by name").fetchall()
    else:
        rows = [(r["Name"], int(r["Calls"])) for r in csv.DictReader(open(stats))]
    calls = {}
    for name, n in rows:
        key = split(short(name))
        calls[key] = calls.get(key, 0) + n
    return calls


def rel(path):
    return os.path.relpath(os.path.abspath(path), ROOT).replace(os.sep, "/")


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    calls = launched(argv[1])
    files = {rel(f) for f in argv[2:]}
    checked, missing = 0, []
    for r in kernel_variants.VARIANTS + eval_kernel_variants.VARIANTS:
        if not any(node.partition("::")[0] in files for node in r["tests"]):
            continue
        checked += 1
        inst = None if r["inst"] is None else re.sub(r"\s+", "", r["inst"])
        n = sum(c for (base, args), c in calls.items() if base == r["kernel"] and (inst is None or args == inst))
        if n == 0:
            missing.append(r)
    print(f"{checked} table rows name tests in {', '.join(sorted(files))}; {checked - len(missing)} launched, "
          f"{len(missing)} never ran")
    for r in missing:
        name = r["kernel"] + ("" if r["inst"] is None else f"<{r['inst']}>")
        print(f"  NOT LAUNCHED {name}  (entry {r['entry']}; when {r['when']})")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
