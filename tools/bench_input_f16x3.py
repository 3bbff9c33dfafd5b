"""Input side of the split-fp16 F(6,3) conv alone: the two-pass transform + temporal mean kernel (form 1) against the fused
input kernels (form 2) at T = 150, D = 2048 and NT = 32 .. 512 -- device events round one call of
ops.wino63_f16x3_input, median and minimum of 30 after 5 warm-ups, in microseconds; also checks that the bytes agree at the
timed size.  One JSON line per NT; `python tools/bench_input_f16x3.py [OUT.json]` (profiles/r31/README.md)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tspn_mi355x as tspn  # noqa: E402

dev = torch.device("cuda", 0)
T, D, M = 150, 2048, 256
out = {"rows": []}
for NT in (32, 64, 128, 256, 512):
    g = torch.Generator(device="cpu").manual_seed(NT)
    x = torch.randn((NT, T, D), generator=g).to(dev)
    need = tspn._abi.lib().tspn_conv3_tc_wino63_f16x3_workspace_bytes(NT, T, D, M)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    res = {}
    row = {"NT": NT}
    for form in (1, 2):
        tspn.ops.wino63_f16x3_set_input_form(form)
        for _ in range(5):
            v, e, fbar, key = tspn.ops.wino63_f16x3_input(x, M, workspace=ws, hot=False)
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            v, e, fbar, key = tspn.ops.wino63_f16x3_input(x, M, workspace=ws, hot=False)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1000.0)
        ts.sort()
        row[f"form{form}_us_med"] = round(ts[len(ts) // 2], 1)
        row[f"form{form}_us_min"] = round(ts[0], 1)
        res[form] = (v.clone(), e.clone(), fbar.clone())
    tspn.ops.wino63_f16x3_set_input_form(0)
    row["same_bytes"] = all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(res[1], res[2]))
    out["rows"].append(row)
    print(json.dumps(row), flush=True)
    del x, ws, res, v, e, fbar
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
