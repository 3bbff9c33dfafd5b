"""The references of tests/test_gpu_conv2d_edges.py checked on the CPU: the case table covers what it claims, the exact
operands are exact (every value an integer below 256, about half of the pre-activation values negative, so a ReLU or a
dropped sign shows), and the float64 reference of the real-valued cases is four times closer to a float32 one than the
bound the kernels are held to (figures: profiles/r16/README.md)."""
import collections

import numpy as np
import torch

import conv2d_edge_cases as cc

F32_ATOL = 2e-5                     # the suite's bound for the fp32 conv kernels
F32_REFERENCE_SHARE = 0.25          # a float32 CPU conv2d must stay within this share of it
BF16_REFERENCE_CAP = 0.0025         # share of outputs whose float32 and float64 references round to different bf16 values:
                                    # a quarter of the 1 % the kernel is allowed (one output where a quarter is less than one)


def test_case_table_holds_what_each_kernel_row_needs():
    n = collections.Counter(c.form for c in cc.CASES)
    print(dict(n), len(cc.CASES))
    assert len(set(cc.CASES)) == len(cc.CASES) == 145
    rows = collections.defaultdict(list)        # kernel row -> its cases
    for c in cc.CASES:
        rows[(c.form,) + (cc.bf16_kernel(c) if c.form == "bf16" else ())].append(c)
    assert set(rows) == {("generic",), ("frag",), ("cin4",), ("bf16", 1, False), ("bf16", 1, True), ("bf16", 2, False),
                         ("bf16", 2, True)}
    for row, cs in rows.items():
        gs = {c.g for c in cs}
        if row[-1] is True:                     # the linear-range form: 3x3 / 1 / 1 only
            assert gs == set(cc.G_RNG) and {c.nb for c in cs} == {cc.NB, cc.NB_MANY}
            continue
        assert any(g.KH != g.KW for g in gs), row
        assert any(g.KH * g.KW > 32 for g in gs) and any(g.KH * g.KW == 64 for g in gs), row
        assert any(g.stride == 3 for g in gs), row
        assert any(g.pad > max(g.KH, g.KW) // 2 or (g.pad and g.KH * g.KW == 1) for g in gs), row   # all-padding windows
        assert any(g.KH > g.H or g.KW > g.W for g in gs), row
    assert {c.g.KH * c.g.KW for c in rows[("cin4",)]} >= {1, 3, 4, 6, 9, 25, 49, 64}
    assert any(c.g.KH * c.g.KW == 1 and c.cout % 64 == 0 for c in rows[("bf16", 1, False)])       # the launcher's mi = 1 rule
    assert any(c.cout == 320 for c in rows[("bf16", 2, False)]) and any(c.cout == 320 for c in rows[("bf16", 2, True)])


def test_exact_operands_stay_exact_and_signed():
    neg = tot = 0
    worst = 0.0
    for c in cc.CASES:
        x, w, b, r = cc.operands(c, "exact")
        for a in (x, w, b) + (() if r is None else (r,)):
            assert (a == np.round(a)).all() and np.array_equal(cc.r16(a), a)
        pre = cc.reference(x, w, c.g, b, r)
        assert bool((pre == pre.round()).all())
        worst = max(worst, float(pre.abs().max()))
        assert float(pre.abs().max()) <= cc.EXACT_LIMIT, cc.case_id(c)
        neg += int((pre < 0).sum())
        tot += pre.numel()
    print(f"largest |reference| {worst}, negative pre-activations {neg / tot:.3f} of {tot}")
    # symmetric operands: P(negative) = (1 - P(zero)) / 2, and P(zero) <= 1/7 (a window wholly in the padding: the sum of
    # two integers uniform in [-3, 3])
    assert 0.40 <= neg / tot <= 0.50


def test_float64_reference_is_four_times_closer_than_the_kernels_bound():
    dev_worst, share_worst = (0.0, None), (0.0, None)
    for c in cc.CASES:
        x, w, b, r = cc.operands(c, "real")
        ref = cc.reference(x, w, c.g, b, r)
        ref32 = cc.reference(x, w, c.g, b, r, dtype=torch.float32)
        if c.form == "bf16":
            share = float((ref32.to(torch.bfloat16) != ref.float().to(torch.bfloat16)).double().mean())
            share_worst = max(share_worst, (share, cc.case_id(c)))
            assert share * ref.numel() <= max(1.0, BF16_REFERENCE_CAP * ref.numel()), (cc.case_id(c), share)
        else:
            dev = float((ref32.double() - ref).abs().max())
            dev_worst = max(dev_worst, (dev, cc.case_id(c)))
            assert dev <= F32_REFERENCE_SHARE * F32_ATOL, (cc.case_id(c), dev)
    print(f"float32 - float64 reference: {dev_worst[0]:.3e} ({dev_worst[1]}); bf16 roundings that differ: "
          f"{share_worst[0]:.3%} ({share_worst[1]})")
