"""tests/fp32_reference.py without a device: three fp32 summation orders, with rounded and with unrounded products, stay inside
the budget the GPU tests hold the fp32 kernels to, on every kind and every contraction depth tests/test_gpu_fp32_bound.py uses,
and are bit-equal to float32(ref64) on every exact generator (which proves the generators' exactness condition); five planted
defects leave the budget and break the exact cases wherever fp32_reference's docstring says they are visible; the emulations
of the mean kernels' orders lie inside the mean's and the sum's intervals and are exact on the exact cases at every T."""
import numpy as np
import pytest

import fp32_reference as fr

# (B, T, Cin, M): every Cin of the GPU file (CONV3_VARIANTS, the tile-map case, the channels-last depths, full depth), two or
# more sequences so that a tap can cross a boundary
CONV_SHAPES = ((2, 5, 8, 4), (2, 5, 24, 8), (3, 3, 12, 4), (2, 4, 37, 4), (2, 5, 16, 8), (2, 5, 32, 4), (2, 5, 48, 8), (2, 3, 2048, 4))
HEADS_C = (21, 16, 24, 48, 2048)
# (P, F, K) of test_predicate_head_split_k_edges and the baseline's; emulated on the first rows / columns at the full shape's splits
LINEAR_ROWS = ((10944, 40, 289), (5, 4500, 10), (70, 63, 17), (9, 129, 144), (9, 127, 145), (3, 2047, 289), (130, 289, 5),
               (70, 11070, 132), (5, 6100, 10))
NORM_ROWS = ((33, 3 + 40 * 70 + 5, 21, 3, 40, 70), (70, 11070, 132, 70, 1000, 8))
MEAN_SHAPES = ((3, 7, 8), (2, 1, 4), (4, 33, 132), (5, 150, 64))
MEAN_T = (1, 3, 7, 33, 150)
VARIANTS = tuple((o, f) for o in fr.ORDERS for f in (False, True))


def ratio(err, bnd):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))))


def same_bits(got, want):
    return np.array_equal(fr.bits(fr.fold_zero(got)), fr.bits(fr.fold_zero(want)))


def test_budgets_in_units_of_u_s():
    assert fr.K_of(3 * 8, fr.K_CONV) == 33 and fr.K_of(3 * 2048, fr.K_CONV) == 6153 and fr.K_of(21, fr.K_HEADS) == 23.5
    assert fr.splits_of(5, 4500, 10) == 64 and fr.kps_of(4500, 64) == 96 and fr.linear_K(4500, 64) == 2 * (4 + 24 + 66) + 1
    assert fr.splits_of(70, 11070, 132) == 64 and fr.splits_of(70, 63, 17) == 1
    assert len(fr.split_table(*NORM_ROWS[0])) > 64 and len({b for _, _, b in fr.split_table(*NORM_ROWS[0])}) == 71
    for row in NORM_ROWS:
        tab = fr.split_table(*row)
        assert tab[0][0] == 0 and tab[-1][1] == row[1] and all(a[1] == b[0] for a, b in zip(tab, tab[1:]))
        for s, e, blk in tab:       # a slice never straddles a block
            assert blk < 0 or (row[3] + blk * row[4] <= s and e <= row[3] + (blk + 1) * row[4])


# ------------------------------------------------------------------------------------------------ conv
def conv_drop(kind, x, w):
    """(column, channel) to drop or double: the last channel's centre tap; the last chunk's hot channel on `hot_channel`, the
    largest share on `wide` (fp32_reference's docstring says why)."""
    Cin = x.shape[2]
    c = Cin - 1 - (Cin % 2 if kind == "cancelling" else 0)      # an odd last channel has no partner there: its weight is 0
    if kind == "hot_channel":
        c = int(fr.hot_index(Cin)[-1])
    elif kind == "wide":
        c = int(np.argmax(np.abs(w[:, :, 1]).max(0) * np.abs(x).max((0, 1))))
    return fr.conv_col(Cin, c, 1)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", fr.PLAIN_KINDS)
def test_conv_orders_stay_inside_the_budget_and_defects_leave_it(tspn, kind, shape):
    x, w, b = fr.make_conv_case(tspn.hashrng, kind, *shape)
    Cin = shape[2]
    for relu in (False, True):
        ref, bnd = fr.conv_ref64(x, w, b, relu), fr.conv_budget(x, w, b)
        assert bool(np.isfinite(ref).all()) and bool((bnd > 0).all()) and ref.size > 0
        for order, fused in (VARIANTS if Cin <= 48 else (("blocks", False), ("pairwise", False), ("sequential", True))):
            err = np.abs(fr.conv_emulate(x, w, b, relu, order=order, fused=fused).astype(np.float64) - ref)
            assert bool((err <= bnd).all()), (kind, shape, order, fused, ratio(err, bnd))
    ref, bnd = fr.conv_ref64(x, w, b), fr.conv_budget(x, w, b)
    col = conv_drop(kind, x, w)
    seen = {}
    for name, kw in (("drop", {"drop": col}), ("double", {"double": col}), ("leak", {"leak": True}), ("bias_shift", {"bias_shift": True}),
                     ("trunc19", {"trunc_chunk": (Cin - 1) // 16})):
        seen[name] = ratio(np.abs(fr.conv_emulate(x, w, b, **kw).astype(np.float64) - ref), bnd)
    print(f"conv {kind} {shape}: " + ", ".join(f"{k} {v:.2f}" for k, v in seen.items()))
    assert seen["leak"] > 1.0                                       # a third of S at a sequence's first or last frame: every kind
    if Cin <= 48 or kind == "hot_channel":
        assert seen["drop"] > 1.0 and seen["double"] > 1.0
    if kind in ("unit", "large", "hot_channel", "cancelling") and Cin <= 48:
        assert seen["bias_shift"] > 1.0


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("which", fr.EXACT_KINDS)
def test_exact_conv_cases_are_exact_in_every_order_and_break_under_every_defect(tspn, which, shape):
    B, T, Cin, M = shape
    for qa, qw in (fr.Q_PAIRS if Cin <= 48 else fr.Q_PAIRS[:2]):
        x, w, b, units, zero_rows = fr.exact_conv_case(tspn.hashrng, which, B, T, Cin, M, qa, qw)
        for relu in (False, True):
            want = fr.conv_ref64(x, w, b, relu).astype(np.float32)
            assert bool(np.isfinite(want).all()) and bool(((want == 0) | (np.abs(want) >= fr.SMALLEST_NORMAL)).all())
            for order, fused in (VARIANTS if Cin <= 48 else (("blocks", False), ("pairwise", False))):
                assert same_bits(fr.conv_emulate(x, w, b, relu, order=order, fused=fused), want), (which, shape, qa, qw, order, fused)
        want = fr.conv_ref64(x, w, b).astype(np.float32)
        if which == "zeros":
            assert len(zero_rows) == 3 and bool(np.signbit(x[x == 0]).any()) and bool((x == 0).any())
            assert np.array_equal(want[:, zero_rows[0]], np.broadcast_to(b[zero_rows[0]], want[:, 0].shape))
            unit = np.float32(2.0 ** (qa + qw))
            assert bool((want[:, zero_rows[1]] == -unit).all()) and bool((want[:, zero_rows[2]] == 0).all())
            r = fr.conv_ref64(x, w, b, True)
            assert bool((r > 0).any()) and bool((r == 0).any())     # the ReLU with both signs in front of it
        else:
            assert float(np.abs(np.ldexp(x[:, :, -1].astype(np.float64), -qa)).min()) >= fr.WIDE_LO
            assert not same_bits(fr.conv_emulate(x, w, b, trunc_chunk=(Cin - 1) // 16), want), "trunc19 is invisible"
        col = fr.conv_col(Cin, 0, 1)
        for kw in ({"drop": col}, {"double": col}, {"leak": True}, {"bias_shift": True}):
            assert not same_bits(fr.conv_emulate(x, w, b, **kw), want), (which, shape, qa, qw, kw)
    print(f"conv {which} {shape}: {units} units")


# ------------------------------------------------------------------------------------------------ heads, pair grid
def heads_forms(tspn, case, R):
    """[(name, h fp32 [P, C, T])]: mode 0, mode 1 on an index table with repeats and an ia == ib row, the pair grid of one video."""
    a, b, bias = case[:3]
    ia, ib = np.array([0, 1, 1, 2, 0]) % R, np.array([0, 2, 0, 2, 1]) % R
    return (("mode0", fr.heads_act(0, a, ia)), ("mode1", fr.heads_act(1, a, ia, b, ib, bias)),
            ("grid", fr.pairgrid_act(np.concatenate([a, b], 1), 1, R)))


@pytest.mark.parametrize("C", HEADS_C)
@pytest.mark.parametrize("kind", fr.KINDS)
def test_heads_orders_stay_inside_the_budget_and_defects_leave_it(tspn, kind, C):
    R, T, H = 3, 3, 12
    case = fr.make_heads_case(tspn.hashrng, kind, R, C, T, H)
    w, bh = case[3], case[4]
    for name, h in heads_forms(tspn, case, R):
        if kind == "relu_edge":
            if name == "mode0":
                continue
            dead = float((h == 0).mean())
            assert 0.3 < dead < 0.7 and float(h.max()) < 2.0 ** -8 * float(np.abs(case[0]).max()), (name, dead)
        ref, bnd = fr.heads_ref64(h, w, bh), fr.heads_budget(h, w, bh)
        assert bool(np.isfinite(ref).all()) and bool((bnd > 0).all()) and bool((h != 0).any())
        for order, fused in (VARIANTS if C <= 48 else (("blocks", False), ("pairwise", False), ("sequential", True))):
            err = np.abs(fr.heads_emulate(h, w, bh, order=order, fused=fused).astype(np.float64) - ref)
            assert bool((err <= bnd).all()), (kind, C, name, order, fused, ratio(err, bnd))
        c = C - 1 - (C % 2 if kind == "cancelling" else 0)
        if kind == "hot_channel":
            c = int(fr.hot_index(C)[-1])
        elif kind == "wide":
            c = int(np.argmax(np.abs(w).max(0) * np.abs(h).max((0, 2))))
        seen = {n: ratio(np.abs(fr.heads_emulate(h, w, bh, **kw).astype(np.float64) - ref), bnd)
                for n, kw in (("drop", {"drop": c}), ("double", {"double": c}), ("bias_shift", {"bias_shift": True}),
                              ("trunc19", {"trunc_chunk": (C - 1) // 16}))}
        print(f"heads {name} {kind} C={C}: " + ", ".join(f"{k} {v:.2f}" for k, v in seen.items()))
        assert seen["drop"] > 1.0 and seen["double"] > 1.0          # S / C is above (C / 2 + 13) u S at every C here
        if kind in ("unit", "large", "relu_edge") or (kind in ("hot_channel", "cancelling") and C <= 48):
            assert seen["bias_shift"] > 1.0


@pytest.mark.parametrize("C", HEADS_C)
@pytest.mark.parametrize("which", fr.EXACT_KINDS)
def test_exact_heads_cases_are_exact_in_every_order_and_break_under_every_defect(tspn, which, C):
    R, T = 3, 3
    for H in (1, 12, 16):
        for qa, qw in (fr.Q_PAIRS if C <= 48 else fr.Q_PAIRS[:2]):
            case = fr.exact_heads_case(tspn.hashrng, which, R, C, T, H, qa, qw)
            w, bh, units, zero_rows = case[3:]
            for name, h in heads_forms(tspn, case, R):
                want = fr.heads_ref64(h, w, bh).astype(np.float32)
                assert bool(np.isfinite(want).all()) and bool(((want == 0) | (np.abs(want) >= fr.SMALLEST_NORMAL)).all())
                mh = np.ldexp(h.astype(np.float64), -qa)
                assert np.array_equal(mh, np.round(mh)), "an activation is not an integer"
                for order, fused in (VARIANTS if C <= 48 else (("blocks", False), ("pairwise", False))):
                    assert same_bits(fr.heads_emulate(h, w, bh, order=order, fused=fused), want), (which, C, H, name, order, fused)
                if zero_rows:
                    assert np.array_equal(want[:, zero_rows[0]], np.broadcast_to(bh[zero_rows[0]], want[:, 0].shape))
                if which == "zeros" and name == "mode1":
                    pre = (case[0][[0, 1, 1, 2, 0]].astype(np.float64) + case[1][[0, 2, 0, 2, 1]] + case[2][None, :, None]) * 2.0 ** -qa
                    assert bool((pre == 0).any()) and bool((pre == -1).any()) and bool((pre > 0).any()) and bool((pre < -1).any())
                if which == "plain":
                    assert not same_bits(fr.heads_emulate(h, w, bh, trunc_chunk=(C - 1) // 16), want) or H == 1
                if H > 1:
                    for kw in ({"drop": 0}, {"double": 0}, {"bias_shift": True}):
                        assert not same_bits(fr.heads_emulate(h, w, bh, **kw), want), (which, C, H, name, kw)
    print(f"heads {which} C={C}: {units} units")


# ------------------------------------------------------------------------------------------------ split-K GEMM, block-L1
@pytest.mark.parametrize("row", LINEAR_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_linear_orders_stay_inside_the_budget_and_exact_cases_are_exact(tspn, row):
    P, F, K = row
    splits = fr.splits_of(P, F, K)
    p, k = min(P, 4), min(K, 6)
    for kind in fr.PLAIN_KINDS:
        x, w, b = fr.make_linear_case(tspn.hashrng, kind, p, F, k)
        ref, bnd = fr.linear_ref64(x, w, b), fr.linear_budget(x, w, b, splits)
        assert bool(np.isfinite(ref).all()) and bool((bnd > 0).all())
        for order, fused in (VARIANTS if F <= 300 else (("blocks", False), ("pairwise", False))):
            err = np.abs(fr.linear_emulate(x, w, b, splits, order, fused).astype(np.float64) - ref)
            assert bool((err <= bnd).all()), (kind, row, order, fused, ratio(err, bnd))
        c = F - 1 - (F % 2 if kind == "cancelling" else 0)
        if kind == "hot_channel":
            c = int(fr.hot_index(F)[-1])
        elif kind == "wide":
            c = int(np.argmax(np.abs(w).max(0) * np.abs(x).max(0)))
        if splits == 1:     # the planted defects go through contract_emulate's arguments: one slice
            seen = {n: ratio(np.abs(fr.linear_emulate(x, w, b, 1, **kw).astype(np.float64) - ref), bnd)
                    for n, kw in (("drop", {"drop": c}), ("double", {"double": c}))}
            print(f"linear {kind} {row}: " + ", ".join(f"{n} {v:.2f}" for n, v in seen.items()))
            assert seen["drop"] > 1.0 and seen["double"] > 1.0
        # a skipped last slice (the reduce kernel stopping one short): where the last slice holds eight columns or more
        if splits > 1 and (splits - 1) * fr.kps_of(F, splits) + 8 <= F and kind not in ("wide", "hot_channel"):
            err = np.abs(fr.linear_emulate(x[:, :(splits - 1) * fr.kps_of(F, splits)], w[:, :(splits - 1) * fr.kps_of(F, splits)], b,
                                           splits - 1).astype(np.float64) - ref)
            assert ratio(err, bnd) > 1.0, (kind, row)
    for which in fr.EXACT_KINDS:
        for qa, qw in fr.Q_PAIRS[:4]:
            x, w, b, units, zero_rows = fr.exact_linear_case(tspn.hashrng, which, p, F, k, qa, qw)
            want = fr.linear_ref64(x, w, b).astype(np.float32)
            for order in ("blocks", "pairwise"):
                assert same_bits(fr.linear_emulate(x, w, b, splits, order), want), (which, row, qa, qw, order)
            assert not same_bits(fr.linear_emulate(x, w, b, splits, drop=0), want) or splits > 1
            if zero_rows:
                assert np.array_equal(want[:, zero_rows[0]], np.broadcast_to(b[zero_rows[0]], want[:, 0].shape))


@pytest.mark.parametrize("row", NORM_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_block_l1_orders_stay_inside_the_budget_and_exact_cases_are_exact(tspn, row):
    P, F, K, first, block, nblocks = row
    norm = (first, block, nblocks)
    # (`subnormal` is left out on purpose: a block norm summed from subnormal |x| has no RELATIVE rounding bound, which is what
    # the budget of sum / L1 stands on; `cancelling` differs from `unit` only by a scale once a block is normalised)
    for kind in ("unit", "large", "tiny", "hot_channel", "wide"):
        x, w, b = fr.make_linear_case(tspn.hashrng, kind, P, F, K)
        if kind == "tiny":
            b = b * np.float32(2.0 ** 10)          # the normalised operand is O(1 / block) whatever x's scale: keep the bias beside it
        x[4, first + block:first + 2 * block] = 0
        sl = (slice(0, 6), slice(None))
        ref = fr.norm_ref64(x, w, b, *norm)[:6, :5]
        bnd = fr.norm_budget(x, w, b, *norm)[:6, :5]
        for order in ("blocks", "pairwise"):
            # the table depends on (P, K): emulate the first rows and columns against the full problem's table
            got = norm_rows(x[:6], w[:5], b[:5], row, order)
            err = np.abs(got.astype(np.float64) - ref)
            print(f"norm {kind} {row} {order}: max err / budget = {ratio(err, bnd):.3f}")
            assert bool((err <= bnd).all()), (kind, row, order, ratio(err, bnd))
    for which in fr.EXACT_KINDS:
        for qa, qw in ((0, 0), (-1, 7), (-100, 100), (100, -100), (50, 0)):
            x, w, b, units, zero_rows = fr.exact_norm_case(tspn.hashrng, which, P, F, K, *norm, qa, qw)
            assert bool((np.abs(x[P // 2, first + min(1, nblocks - 1) * block:][:block]) == 0).all())
            want = fr.norm_ref64(x, w, b, *norm).astype(np.float32)
            assert bool(np.isfinite(want).all()) and bool((want != 0).any())
            rows = slice(P // 2 - 2, P // 2 + 2)
            for order in ("blocks", "pairwise"):
                assert same_bits(norm_rows(x[rows], w[:5], b[:5], row, order), want[rows, :5]), (which, row, qa, qw, order)
        print(f"norm {which} {row}: {units} units")


def norm_rows(x, w, b, row, order):
    """norm_emulate of a few rows / columns with the slice table of the full (P, K)."""
    P, F, K, first, block, nblocks = row
    full = fr.split_table
    try:
        fr.split_table = lambda *_: full(P, F, K, first, block, nblocks)
        return fr.norm_emulate(x, w, b, first, block, nblocks, order=order)
    finally:
        fr.split_table = full


# ------------------------------------------------------------------------------------------------ mean, sum
@pytest.mark.parametrize("shape", MEAN_SHAPES + tuple((3, T, 8) for T in MEAN_T), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", fr.MEAN_KINDS)
def test_mean_and_sum_emulations_lie_in_their_intervals(tspn, kind, shape):
    x = fr.make_mean_case(tspn.hashrng, kind, *shape)
    T = shape[1]
    for mean, (lo, hi) in ((True, fr.mean_interval(x)), (False, fr.sum_interval(x))):
        assert bool((lo <= hi).all())
        for form in ("td", "ct", "pairwise"):
            got = fr.mean_emulate(x, form, mean)
            assert bool(((lo <= got) & (got <= hi)).all()), (kind, shape, form, mean)
        if T == 1:
            assert np.array_equal(fr.bits(fr.fold_zero(lo)), fr.bits(fr.fold_zero(x[:, 0]))) and np.array_equal(lo, hi)
        # a divisor rounded to a power of two (T = 150 -> 128) and a dropped last frame leave the interval
        if mean and T in (3, 7, 33, 150) and kind != "cancelling":
            bad = fr.mean_emulate(x, "td", False) / np.float32(2.0 ** round(np.log2(T)))
            assert not bool(((lo <= bad) & (bad <= hi)).all())
        if T > 1 and kind in ("unit", "large", "tiny"):
            bad = fr.mean_emulate(x[:, :-1], "td", False) / np.float32(T) if mean else fr.mean_emulate(x[:, :-1], "td", False)
            assert not bool(((lo <= bad) & (bad <= hi)).all())
    if kind == "cancelling" and T % 2 == 0:
        assert float(np.abs(x.astype(np.float64).mean(1)).max()) < 0.1 * float(np.abs(x).mean())


@pytest.mark.parametrize("T", MEAN_T)
def test_exact_mean_and_sum_cases(tspn, T):
    inexact = 0
    for q in fr.Q_MEAN:
        x, want_mean, want_sum = fr.exact_mean_case(tspn.hashrng, 3, T, 40, q)
        assert bool((x != 0).any()) and bool(np.signbit(x[x == 0]).any())
        for form in ("td", "ct", "pairwise"):
            assert same_bits(fr.mean_emulate(x, form, True), want_mean), (T, q, form)
            assert same_bits(fr.mean_emulate(x, form, False), want_sum), (T, q, form)
        lo, hi = fr.mean_interval(x)
        assert bool(((lo <= want_mean) & (want_mean <= hi)).all())
        inexact += int((want_mean.astype(np.float64) * T != want_sum.astype(np.float64)).sum())
    if T not in (1,):
        assert inexact > 20, inexact            # the division rounds: the reference's one rounding is what is compared
