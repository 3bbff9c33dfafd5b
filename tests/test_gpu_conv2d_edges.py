"""The four implicit-GEMM conv2d forms off ResNet's own geometries (csrc/tspn_roi.hip, csrc/tspn_roi_bf16.hip), each
against torch.nn.functional.conv2d in float64 on the CPU on the same operands.

Table (tests/conv2d_edge_cases.py; checked on the CPU by tests/test_conv2d_edge_cases_host.py): 17 geometries -- KH != KW,
49 and 64 taps, stride 3 and unread rows / columns, windows wholly in the padding and kernels larger than the map, the
five 3x3 / 1 / 1 maps on which the bf16 linear-range form wraps rows (1x1, 1x5, 5x1, 2x2, 3x2), a 2x2 kernel -- at NB = 3,
three of them also at NB = 70 (one 128-pixel tile spans 8 to 128 images, the last tile is partial).  Every geometry runs
with the smallest channel pair of a form (two for bf16: Cout = 32 and Cout = 64), every other channel pair with one
linear-range geometry and one other (bf16 with Cout % 64 == 0: also a 1x1).  145 cases:

    kernel row (tests/kernel_variants.py)        cases  KH != KW  tap >= 32  all padding  stride 3  one term  non-finite
    conv2d_nhwc_kernel<16>             generic     34      x          x           x          x         x          x
    conv2d_nhwc_frag_kernel<false>     frag        26      x          x           x          x         x          x
    conv2d_nhwc_frag_kernel<true>      cin4        30      x          x           x          x         x          x
    conv2d_nhwc_bf16_kernel<1, false>  bf16        21      x          x           x          x         x          x
    conv2d_nhwc_bf16_kernel<2, false>  bf16        14      x          x           x          x         x          x
    conv2d_nhwc_bf16_kernel<1, true>   bf16        10      -          -           -          -         x          x
    conv2d_nhwc_bf16_kernel<2, true>   bf16        10      -          -           -          -         x          x
    (the linear-range form exists for 3x3 / stride 1 / pad 1 only: 9 taps, and every window holds its centre pixel)

Tests: 145 exact + 145 real-valued + 54 epilogue + 7 guard-band + 20 non-finite + 12 refusals = 383 small cases; a case is
one or two launches on a map of at most 70 x 2 x 2 or 3 x 9 x 10 pixels and one float64 conv2d on the CPU.

Tolerances are the suite's own (tests/test_gpu_roi_head.py): fp32 atol 2e-5; bf16 |ref| 2^-8 + 3e-5 with more than 99 % of
the outputs the correctly rounded float64 value; the registers-direct form equals the LDS form bit for bit.  The exact
operands (small integers, 48 weights of +-1 per output channel) make every partial sum an integer below 2^24 and every
result one below 256, so all four forms must give the float64 reference bit for bit, whatever their order of summation."""
import numpy as np
import pytest
import torch

import conv2d_edge_cases as cc
from sentinel_buffers import assert_untouched, assert_written_inside_only, held, refused

pytestmark = pytest.mark.gpu

F32_ATOL = 2e-5


def by_id(cases):
    return dict(argvalues=cases, ids=[cc.case_id(c) for c in cases])


def out_dtype(form):
    return torch.bfloat16 if form == "bf16" else torch.float32


def assert_bits_equal(got, ref, what):
    """`got` (device, fp32 or bf16) equals the float64 reference bit for bit (the reference is exact in both types)."""
    want = ref.to(got.dtype)
    assert bool((want.double() == ref).all()), f"{what}: the reference is not exact in {got.dtype}"
    assert tuple(got.shape) == tuple(want.shape), what
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    same = got.cpu().view(bits) == want.view(bits)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} outputs differ, first at {torch.nonzero(~same)[0].tolist()}"


def assert_close(form, got, ref, what, where=None):
    """The suite's bounds for real-valued operands, on the elements `where` (all by default)."""
    got = got.cpu().double()
    assert tuple(got.shape) == tuple(ref.shape), what
    if where is None:
        where = torch.ones_like(ref, dtype=torch.bool)
    g, r = got[where], ref[where]
    err = (g - r).abs()
    if form == "bf16":
        tol = r.abs() * 2.0 ** -8 + 3e-5
        exact = float((g == r.float().to(torch.bfloat16).double()).double().mean()) if r.numel() else 1.0
        print(f"{what}: largest excess over the bound {float((err - tol).max()):.3e}, correctly rounded {exact:.4%}")
        assert bool((err <= tol).all()), f"{what}: {float((err - tol).max())}"
        assert exact > 0.99, f"{what}: {exact}"
    else:
        print(f"{what}: largest deviation {float(err.max()):.3e}")
        assert bool((err <= F32_ATOL).all()), f"{what}: {float(err.max())}"


# ============================================================================================ 1. exact operands
@pytest.mark.parametrize("case", **by_id(cc.CASES))
def test_exact_operands_give_the_float64_reference_bit_for_bit(tspn, device, case):
    """Integer operands, bias + residual (bias only for the stem form), no ReLU: negative values stay visible."""
    x, w, b, r = cc.operands(case, "exact")
    ref = cc.reference(x, w, case.g, b, r)
    got = cc.run(tspn, device, case.form, x, w, case.g, b, r)
    assert got.dtype == out_dtype(case.form)
    assert_bits_equal(got, ref, cc.case_id(case))


# ============================================================================================ 2. real-valued operands
@pytest.mark.parametrize("case", **by_id(cc.CASES))
def test_real_operands_within_the_suites_bounds(tspn, device, case):
    """x, residual uniform in [-1, 1), weights and bias normal(0.1), bias + residual, no ReLU; the registers-direct form
    equals the LDS form on the same operands bit for bit."""
    x, w, b, r = cc.operands(case, "real")
    ref = cc.reference(x, w, case.g, b, r)
    got = cc.run(tspn, device, case.form, x, w, case.g, b, r)
    assert_close(case.form, got, ref, cc.case_id(case))
    if case.form == "frag":
        assert torch.equal(got.view(torch.int32), cc.run(tspn, device, "generic", x, w, case.g, b, r).view(torch.int32))


# ============================================================================================ 3. epilogue terms
EPI_GEOMS = [cc.Geom(3, 3, 1, 1, 3, 2), cc.Geom(2, 3, 1, 1, 5, 4)]          # linear-range and not
EPI_ROWS = [("generic", 16, 4), ("frag", 16, 32), ("cin4", 1, 32), ("bf16", 64, 32), ("bf16", 64, 64)]
EPI_TERMS = [(True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True),
             (True, True, True)]
EPI_CASES = [(cc.Case(f, ci, co, g, cc.NB), terms) for f, ci, co in EPI_ROWS for g in EPI_GEOMS for terms in EPI_TERMS
             if not (f == "cin4" and terms[1])]


@pytest.mark.parametrize("case,terms", EPI_CASES, ids=[cc.case_id(c) + "-" + "".join(n for n, on in zip(("bias", "res", "relu"), tm) if on)
                                                       for c, tm in EPI_CASES])
def test_each_epilogue_term_on_its_own(tspn, device, case, terms):
    """bias, residual and ReLU are three independent branches: each alone, each pair with ReLU, all three; exact operands,
    bit equality.  (The stem form has no residual.)"""
    bias, res, relu = terms
    x, w, b, r = cc.operands(case, "exact")
    b, r = (b if bias else None), (r if res else None)
    ref = cc.reference(x, w, case.g, b, r, relu)
    if relu:
        assert 0.25 < float((ref == 0).double().mean()) < 0.75              # the ReLU cuts and lets through
    got = cc.run(tspn, device, case.form, x, w, case.g, b, r, relu)
    assert_bits_equal(got, ref, cc.case_id(case))


# ============================================================================================ 4. guard bands
GUARD_CASES = [cc.Case("generic", 16, 36, *cc.WIDE_RNG), cc.Case("frag", 16, 160, *cc.WIDE_RNG), cc.Case("cin4", 3, 96, *cc.WIDE_RNG),
               cc.Case("bf16", 64, 96, *cc.WIDE_RNG), cc.Case("bf16", 64, 96, *cc.WIDE_TAPS),
               cc.Case("bf16", 64, 320, *cc.WIDE_RNG), cc.Case("bf16", 64, 320, *cc.WIDE_TAPS)]


@pytest.mark.parametrize("case", **by_id(GUARD_CASES))
def test_every_output_written_and_nothing_else(tspn, device, case):
    """Through the C ABI into a sentinel-filled buffer: a partial last pixel tile (280 = 2 x 128 + 24 or 45 pixels) and
    a partial row tile (Cout = 36, 160, 96 of 128-row tiles; 320 of 256-row tiles).  Every output is written, the guard
    bands keep the sentinel, and the result is the float64 reference bit for bit."""
    x, w, b, r = cc.operands(case, "exact")
    ref = cc.reference(x, w, case.g, b, r)
    packed = cc.pack(tspn, device, case.form, w)
    xd = cc.device_x(device, case.form, x)
    bd = cc.t(b).to(device)
    rd = None if r is None else cc.t(r).to(device).to(out_dtype(case.form))
    buf, out = held(tuple(ref.shape), device, out_dtype(case.form))
    assert out.data_ptr() % 16 == 0
    tspn._abi.check(cc.run_raw(tspn, case.form, xd, case.nb, case.g, case.cin, packed, case.cout, bd, rd, False, out))
    torch.cuda.synchronize()
    assert_written_inside_only(buf, out, cc.case_id(case))
    assert_bits_equal(out, ref, cc.case_id(case))


# ============================================================================================ 5. non-finite values
NONFINITE_GEOMS = [cc.Geom(3, 3, 1, 1, 3, 2), cc.Geom(3, 3, 1, 2, 2, 2), cc.Geom(3, 1, 2, 1, 6, 7), cc.Geom(3, 3, 2, 0, 4, 6)]
NONFINITE_CASES = [cc.Case(f, ci, co, g, cc.NB) for f, ci, co in EPI_ROWS for g in NONFINITE_GEOMS]


def unread_pixel(g):
    """(row, column) of an input pixel that no window reads, or None."""
    oh, ow = cc.out_hw(g)
    rows = {o * g.stride - g.pad + a for o in range(oh) for a in range(g.KH)}
    cols = {o * g.stride - g.pad + b for o in range(ow) for b in range(g.KW)}
    for i in range(g.H - 1, -1, -1):
        for j in range(g.W - 1, -1, -1):
            if i not in rows or j not in cols:
                return i, j
    return None


@pytest.mark.parametrize("case", **by_id(NONFINITE_CASES))
def test_an_infinity_reaches_exactly_the_windows_that_hold_it(tspn, device, case):
    """+Inf in one channel of: the last pixel of image 0, pixel (0, 0) of image 1, the last pixel of a middle row and the
    centre pixel of image 2, and (image 1) a pixel no window reads where the stride leaves one.  Non-zero real weights,
    bias, no residual, no ReLU.  The non-finite outputs (+-Inf, NaN where +Inf and -Inf meet) are the reference's, at the
    reference's positions; every other output meets the real-valued bound.  A padding tap, a masked tap of the
    linear-range form or a neighbouring image's pixel that took part as 0 x Inf would show as NaN."""
    g = case.g
    x, w, b, _ = cc.operands(case, "real")
    w = np.where(w == 0, np.float32(0.125), w)        # (a weight drawn as exactly zero would make 0 x Inf part of the reference)
    x = np.array(x)
    spots = [(0, g.H - 1, g.W - 1), (1, 0, 0), (2, g.H // 2, g.W - 1), (2, g.H // 2, g.W // 2)]
    skipped = unread_pixel(g)
    if g.stride == 2:
        assert skipped is not None
    if skipped is not None:
        spots.append((1,) + skipped)
    for k, (n, i, j) in enumerate(spots):
        x[n, i, j, (5 * k + 1) % case.cin] = np.inf
    ref = cc.reference(x, w, g, b)
    finite = torch.isfinite(ref)
    nonfinite = int((~finite).sum())
    print(f"{cc.case_id(case)}: {nonfinite} of {ref.numel()} reference outputs are not finite")
    assert finite.any() and nonfinite > 0
    got = cc.run(tspn, device, case.form, x, w, g, b).cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "NaN at other positions than the reference's"
    assert torch.equal(torch.isinf(got), torch.isinf(ref)), "Inf at other positions than the reference's"
    assert torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), "an infinity of the other sign"
    assert_close(case.form, got, ref, cc.case_id(case), where=finite)


# ============================================================================================ the refusal
EMPTY = [(1, 1, 2, 2, 2, 0), (2, 1, 3, 3, 2, 0), (1, 4, 1, 8, 7, 1)]          # (H, W, KH, KW, stride, pad)


@pytest.mark.parametrize("form,cin,cout", [r for r in EPI_ROWS if r[2] != 64], ids=[r[0] for r in EPI_ROWS if r[2] != 64])
@pytest.mark.parametrize("H,W,KH,KW,stride,pad", EMPTY)
def test_a_kernel_larger_than_the_padded_map_is_refused(tspn, device, form, cin, cout, H, W, KH, KW, stride, pad):
    """C's truncating division gives (H + 2 pad - KH) / stride + 1 = 1 for -stride < H + 2 pad - KH < 0; torch raises,
    the wrappers raise ValueError, and the C entries return TSPN_EINVAL without writing.  The buffer holds the one row
    [NB, 1, 1, Cout] that an entry without the check would write."""
    g = cc.Geom(KH, KW, stride, pad, H, W)
    assert H + 2 * pad < KH or W + 2 * pad < KW
    assert (H + 2 * pad - KH) // stride + 1 <= 0 or (W + 2 * pad - KW) // stride + 1 <= 0
    nb = 2
    rng = tspn.hashrng
    x = rng.uniform(1603, "x", (nb, H, W, cin), -1, 1)
    w = rng.normal(1603, "w", (cout, cin, KH, KW), std=0.1)
    with pytest.raises(RuntimeError):
        cc.reference(x, w, g)
    packed = cc.pack(tspn, device, form, w)
    xd = cc.device_x(device, form, x)
    with pytest.raises(ValueError, match="empty output"):
        if form == "cin4":
            tspn.ops.conv2d_nhwc_cin4(xd, packed, (KH, KW), stride, pad)
        elif form == "bf16":
            tspn.ops.conv2d_nhwc_bf16(xd, packed, (KH, KW), stride, pad)
        else:
            tspn.ops.conv2d_nhwc(xd, packed, (KH, KW), stride, pad)
    buf, out = held((nb, 1, 1, cout), device, out_dtype(form))
    rc = cc.run_raw(tspn, form, xd, nb, g, cin, packed, cout, None, None, False, out)
    refused(tspn, rc, tspn._abi.TSPN_EINVAL, f"{form} {tuple(g)}")
    assert b"empty output" in tspn._abi.lib().tspn_last_error()
    torch.cuda.synchronize()
    assert_untouched(buf, f"{form} {tuple(g)}")
