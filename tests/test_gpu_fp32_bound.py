"""The fp32 scorer kernels against float64 at a RELATIVE, derived bound on eight input kinds, and on inputs where the result
must be float32(ref64) bit for bit whatever the summation order, every output held in a sentinel buffer.  The budget, its
derivation per kernel, the kinds and the exact-case generators are tests/fp32_reference.py (host side:
tests/test_fp32_reference_host.py).  With u = 2^-24 and S the sum of magnitudes:

    conv (v_mfma_f32_32x32x2_f32, k = 2):                 |got - ref64| <= (2 (2 + 3 Cin / 2 + 2) + 1) u S
    heads, pair grid (v_mfma_f32_16x16x4_f32, k = 4):     |got - ref64| <= (2 (4 + C / 4 + 2) + 1) u S
    split-K GEMM (the same MFMA, `splits` slices of kps): |got - ref64| <= (2 (4 + kps / 4 + splits + 2) + 1) u S
    block-L1 form: fp32_reference.norm_K;  mean, sum: the intervals fl32((s -+ 2 (T - 1) u sum |x|) / T), fl32(s -+ ..)

Every launch goes through the C ABI into sentinel_buffers.held outputs.  The shapes are the case tables of
tests/test_gpu_kernel_variants.py, by import.  Each budget case prints its worst |err| / budget; profiles/r32/README.md has the
table, the sigmoid measurement behind SIGMOID_CAP_U and the planted defects these tests were run against."""
import numpy as np
import pytest
import torch

import fp32_reference as fr
import oracle
from sentinel_buffers import assert_written_inside_only, held, p
from test_gpu_kernel_variants import (CONV3_BT, CONV3_VARIANTS, conv3_variant, off4, pairgrid_variant, splits_of)

pytestmark = pytest.mark.gpu

# sigmoid epilogue: the worst |out - sigmoid64(raw)| / u measured over every case of test_sigmoid_epilogue.. was 1.463 u
# (profiles/r32/README.md); the cap is twice that, because the device's expf and reciprocal are not specified to the ulp
SIGMOID_MEASURED_U = 1.463
SIGMOID_CAP_U = 2.0 * SIGMOID_MEASURED_U
SPLIT_K_ROWS = [(10944, 40, 289, 1), (5, 4500, 10, 64), (70, 63, 17, 1), (9, 129, 144, 2), (9, 127, 145, 1), (3, 2047, 289, 31),
                (130, 289, 5, 4)]          # test_predicate_head_split_k_edges' rows
BASELINE_ROW = (70, 11070, 132, 64)
# 64 slices of which the LAST holds columns: kps = 96 and 63 * 96 = 6048 < 6100.  At F = 4500 (kps = 96) the slices from 47 up and
# at F = 11070 (kps = 192) those from 58 up are empty, so neither row above sees a reduce kernel that stops one slice short
# (planted defect d of profiles/r32/README.md went unseen until this row)
LIVE_LAST_SLICE_ROW = (5, 6100, 10, 64)
NORM_ROWS = [(33, 3 + 40 * 70 + 5, 21, 3, 40, 70), (70, 11070, 132, 70, 1000, 8)]
MEAN_SHAPES = [(3, 7, 8), (2, 1, 4), (4, 33, 132), (5, 150, 64)]


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def q_of(*key):
    """One (qa, qw) of Q_PAIRS per case, walking through all nine over a parametrised test."""
    return fr.Q_PAIRS[sum(int(k) for k in key) % len(fr.Q_PAIRS)]


def call(tspn, name, *args):
    tspn._abi.check(getattr(tspn._abi.lib(), name)(*args, tspn.ops._stream()))


def check_budget(got, ref, bnd, what):
    """|got - ref64| <= budget elementwise, no element excluded; prints the worst ratio and returns it."""
    assert got.shape == ref.shape and got.size > 0 and bool(np.isfinite(got).all()), what
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(r), r.shape)
    print(f"BOUND {what}: worst |err| / budget = {float(r[worst]):.3f}")
    assert bool((err <= bnd).all()), f"{what}: |err| = {err[worst]:.3e} > budget {bnd[worst]:.3e} at {worst}"
    return float(r[worst])


def assert_bits(got, want, what):
    """Bit equality with float32(ref64), -0 folded onto +0 on both sides (fp32_reference: the sign of a zero output)."""
    got, want = fr.fold_zero(got), fr.fold_zero(np.asarray(want, np.float32))
    assert got.shape == want.shape and got.size > 0, what
    off = fr.bits(got) != fr.bits(want)
    assert not off.any(), (f"{what}: {int(off.sum())} of {off.size} outputs differ from float32(ref64), first at "
                           f"{tuple(np.argwhere(off)[0])}: {got[off][0]!r} != {want[off][0]!r}")


def report_subnormal(got, ref, flushed, bnd, what):
    """What the kernel does with fp32 subnormal operands: the error in units of the budget (floor excluded) and of the error
    of a kernel that reads every subnormal operand as zero (`flushed` = that kernel's float64 result)."""
    err = np.abs(got.astype(np.float64) - ref)
    ferr = np.abs(flushed - ref)
    print(f"SUBNORMAL {what}: worst |err| / budget = {float((err / bnd).max()):.3f}, worst |err| / flush error = "
          f"{float((err / np.maximum(ferr, 1e-300)).max()):.3e}, flush error / budget = {float((ferr / bnd).max()):.3e}")


# ------------------------------------------------------------------------------------------------ conv
def conv_launch(tspn, device, entry, x_tc, packed, bias, relu, x_offset=False):
    """tspn_conv3_f32 (x handed over as [B, Cin, T]) or tspn_conv3_tc_f32 (x [B, T, Cin]) into a held [B, M, T]."""
    B, T, Cin = x_tc.shape
    M = packed.shape[2]
    xs = x_tc if entry == "tspn_conv3_tc_f32" else np.ascontiguousarray(x_tc.transpose(0, 2, 1))
    xd = off4(t(xs), device) if x_offset else t(xs).to(device)
    bd = None if bias is None else t(bias).to(device)
    buf, y = held((B, M, T), device)
    dims = (B, T, Cin) if entry == "tspn_conv3_tc_f32" else (B, Cin, T)
    call(tspn, entry, p(xd), *dims, p(packed), M, p(bd), 1 if relu else 0, p(y))
    assert_written_inside_only(buf, y, f"{entry} {dims} M={M}")
    return y.cpu().numpy()


def pack(tspn, device, w, variant=None):
    packed = tspn.ops.pack_conv3(t(w).to(device))
    if variant == "scalar":
        packed = off4(packed, device)
    if variant is not None:
        assert conv3_variant(w.shape[1], w.shape[0], packed) == variant
    return packed


def conv_exact(tspn, device, entry, variant, B, T, Cin, M, both=None):
    """plain and zeros, with bias and ReLU on and off; `both`: also tspn_conv3_tc_f32, whose bits must be the same."""
    for which in fr.EXACT_KINDS:
        qa, qw = q_of(B, T, Cin, M, which == "zeros")
        x, w, b, units, zero_rows = fr.exact_conv_case(tspn.hashrng, which, B, T, Cin, M, qa, qw)
        packed = pack(tspn, device, w, variant)
        for bias in (b, None):
            for relu in (False, True):
                want = fr.conv_ref64(x, w, bias, relu).astype(np.float32)
                what = f"{entry} {variant} {which} {(B, T, Cin, M)} q=({qa}, {qw}) bias={bias is not None} relu={relu}, {units} units"
                got = conv_launch(tspn, device, entry, x, packed, bias, relu, x_offset=(which == "zeros" and entry == "tspn_conv3_f32"))
                assert_bits(got, want, what)
                if both:
                    np.testing.assert_array_equal(fr.bits(conv_launch(tspn, device, both, x, packed, bias, relu)), fr.bits(got))
        if which == "zeros":
            r = fr.conv_ref64(x, w, b, False)
            assert bool((r > 0).any()) and bool((r < 0).any()) and bool((r[:, zero_rows[1]] < 0).all())


def conv_budget_kinds(tspn, device, entry, variant, B, T, Cin, M, kinds=fr.PLAIN_KINDS):
    for kind in kinds:
        x, w, b = fr.make_conv_case(tspn.hashrng, kind, B, T, Cin, M)
        packed = pack(tspn, device, w, variant)
        for bias, relu in ((b, False), (None, True)):
            got = conv_launch(tspn, device, entry, x, packed, bias, relu)
            ref, bnd = fr.conv_ref64(x, w, bias, relu), fr.conv_budget(x, w, bias)
            what = f"{entry} {variant} {kind} {(B, T, Cin, M)} bias={bias is not None} relu={relu}"
            if kind == "subnormal":
                flushed = np.zeros_like(ref) if bias is None else np.broadcast_to(b.astype(np.float64)[None, :, None], ref.shape)
                report_subnormal(got, ref, np.maximum(flushed, 0) if relu else flushed, bnd, what)
            check_budget(got, ref, bnd, what)


@pytest.mark.parametrize("variant,cins", CONV3_VARIANTS)
@pytest.mark.parametrize("B,T", CONV3_BT)
@pytest.mark.parametrize("M", [4, 132])
def test_conv3_every_variant_is_exact_at_tile_edges(tspn, device, variant, cins, B, T, M):
    for Cin in cins:
        conv_exact(tspn, device, "tspn_conv3_f32", variant, B, T, Cin, M)


@pytest.mark.parametrize("variant,cins", CONV3_VARIANTS)
def test_conv3_every_variant_meets_the_budget_on_every_kind(tspn, device, variant, cins):
    B, T, M = 43, 3, 132            # B T = 129 columns: two column tiles, sequences across the tile edge
    for Cin in cins:
        conv_budget_kinds(tspn, device, "tspn_conv3_f32", variant, B, T, Cin, M)


@pytest.mark.parametrize("variant,Cin", [("dma16", 32), ("dma8", 8), ("vec", 12), ("scalar", 16)])
def test_conv3_is_exact_on_the_tile_map_with_a_short_last_group(tspn, device, variant, Cin):
    """M = 9 * 128, (B, T) = (5, 43): 18 workgroups, two groups of weight panels, two column tiles; into a sentinel buffer, so a
    tile that was never computed is seen as such."""
    conv_exact(tspn, device, "tspn_conv3_f32", variant, 5, 43, Cin, 9 * 128, both="tspn_conv3_tc_f32" if Cin % 16 == 0 and variant != "scalar" else None)


def test_conv3_at_full_depth(tspn, device):
    """Cin = 2048, 128 chunks through both LDS stages: exact, and the two kinds a depth-6144 budget can still tell apart."""
    conv_exact(tspn, device, "tspn_conv3_f32", "dma16", 1, 7, 2048, 132, both="tspn_conv3_tc_f32")
    conv_budget_kinds(tspn, device, "tspn_conv3_f32", "dma16", 1, 7, 2048, 132, kinds=("hot_channel", "cancelling"))
    conv_budget_kinds(tspn, device, "tspn_conv3_tc_f32", None, 1, 7, 2048, 132, kinds=("hot_channel", "cancelling"))


@pytest.mark.parametrize("B,T", CONV3_BT + [(5, 43)])
@pytest.mark.parametrize("Cin", [16, 48])
def test_conv3_channels_last_is_exact_and_has_the_bits_of_the_channels_first_kernel(tspn, device, Cin, B, T):
    M = 9 * 128 if (B, T) == (5, 43) else 132
    conv_exact(tspn, device, "tspn_conv3_tc_f32", None, B, T, Cin, M, both="tspn_conv3_f32")


@pytest.mark.parametrize("Cin", [16, 48])
def test_conv3_channels_last_meets_the_budget_on_every_kind(tspn, device, Cin):
    conv_budget_kinds(tspn, device, "tspn_conv3_tc_f32", None, 43, 3, Cin, 132)


# ------------------------------------------------------------------------------------------------ heads
def heads_launch(tspn, device, mode, a, b, ia, ib, bias, w, bh, P, T, forms=("aligned",)):
    """tspn_heads_f32 into a held [P, H, T] for every form: "aligned", and a, b or out at a 4-byte offset (the scalar kernel at
    an even T).  Returns the outputs, which must all have the same bits."""
    H, C = w.shape
    dev = lambda v: None if v is None else t(v).to(device)   # noqa: E731
    wd, bhd, biasd, iad, ibd = dev(w), dev(bh), dev(bias), dev(ia), dev(ib)
    outs = []
    for form in forms:
        ad = off4(t(a), device) if form == "a4" else dev(a)
        bd = None if b is None else (off4(t(b), device) if form == "b4" else dev(b))
        buf, out = held((P, H, T), device, offset=1 if form == "out4" else 0)
        call(tspn, "tspn_heads_f32", mode, p(ad), p(bd), C, p(iad), p(ibd), 1, p(biasd), p(wd), p(bhd), H, P, C, T, p(out))
        assert_written_inside_only(buf, out, f"tspn_heads_f32 mode {mode} {form} {(P, H, C, T)}")
        outs.append(out.cpu().numpy())
    for o in outs[1:]:
        np.testing.assert_array_equal(fr.bits(o), fr.bits(outs[0]))
    return outs[0]


def index_tables(tspn, P, R):
    ia = tspn.hashrng.integers(410, "ia", (P,), 0, R)
    ib = tspn.hashrng.integers(410, "ib", (P,), 0, R)
    ib[0] = ia[0]                   # an ia == ib row; R = max(P // 2, 1) rows for P pairs: repeats
    return ia, ib


FORMS = ("aligned", "a4", "b4", "out4")


@pytest.mark.parametrize("H", [1, 12, 16])
@pytest.mark.parametrize("T", [2, 31, 32, 33, 34])
@pytest.mark.parametrize("P", [1, 3, 5, 9])
def test_heads_kernel_is_exact_in_both_modes_vec2_and_scalar(tspn, device, P, T, H):
    C, R = 21, max(P // 2, 1)
    ia, ib = index_tables(tspn, P, R)
    for which in fr.EXACT_KINDS:
        qa, qw = q_of(P, T, H, which == "zeros")
        a, b, bias, w, bh, units, _ = fr.exact_heads_case(tspn.hashrng, which, R, C, T, H, qa, qw)
        what = f"P={P} T={T} H={H} {which} q=({qa}, {qw}), {units} units"
        got = heads_launch(tspn, device, 0, a, None, ia, None, None, w, bh, P, T, ("aligned", "a4", "out4"))
        assert_bits(got, fr.heads_ref64(fr.heads_act(0, a, ia), w, bh).astype(np.float32), "mode 0 " + what)
        for bs in (bias, None):
            h = fr.heads_act(1, a, ia, b, ib, bs)
            assert bool((h == 0).any()) and bool((h > 0).any())
            got = heads_launch(tspn, device, 1, a, b, ia, ib, bs, w, bh, P, T, FORMS if bs is not None else ("aligned",))
            assert_bits(got, fr.heads_ref64(h, w, bh).astype(np.float32), f"mode 1 bias={bs is not None} " + what)
        got = heads_launch(tspn, device, 1, a, b, ia, ib, bias, w, None, P, T)
        assert_bits(got, fr.heads_ref64(fr.heads_act(1, a, ia, b, ib, bias), w).astype(np.float32), "mode 1 no head bias " + what)


@pytest.mark.parametrize("which", fr.EXACT_KINDS)
def test_heads_kernel_is_exact_at_full_depth(tspn, device, which):
    P, T, H, C, R = 5, 33, 12, 2048, 2
    ia, ib = index_tables(tspn, P, R)
    for qa, qw in fr.Q_PAIRS[:4]:
        a, b, bias, w, bh, units, _ = fr.exact_heads_case(tspn.hashrng, which, R, C, T, H, qa, qw)
        got = heads_launch(tspn, device, 0, a, None, ia, None, None, w, bh, P, T)
        assert_bits(got, fr.heads_ref64(fr.heads_act(0, a, ia), w, bh).astype(np.float32), f"mode 0 C=2048 {which} q=({qa}, {qw})")
        got = heads_launch(tspn, device, 1, a, b, ia, ib, bias, w, bh, P, T)
        assert_bits(got, fr.heads_ref64(fr.heads_act(1, a, ia, b, ib, bias), w, bh).astype(np.float32),
                    f"mode 1 C=2048 {which} q=({qa}, {qw}), {units} units")


@pytest.mark.parametrize("C,P,T,H", [(21, 9, 34, 12), (21, 5, 33, 16), (2048, 5, 33, 12)], ids=["vec2", "scalar", "C2048"])
@pytest.mark.parametrize("kind", fr.KINDS)
def test_heads_kernel_meets_the_budget_on_every_kind(tspn, device, kind, C, P, T, H):
    R = max(P // 2, 1)
    ia, ib = index_tables(tspn, P, R)
    a, b, bias, w, bh = fr.make_heads_case(tspn.hashrng, kind, R, C, T, H)
    for mode in ((1,) if kind == "relu_edge" else (0, 1)):
        h = fr.heads_act(mode, a, ia, b, ib, bias)
        got = (heads_launch(tspn, device, 1, a, b, ia, ib, bias, w, bh, P, T) if mode
               else heads_launch(tspn, device, 0, a, None, ia, None, None, w, bh, P, T))
        ref, bnd = fr.heads_ref64(h, w, bh), fr.heads_budget(h, w, bh)
        what = f"tspn_heads_f32 mode {mode} {kind} C={C} T={T}"
        if kind == "relu_edge":
            assert 0.3 < float((h == 0).mean()) < 0.7
        if kind == "subnormal":
            assert float(np.abs(h).max()) < fr.SMALLEST_NORMAL and bool((h != 0).any())
            report_subnormal(got, ref, np.broadcast_to(bh.astype(np.float64)[None, :, None], ref.shape), bnd, what)
        check_budget(got, ref, bnd, what)


# ------------------------------------------------------------------------------------------------ pair grid
def pairgrid_launch(tspn, device, y, B, N, w, bh, T, offset):
    C, H = y.shape[1] // 2, w.shape[0]
    yd = off4(t(y), device) if offset else t(y).to(device)
    P = B * N * (N - 1)
    wd, bhd = t(w).to(device), t(bh).to(device)       # held by name until the launch is issued
    buf, out = held((P, H, T), device)
    call(tspn, "tspn_heads_pairgrid_f32", p(yd), B, N, C, T, p(wd), p(bhd), H, p(out))
    assert_written_inside_only(buf, out, f"tspn_heads_pairgrid_f32 {(B, N, C, T)} offset={offset}")
    return out.cpu().numpy(), pairgrid_variant(C, T, yd, out)


@pytest.mark.parametrize("C", [16, 24, 48])
@pytest.mark.parametrize("T", [2, 32, 33, 34, 150])
@pytest.mark.parametrize("N", [2, 8, 9, 17])
def test_heads_pairgrid_is_exact_in_every_variant_and_has_the_bits_of_heads_mode_1(tspn, device, N, T, C):
    B, H = 2, 12
    tab = fr.pair_table(B, N)
    seen = set()
    for which in fr.EXACT_KINDS:
        qa, qw = q_of(N, T, C, which == "zeros")
        a, b, _, w, bh, units, _ = fr.exact_heads_case(tspn.hashrng, which, B * N, C, T, H, qa, qw)
        y = np.concatenate([a, b], 1)
        h = fr.pairgrid_act(y, B, N)
        assert bool((h == 0).any()) and bool((h > 0).any())
        want = fr.heads_ref64(h, w, bh).astype(np.float32)
        for offset in (False, True):
            got, variant = pairgrid_launch(tspn, device, y, B, N, w, bh, T, offset)
            seen.add(variant)
            assert_bits(got, want, f"pair grid {variant} N={N} T={T} C={C} {which} q=({qa}, {qw}), {units} units")
        # the same rows through tspn_heads_f32 mode 1 on the canonical table: a = y's U half, b = its V half, lda = 2C
        yd, iad, ibd, wd, bhd = (t(v).to(device) for v in (y, tab[:, 0].copy(), tab[:, 1].copy(), w, bh))
        buf, out = held((len(tab), H, T), device)
        call(tspn, "tspn_heads_f32", 1, p(yd), p(yd.view(-1)[C * T:]), 2 * C, p(iad), p(ibd), 1, p(None), p(wd), p(bhd), H, len(tab),
             C, T, p(out))
        assert_written_inside_only(buf, out, "tspn_heads_f32 on the canonical table")
        np.testing.assert_array_equal(fr.bits(fr.fold_zero(out.cpu().numpy())), fr.bits(fr.fold_zero(got)))
    assert "scalar" in seen and (("v3" in seen) == (T % 4 == 0 and C % 16 == 0)) and (("vec2" in seen) == (T % 2 == 0 and "v3" not in seen))


@pytest.mark.parametrize("C,T,offset,variant", [(48, 32, False, "v3"), (24, 34, False, "vec2"), (48, 33, False, "scalar"),
                                                (48, 32, True, "scalar")], ids=["v3", "vec2", "scalar", "scalar-offset"])
@pytest.mark.parametrize("kind", fr.KINDS)
def test_heads_pairgrid_meets_the_budget_on_every_kind(tspn, device, kind, C, T, offset, variant):
    B, N, H = 2, 9, 12
    a, b, _, w, bh = fr.make_heads_case(tspn.hashrng, kind, B * N, C, T, H)
    y = np.concatenate([a, b], 1)
    h = fr.pairgrid_act(y, B, N)
    got, ran = pairgrid_launch(tspn, device, y, B, N, w, bh, T, offset)
    assert ran == variant
    ref, bnd = fr.heads_ref64(h, w, bh), fr.heads_budget(h, w, bh)
    if kind == "relu_edge":
        assert 0.3 < float((h == 0).mean()) < 0.7
    if kind == "subnormal":
        report_subnormal(got, ref, np.broadcast_to(bh.astype(np.float64)[None, :, None], ref.shape), bnd, f"pair grid {variant}")
    check_budget(got, ref, bnd, f"tspn_heads_pairgrid_f32 {variant} {kind} C={C} T={T}")


# ------------------------------------------------------------------------------------------------ split-K GEMM
def linear_launch(tspn, device, x, w, b, sigmoid=0, norm=None):
    """tspn_predicate_head_f32 / tspn_predicate_head_norm_f32 into a held [P, K]; the workspace is exactly the bytes asked for."""
    P, F = x.shape
    K = w.shape[0]
    l = tspn._abi.lib()
    xd, wd, bd = t(x).to(device), t(w).to(device), None if b is None else t(b).to(device)
    buf, out = held((P, K), device)
    if norm is None:
        need = l.tspn_predicate_head_workspace_bytes(P, F, K)
        assert need == splits_of(P, F, K) * P * K * 4
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        call(tspn, "tspn_predicate_head_f32", p(xd), P, F, F, p(wd), p(bd), K, p(out), sigmoid, p(ws), need)
    else:
        need = l.tspn_predicate_head_norm_workspace_bytes(P, F, K, *norm)
        assert need == len(fr.split_table(P, F, K, *norm)) * P * (K + 1) * 4
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        call(tspn, "tspn_predicate_head_norm_f32", p(xd), P, F, F, p(wd), p(bd), K, *norm, p(out), sigmoid, p(ws), need)
    assert_written_inside_only(buf, out, f"predicate head {(P, F, K)} norm={norm}")
    return out.cpu().numpy()


@pytest.mark.parametrize("P,F,K,splits", SPLIT_K_ROWS + [BASELINE_ROW, LIVE_LAST_SLICE_ROW], ids=lambda v: str(v))
def test_predicate_head_raw_is_exact_on_every_split_k_row(tspn, device, P, F, K, splits):
    assert splits_of(P, F, K) == splits == fr.splits_of(P, F, K)
    if (P, F, K, splits) == LIVE_LAST_SLICE_ROW:
        assert (splits - 1) * fr.kps_of(F, splits) + 32 < F
    for which in fr.EXACT_KINDS:
        for qa, qw in (q_of(P, F, K), q_of(P, F, K, 4)):
            x, w, b, units, _ = fr.exact_linear_case(tspn.hashrng, which, P, F, K, qa, qw)
            for bias in (b, None):
                assert_bits(linear_launch(tspn, device, x, w, bias), fr.linear_ref64(x, w, bias).astype(np.float32),
                            f"split-K {(P, F, K)} splits={splits} {which} q=({qa}, {qw}) bias={bias is not None}, {units} units")


@pytest.mark.parametrize("P,F,K,splits", [(70, 63, 17, 1), (5, 4500, 10, 64), LIVE_LAST_SLICE_ROW], ids=["one-split", "64-splits", "64-live-slices"])
@pytest.mark.parametrize("kind", fr.PLAIN_KINDS)
def test_predicate_head_raw_meets_the_budget_on_every_kind(tspn, device, kind, P, F, K, splits):
    assert splits_of(P, F, K) == splits
    x, w, b = fr.make_linear_case(tspn.hashrng, kind, P, F, K)
    got = linear_launch(tspn, device, x, w, b)
    ref, bnd = fr.linear_ref64(x, w, b), fr.linear_budget(x, w, b)
    if kind == "subnormal":
        report_subnormal(got, ref, np.broadcast_to(b.astype(np.float64)[None, :], ref.shape), bnd, f"split-K splits={splits}")
    check_budget(got, ref, bnd, f"tspn_predicate_head_f32 {kind} {(P, F, K)} splits={splits}")


def test_training_backward_products_are_exact_on_the_split_k_gemm(tspn, device):
    """y = x W^T, dx = nt(g, W^T), dW = nt(g^T, x^T) as model._LinearFn forms them, at (P, F, K) = (130, 150, 160): three row
    tiles, two column tiles and two splits in each of the three products; integer operands, every product exact."""
    P, F, K = 130, 150, 160
    x, w, _, _, _ = fr.exact_linear_case(tspn.hashrng, "zeros", P, F, K, -1, 7)
    g = fr._to_f32(tspn.hashrng.integers(330, "g", (P, K), -15, 16), 3)
    tr = lambda v: np.ascontiguousarray(v.T)   # noqa: E731
    for name, a, bt in (("y", x, w), ("dx", g, tr(w)), ("dW", tr(g), tr(x))):
        rows, depth = a.shape
        cols = bt.shape[0]
        assert rows > 64 and cols > 144 and splits_of(rows, depth, cols) > 1
        want64 = fr.linear_ref64(a, bt)
        assert float(np.abs(fr.linear_S(a, bt)).max()) < 2.0 ** 24 * 2.0 ** (-1 + 7 if name == "y" else 3 + 7 if name == "dx" else 3 - 1)
        assert_bits(linear_launch(tspn, device, a, bt, None), want64.astype(np.float32), f"backward product {name}")
    g, wt, _ = fr.make_linear_case(tspn.hashrng, "hot_channel", P, K, F)        # g [P, K] against W^T [F, K]: depth K
    check_budget(linear_launch(tspn, device, g, wt, None), fr.linear_ref64(g, wt), fr.linear_budget(g, wt), "nt(g, W^T) hot_channel")


@pytest.mark.parametrize("row", NORM_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_predicate_head_norm_is_exact_and_meets_the_budget(tspn, device, row):
    P, F, K, first, block, nblocks = row
    norm = (first, block, nblocks)
    for which in fr.EXACT_KINDS:
        for qa, qw in ((0, 0), (-1, 7), (-100, 100), (100, -100), (50, 0)):
            x, w, b, units, _ = fr.exact_norm_case(tspn.hashrng, which, P, F, K, *norm, qa, qw)
            assert_bits(linear_launch(tspn, device, x, w, b, norm=norm), fr.norm_ref64(x, w, b, *norm).astype(np.float32),
                        f"block-L1 {row} {which} q=({qa}, {qw}), {units} units")
    # (`subnormal` is left out on purpose: a block norm summed from subnormal |x| has no RELATIVE rounding bound, which is what
    # the budget of sum / L1 stands on; `cancelling` differs from `unit` only by a scale once a block is normalised)
    for kind in ("unit", "large", "tiny", "hot_channel", "wide"):
        x, w, b = fr.make_linear_case(tspn.hashrng, kind, P, F, K)
        if kind == "tiny":
            b = b * np.float32(2.0 ** 10)      # the normalised operand is O(1 / block) whatever x's scale: keep the bias beside it
        x[4, first + block:first + 2 * block] = 0
        check_budget(linear_launch(tspn, device, x, w, b, norm=norm), fr.norm_ref64(x, w, b, *norm), fr.norm_budget(x, w, b, *norm),
                     f"tspn_predicate_head_norm_f32 {kind} {row}")


def sigmoid_cases(tspn):
    """(x, w, b, norm): the `unit` kind and a `zeros` exact case of every split-K row, and the block-L1 tables."""
    for P, F, K, _ in SPLIT_K_ROWS + [BASELINE_ROW]:
        yield fr.make_linear_case(tspn.hashrng, "unit", P, F, K) + (None,)
        x, w, b, _, _ = fr.exact_linear_case(tspn.hashrng, "zeros", P, F, K, 0, -int(np.ceil(np.log2(70.0 * np.sqrt(F)))))
        yield x, w, b, None                 # integer logits scaled to O(1)
    for P, F, K, first, block, nblocks in NORM_ROWS:
        x, w, b = fr.make_linear_case(tspn.hashrng, "unit", P, F, K)
        yield x, w * np.float32(block / 4), b, (first, block, nblocks)


def test_sigmoid_epilogue_against_the_float64_sigmoid_of_the_kernels_own_logits(tspn, device):
    """apply_sigmoid = 1 against 1 / (1 + exp(-raw)) in float64 of the kernel's OWN raw logits (a second launch; two raw launches
    are bit-equal): summation error is charged to nobody.  The cap is twice the worst distance measured (SIGMOID_CAP_U)."""
    worst, n = 0.0, 0
    for x, w, b, norm in sigmoid_cases(tspn):
        raw = linear_launch(tspn, device, x, w, b, 0, norm)
        np.testing.assert_array_equal(fr.bits(raw), fr.bits(linear_launch(tspn, device, x, w, b, 0, norm)))
        got = linear_launch(tspn, device, x, w, b, 1, norm)
        with np.errstate(over="ignore"):
            want = 1.0 / (1.0 + np.exp(-raw.astype(np.float64)))
        assert bool(((want > 0.01) & (want < 0.99)).any()), "every logit is saturated"
        d = float(np.abs(got.astype(np.float64) - want).max() / fr.U)
        print(f"SIGMOID {x.shape} x {w.shape} norm={norm}: worst |out - sigmoid64(raw)| = {d:.3f} u")
        worst, n = max(worst, d), n + 1
    print(f"SIGMOID worst over {n} cases: {worst:.3f} u (cap {SIGMOID_CAP_U} u)")
    assert n == 18 and worst <= SIGMOID_CAP_U


# ------------------------------------------------------------------------------------------------ mean, sum
def mean_launch(tspn, device, x, form):
    """tspn_temporal_mean_f32 / tspn_temporal_sum_f32 on x [R, T, D] into a held [R, D]: "td4" aligned, "td" at a 4-byte offset
    (the scalar kernel), "ct" / "ct4" the transposed layout aligned / at an offset, "sum"."""
    R, T, D = x.shape
    src = np.ascontiguousarray(x.transpose(0, 2, 1)) if form in ("ct", "ct4") else x
    xd = off4(t(src), device) if form in ("td", "ct4") else t(src).to(device)
    buf, out = held((R, D), device)
    if form == "sum":
        call(tspn, "tspn_temporal_sum_f32", p(xd), R, T, D, p(out))
    else:
        call(tspn, "tspn_temporal_mean_f32", p(xd), R, T, D, 0 if form in ("ct", "ct4") else 1, p(out))
    assert_written_inside_only(buf, out, f"temporal {form} {(R, T, D)}")
    return out.cpu().numpy()


MEAN_FORMS = ("td4", "td", "ct", "ct4", "sum")


@pytest.mark.parametrize("R,T,D", MEAN_SHAPES + [(3, 3, 8)])
def test_temporal_mean_and_sum_are_exact_for_every_t(tspn, device, R, T, D):
    """The integer frame sum is exact in any order and the one division by float(T) is correctly rounded:
    float32(float32(s) / float32(T)) bit for bit, T = 1, 3, 7, 33, 150."""
    for q in fr.Q_MEAN:
        x, want_mean, want_sum = fr.exact_mean_case(tspn.hashrng, R, T, D, q)
        for form in MEAN_FORMS:
            assert_bits(mean_launch(tspn, device, x, form), want_sum if form == "sum" else want_mean, f"{form} {(R, T, D)} q={q}")


@pytest.mark.parametrize("R,T,D", MEAN_SHAPES)
@pytest.mark.parametrize("kind", fr.MEAN_KINDS)
def test_temporal_mean_and_sum_lie_in_their_intervals(tspn, device, kind, R, T, D):
    x = fr.make_mean_case(tspn.hashrng, kind, R, T, D)
    for form in MEAN_FORMS:
        got = mean_launch(tspn, device, x, form)
        lo, hi = fr.sum_interval(x) if form == "sum" else fr.mean_interval(x)
        bad = ~((lo <= got) & (got <= hi))
        print(f"INTERVAL {form} {kind} {(R, T, D)}: {float((lo != hi).mean()):.3f} of the intervals hold more than one value")
        assert not bad.any(), f"{form} {kind} {(R, T, D)}: {int(bad.sum())} outside, first {got[bad][0]!r} not in [{lo[bad][0]!r}, {hi[bad][0]!r}]"
    np.testing.assert_array_equal(fr.bits(mean_launch(tspn, device, x, "td4")), fr.bits(mean_launch(tspn, device, x, "td")))


# ------------------------------------------------------------------------------------------------ compositions
def composition_case(rng, B, N, T, D, A, K, seed=340):
    """Integer operands of the whole pass, sized so that conv outputs x head weights stay below 2^24 units (asserted):
    feats [B N, T, D] |m| <= 3 with the last frame chosen so that every frame sum is a multiple of T (the mean is an integer),
    conv.weight [C, C, 3], conv.bias [C], head_w [3A, C], head_b, cls_w [K, C] all |m| <= 3, cls_b |m| <= 100; C = 2 D."""
    C, NT = 2 * D, B * N
    f = rng.integers(seed, "f", (NT, T, D), -3, 4)
    f[:, -1] = 0
    f[:, -1] = -(f.sum(1) % T) + T * rng.integers(seed, "fl", (NT, D), 0, 2)
    assert bool((f.sum(1) % T == 0).all()) and int(np.abs(f).max()) <= T + 3
    cw = rng.integers(seed, "cw", (C, C, 3), -3, 4)
    cb = rng.integers(seed, "cb", (C,), -3, 4)
    hw = rng.integers(seed, "hw", (3 * A, C), -3, 4)
    hb = rng.integers(seed, "hb", (3 * A,), -100, 101)
    kw = rng.integers(seed, "kw", (K, C), -3, 4)
    kb = rng.integers(seed, "kb", (K,), -100, 101)
    ymax = 2 * int(np.abs(f).max()) * 3 * D * 3 + 3                   # |u_s + v_o + bias|
    assert ymax * 3 * C + 100 < (1 << 24) and int(np.abs(f.sum(1) // T).max()) * 3 * C + 100 < (1 << 24)
    f32 = lambda v: np.ascontiguousarray(v, np.float32)   # noqa: E731
    return tuple(f32(v) for v in (f, cw, cb, hw, hb, kw, kb))


@pytest.mark.parametrize("B,N,T,D", [(2, 3, 7, 16), (1, 3, 32, 16)])
def test_fused_pass_is_exact_and_equals_its_stages(tspn, device, B, N, T, D):
    """tspn_forward_fused_f32 with the direct conv, canonical and scattered pairs: heads bit-equal to float32(ref64) and to the
    stand-alone conv -> pair stage chain, logits bit-equal to the stand-alone temporal_mean -> predicate_head chain."""
    A, K, C = 4, 37, 2 * D
    f, cw, cb, hw, hb, kw, kb = composition_case(tspn.hashrng, B, N, T, D, A, K)
    dev = lambda v: t(v).to(device)   # noqa: E731
    packed = tspn.ops.pack_conv3(dev(cw), split=D)
    canon = fr.pair_table(B, N)
    scattered = np.concatenate([canon[::-1][:5], canon[:2], canon[:1]])
    # float64: y = [U + bias | V], h = relu(U_s + V_o), heads; logits = sigmoid(cat(mean_s, mean_o) . cls_w^T + b)
    w2 = np.concatenate([cw[:, :D], cw[:, D:]], 0)                      # [2C, D, 3]: U rows, then V rows
    bias2 = np.concatenate([cb, np.zeros(C, np.float32)])
    y64 = fr.conv_ref64(f, w2, bias2)
    means = f.astype(np.float64).mean(1)
    assert np.array_equal(means, np.round(means))
    # the stages, stand-alone, into held outputs
    y = conv_launch(tspn, device, "tspn_conv3_tc_f32", f, packed, bias2, False)
    assert_bits(y, y64.astype(np.float32), "conv of the composition")
    mean_gpu = mean_launch(tspn, device, f, "td4")
    assert_bits(mean_gpu, means.astype(np.float32), "mean of the composition")
    for pairs, canonical in ((canon, True), (scattered, False)):
        P = len(pairs)
        bh, oh = held((P, 3 * A, T), device)
        bl, ol = held((P, K), device)
        need = tspn.ops.fused_workspace_bytes(B, N, T, D, A, K, P)
        ws = torch.full((need,), 0x7F, dtype=torch.uint8, device=device)
        tspn.ops.forward_fused(dev(f), dev(pairs), B, N, packed, dev(cb), dev(hw), dev(hb), dev(kw), dev(kb), workspace=ws,
                               out_heads=oh, out_logits=ol, canonical_pairs=canonical)
        assert_written_inside_only(bh, oh, "fused heads")
        assert_written_inside_only(bl, ol, "fused logits")
        h64 = np.maximum(y64[pairs[:, 0], :C] + y64[pairs[:, 1], C:], 0.0)
        assert bool((h64 == 0).any()) and bool((h64 > 0).any())
        heads = oh.cpu().numpy()
        assert_bits(heads, fr.heads_ref64(h64, hw, hb).astype(np.float32), f"fused heads canonical={canonical}")
        if canonical:
            chain, _ = pairgrid_launch(tspn, device, y, B, N, hw, hb, T, False)
        else:
            yd, iad, ibd, hwd, hbd = (dev(v) for v in (y, pairs[:, 0].copy(), pairs[:, 1].copy(), hw, hb))
            bc, oc = held((P, 3 * A, T), device)
            call(tspn, "tspn_heads_f32", 1, p(yd), p(yd.view(-1)[C * T:]), 2 * C, p(iad), p(ibd), 1, p(None), p(hwd), p(hbd), 3 * A, P, C,
                 T, p(oc))
            assert_written_inside_only(bc, oc, "stand-alone pair stage")
            chain = oc.cpu().numpy()
        np.testing.assert_array_equal(fr.bits(fr.fold_zero(heads)), fr.bits(fr.fold_zero(chain)))
        pooled = np.concatenate([mean_gpu[pairs[:, 0]], mean_gpu[pairs[:, 1]]], 1)
        raw = linear_launch(tspn, device, pooled, kw, kb, 0)
        assert_bits(raw, fr.linear_ref64(pooled, kw, kb).astype(np.float32), "logits before the sigmoid")
        np.testing.assert_array_equal(fr.bits(ol.cpu().numpy()), fr.bits(linear_launch(tspn, device, pooled, kw, kb, 1)))


@pytest.mark.parametrize("B,N,T,D", [(2, 3, 7, 16), (1, 3, 32, 16)])
def test_temporal_encoder_heads_is_exact_and_equals_its_stages(tspn, device, B, N, T, D):
    """tspn_temporal_encoder_heads_f32 on a materialised x [P, C, T]: relu(conv) into the caller's h_ws, heads mode 0 on it."""
    A, C, P = 4, 2 * D, B * N
    f, cw, cb, hw, hb, _, _ = composition_case(tspn.hashrng, B, N, T, C, A, 5, seed=341)
    x_tc, cw, cb, hw = f, cw[:C, :C], cb[:C], hw[:, :C]           # x [P, T, C]; the conv is [C, C, 3]
    dev = lambda v: t(v).to(device)   # noqa: E731
    packed = tspn.ops.pack_conv3(dev(cw))
    h64 = fr.conv_ref64(x_tc, cw, cb, True)
    assert float(np.abs(h64).max()) * 3 * C + 100 < 2.0 ** 24 and bool((h64 == 0).any()) and bool((h64 > 0).any())
    bw, h_ws = held((P, C, T), device)
    bo, out = held((P, 3 * A, T), device)
    xd, cbd, hwd, hbd = (dev(v) for v in (np.ascontiguousarray(x_tc.transpose(0, 2, 1)), cb, hw, hb))
    call(tspn, "tspn_temporal_encoder_heads_f32", p(xd), P, C, T, p(packed), p(cbd), p(hwd), p(hbd), 3 * A, p(h_ws), p(out))
    assert_written_inside_only(bw, h_ws, "encoder activation")
    assert_written_inside_only(bo, out, "encoder heads")
    assert_bits(h_ws.cpu().numpy(), h64.astype(np.float32), "encoder activation")
    assert_bits(out.cpu().numpy(), fr.heads_ref64(h64, hw, hb).astype(np.float32), "encoder heads")
    h = conv_launch(tspn, device, "tspn_conv3_f32", x_tc, packed, cb, True)
    chain = heads_launch(tspn, device, 0, h, None, None, None, None, hw, hb, P, T)
    np.testing.assert_array_equal(fr.bits(out.cpu().numpy()), fr.bits(chain))


# ------------------------------------------------------------------------------------------------ data movers
def test_data_movers_into_held_outputs(tspn, device):
    """tspn_transpose_td_f32, tspn_pair_rows_f32 and the feature half of tspn_pair_gather_f32 (both forms), bit-exact, no longer
    relying on what a fresh allocation holds."""
    R, T, D = 4, 33, 132
    x = tspn.hashrng.uniform(350, "x", (R, T, D), -1, 1)
    xd = t(x).to(device)
    buf, out = held((R, D, T), device)
    call(tspn, "tspn_transpose_td_f32", p(xd), R, T, D, p(out))
    assert_written_inside_only(buf, out, "tspn_transpose_td_f32")
    np.testing.assert_array_equal(out.cpu().numpy(), x.transpose(0, 2, 1))
    src = tspn.hashrng.uniform(350, "src", (7, 37), -1, 1)
    pairs = oracle.pair_index(7).numpy()
    srcd, pd = t(src).to(device), t(pairs).to(device)
    buf, out = held((len(pairs), 2 * 37), device)
    call(tspn, "tspn_pair_rows_f32", p(srcd), 7, 37, p(pd), len(pairs), p(out))
    assert_written_inside_only(buf, out, "tspn_pair_rows_f32")
    np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate([src[pairs[:, 0]], src[pairs[:, 1]]], 1))
    N, D = 5, 64
    pairs = oracle.pair_index(N).numpy()
    for T in (160, 161):                # the rows form and the 32 x 32 form (test_pair_gather_rows_form_and_32x32_form)
        f = tspn.hashrng.uniform(350, f"f{T}", (N, T, D), -1, 1)
        fd, pd = t(f).to(device), t(pairs).to(device)
        buf, out = held((len(pairs), 2 * D, T), device)
        call(tspn, "tspn_pair_gather_f32", p(fd), p(None), N, T, D, p(pd), len(pairs), p(out), p(None))
        assert_written_inside_only(buf, out, f"tspn_pair_gather_f32 T={T}")
        np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate([f[pairs[:, 0]], f[pairs[:, 1]]], 2).transpose(0, 2, 1))


@pytest.mark.parametrize("F", [2, 3], ids=["float2", "scalar"])
def test_gather_rows_past_one_slab(tspn, device, F):
    """tspn_gather_rows_f32 loops over slabs of 65 535 rows (idx + r0, out + r0 * F): R = 65 537 reaches the second, with a padded
    source (ld = F + 2) and idx_base = 5, which ops.gather_rows never passes."""
    R, rows, ld, base = 65537, 37, F + 2, 5
    src = tspn.hashrng.uniform(360, "src", (rows, ld), -1, 1)
    idx = tspn.hashrng.integers(360, "idx", (R,), 0, rows - base)
    idx[65535], idx[65536] = 1, rows - base - 1
    srcd, idxd = t(src).to(device), t(idx).to(device)
    buf, out = held((R, F), device)
    call(tspn, "tspn_gather_rows_f32", p(srcd), ld, F, p(idxd), base, R, p(out))
    assert_written_inside_only(buf, out, f"tspn_gather_rows_f32 F={F}")
    np.testing.assert_array_equal(out.cpu().numpy(), src[base + idx, :F])
