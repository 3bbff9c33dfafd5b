"""The bf16 scoring path against float64 at a RELATIVE, derived bound, on eight input kinds and at cfg3's depth, and on
inputs where the result must be the correctly rounded sum bit for bit whatever the summation order (ties at the rounding
points included).  The budget, its derivation, the kinds and the exact-case generators are tests/bf16_reference.py (host
side: tests/test_bf16_reference_host.py).  With u = 2^-24 and S the sum of magnitudes:

    pair stages, dense heads (v_mfma_f32_16x16x32_bf16, k = 32):   |got - ref64| <= 2 (32 + C / 32 + 2) u S
    conv (v_mfma_f32_32x32x16_bf16, k = 16):                       |got - ref64| <= 2 (16 + 3 Cin / 16 + 2) u S
    mean:  bf16(fl32(m - e)) <= got <= bf16(fl32(m + e)),  e = 2 (ceil(T / 4) + 3) u sum |x_t| / T

Every reference starts from the kernel's own bf16 operands (the fp32 add u + v is formed in numpy float32), so a flip at a
rounding point is charged to nobody.  Each case prints its worst |err| / budget; profiles/r26/README.md has the table."""
import numpy as np
import pytest
import torch

import bf16_reference as br
from sentinel_buffers import p
from test_gpu_bf16_heads_h import scattered_table

pytestmark = pytest.mark.gpu

H = 12
# (B, N, T): <4, 8, 2> with two videos, <8, 16, 2> with two ragged tiles per axis (T % 16 != 0); at C = 2048 the k-loop runs 64
# steps, both LDS stages in use, on the smallest grid there is
TILE_FORMS = [(2, 5, 18), (1, 17, 18)]
PAIR_CASES = ([(kind, C, *f) for kind in br.KINDS for C in (32, 96) for f in TILE_FORMS]
              + [(kind, 2048, 1, 3, 16) for kind in br.KINDS])
CONV_SHAPES = [(2, 5, 32, 8), (3, 33, 48, 132), (2, 20, 1024, 64)]        # the last: cfg3's depth, 192 k-steps of the ring
MEAN_T = (1, 2, 3, 4, 5, 7, 53, 900)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def dev16(x, device):
    """bf16 values held in fp32 -> bf16 on the device (the cast is exact)."""
    assert np.array_equal(br.rne_bf16(x), x, equal_nan=True)
    return t(x).to(torch.bfloat16).to(device)


def check_budget(got, ref, bnd, what):
    """|got - ref64| <= budget elementwise; prints the worst ratio and returns it."""
    assert got.shape == ref.shape and bool(np.isfinite(got).all()), what
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(r), r.shape)
    print(f"{what}: worst |err| / budget = {float(r[worst]):.3f}")
    assert bool((err <= bnd).all()), f"{what}: |err| = {err[worst]:.3e} > budget {bnd[worst]:.3e} at {worst}"
    return float(r[worst])


def assert_bits(got, want, what):
    off = br.bits(got) != br.bits(want)
    assert not off.any(), (f"{what}: {int(off.sum())} of {off.size} outputs differ from float32(ref64), worst "
                           f"{np.abs(got.astype(np.float64) - want).max():.3e} at |ref| up to {np.abs(want).max():.3e}")
    np.testing.assert_array_equal(br.bits(got), br.bits(want))


def grid(tspn, device, y, w, b, B, N):
    Hh = w.shape[0]
    return tspn.ops.heads_pairgrid_bf16(t(y).to(device), B, N, tspn.ops.pack_heads_bf16(t(w).to(device)), t(b).to(device),
                                        Hh).cpu().numpy()


# ------------------------------------------------------------------------------------------------ pair stage
@pytest.mark.parametrize("kind,C,B,N,T", PAIR_CASES, ids=[f"{c[0]}-C{c[1]}-N{c[3]}" for c in PAIR_CASES])
def test_heads_pairgrid_bf16_meets_the_budget(tspn, device, kind, C, B, N, T):
    y, w, b = br.make_pair_case(tspn.hashrng, kind, B, N, C, T, H)
    a = br.pair_activations(y, br.pair_table(B, N))
    check_budget(grid(tspn, device, y, w, b, B, N), br.heads_ref64(a, w, b), br.heads_budget(a, w, b),
                 f"grid {kind} C={C} {(B, N, T)}")


def test_heads_pairgrid_bf16_meets_the_budget_with_sixteen_heads(tspn, device):
    B, N, T, C = 2, 5, 18, 32
    y, w, b = br.make_pair_case(tspn.hashrng, "hot_channel", B, N, C, T, 16)
    a = br.pair_activations(y, br.pair_table(B, N))
    check_budget(grid(tspn, device, y, w, b, B, N), br.heads_ref64(a, w, b), br.heads_budget(a, w, b), "grid hot_channel H=16")


@pytest.mark.parametrize("C,B,N,T", [(32, 2, 5, 18), (32, 1, 17, 18), (2048, 1, 3, 16)], ids=["C32-N5", "C32-N17", "C2048-N3"])
@pytest.mark.parametrize("which", br.EXACT_KINDS)
def test_heads_pairgrid_bf16_is_exact_where_every_partial_sum_is(tspn, device, which, C, B, N, T):
    """plain / ties / zeros at every (qa, qw) extreme: integer partial sums below 2^24 units (asserted by the generator), so
    the output is float32(ref64) bit for bit; on `ties` ties-to-even alone decides the activations."""
    for qa, qw in br.Q_PAIRS:
        y, w, b, units = br.exact_pair_case(tspn.hashrng, which, B, N, C, T, qa, qw, H)
        a = br.pair_activations(y, br.pair_table(B, N))
        want = br.heads_ref64(a, w, b).astype(np.float32)
        assert_bits(grid(tspn, device, y, w, b, B, N), want, f"grid {which} C={C} N={N} q=({qa}, {qw}), {units} units")


@pytest.mark.parametrize("C", [32, 2048])
def test_heads_pairlist_bf16_rows_off_the_benign_distribution(tspn, device, C):
    """A scattered table (repeated rows, an (s, s) row, two videos interleaved): the exact generators give float32(ref64) on
    every row, `hot_channel` meets the budget, and every row with s != o has the bits of the grid's row."""
    B, N, T = 2, 5, 18
    table = scattered_table(B, N)
    assert bool((table[:, 0] == table[:, 1]).any()) and len(np.unique(table, axis=0)) < len(table)
    off = table[:, 0] != table[:, 1]
    bb, s, o = table[off, 0] // N, table[off, 0] % N, table[off, 1] % N
    row = bb * N * (N - 1) + s * (N - 1) + np.where(o < s, o, o - 1)

    def both(y, w, b):
        yd, packed, bd = t(y).to(device), tspn.ops.pack_heads_bf16(t(w).to(device)), t(b).to(device)
        lst = tspn.ops.heads_pairlist_bf16(yd, t(table).to(device), B, N, packed, bd, H).cpu().numpy()
        grd = tspn.ops.heads_pairgrid_bf16(yd, B, N, packed, bd, H).cpu().numpy()
        np.testing.assert_array_equal(br.bits(lst[off]), br.bits(grd[row]))
        return lst

    for which in br.EXACT_KINDS:
        for qa, qw in (br.Q_PAIRS if C == 32 else br.Q_PAIRS[:4]):
            y, w, b, _ = br.exact_pair_case(tspn.hashrng, which, B, N, C, T, qa, qw, H)
            want = br.heads_ref64(br.pair_activations(y, table), w, b).astype(np.float32)
            assert_bits(both(y, w, b), want, f"list {which} C={C} q=({qa}, {qw})")
    y, w, b = br.make_pair_case(tspn.hashrng, "hot_channel", B, N, C, T, H)
    a = br.pair_activations(y, table)
    check_budget(both(y, w, b), br.heads_ref64(a, w, b), br.heads_budget(a, w, b), f"list hot_channel C={C}")


# ------------------------------------------------------------------------------------------------ dense heads
_identity = {}


def identity_conv(tspn, device, C):
    """pack_conv3_bf16 of the centre-tap identity [C, C, 3]: the encoder hands its bf16 input to the heads unchanged."""
    if C not in _identity:
        w = torch.zeros((C, C, 3), device=device)
        w[torch.arange(C), torch.arange(C), 1] = 1.0
        _identity[C] = tspn.ops.pack_conv3_bf16(w)
    return _identity[C]


def dense_entry(tspn, device, y, w, b):
    """tspn_heads_dense_bf16 through the C ABI on fp32 y [P, T, C]."""
    P, T, C = y.shape
    yd, packed, bd = t(y).to(device), tspn.ops.pack_heads_bf16(t(w).to(device)), t(b).to(device)
    out = torch.empty((P, w.shape[0], T), dtype=torch.float32, device=device)
    rc = tspn._abi.lib().tspn_heads_dense_bf16(p(yd), C, P, C, T, p(packed), p(bd), w.shape[0], p(out), tspn.ops._stream())
    assert rc == 0, tspn._abi.lib().tspn_last_error()
    return out.cpu().numpy()


def encoder_entry(tspn, device, y, w, b):
    """temporal_encoder_heads_bf16 on x = bf16(y) with the identity conv: (heads, the y the heads read)."""
    P, T, C = y.shape
    x = dev16(br.rne_bf16(y), device)
    y_ws = torch.empty((P, T, C), dtype=torch.float32, device=device)
    out = tspn.ops.temporal_encoder_heads_bf16(x, identity_conv(tspn, device, C), None, tspn.ops.pack_heads_bf16(t(w).to(device)),
                                               t(b).to(device), w.shape[0], y_ws=y_ws)
    return out.cpu().numpy(), y_ws.cpu().numpy()


@pytest.mark.parametrize("C", [32, 2048])
@pytest.mark.parametrize("kind", br.KINDS)
def test_dense_heads_bf16_meet_the_budget_through_both_entries(tspn, device, kind, C):
    P, T = 3, 18
    y, w, b = br.make_dense_case(tspn.hashrng, kind, P, C, T, H)
    a = br.dense_activations(y)
    check_budget(dense_entry(tspn, device, y, w, b), br.heads_ref64(a, w, b), br.heads_budget(a, w, b), f"dense {kind} C={C}")
    out, y_ws = encoder_entry(tspn, device, y, w, b)
    np.testing.assert_array_equal(y_ws, br.rne_bf16(y))            # the identity conv is exact, bf16 subnormals included
    a = br.dense_activations(y_ws)                                 # teacher-forced: what the heads read
    check_budget(out, br.heads_ref64(a, w, b), br.heads_budget(a, w, b), f"encoder + heads {kind} C={C}")


@pytest.mark.parametrize("C", [32, 2048])
@pytest.mark.parametrize("which", br.EXACT_KINDS)
def test_dense_heads_bf16_are_exact_where_every_partial_sum_is(tspn, device, which, C):
    P, T = 3, 18
    for qa, qw in br.Q_PAIRS:
        y, w, b, units = br.exact_dense_case(tspn.hashrng, which, P, C, T, qa, qw, H)
        want = br.heads_ref64(br.dense_activations(y), w, b).astype(np.float32)
        assert_bits(dense_entry(tspn, device, y, w, b), want, f"dense {which} C={C} q=({qa}, {qw}), {units} units")
        out, y_ws = encoder_entry(tspn, device, y, w, b)           # a tie is rounded at the input instead: the same value
        assert_bits(out, want, f"encoder + heads {which} C={C} q=({qa}, {qw})")


# ------------------------------------------------------------------------------------------------ conv
def conv(tspn, device, x, w, b):
    packed = tspn.ops.pack_conv3_bf16(t(w).to(device))
    return tspn.ops.conv3_tc_bf16(dev16(x, device), packed, None if b is None else t(b).to(device)).cpu().numpy()


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", br.CONV_KINDS)
def test_conv3_bf16_meets_the_budget(tspn, device, kind, shape):
    x, w, b = br.make_conv_case(tspn.hashrng, kind, *shape)
    check_budget(conv(tspn, device, x, w, b), br.conv_ref64(x, w, b), br.conv_budget(x, w, b), f"conv {kind} {shape}")
    check_budget(conv(tspn, device, x, w, None), br.conv_ref64(x, w), br.conv_budget(x, w), f"conv {kind} {shape} no bias")


@pytest.mark.parametrize("which", ["plain", "zeros"])
def test_conv3_bf16_is_exact_at_cfg3_depth(tspn, device, which):
    B, T, Cin, M = 2, 20, 1024, 64
    for qa, qw in br.Q_PAIRS:
        x, w, b, units = br.exact_conv_case(tspn.hashrng, which, B, T, Cin, M, qa, qw)
        assert_bits(conv(tspn, device, x, w, b), br.conv_ref64(x, w, b).astype(np.float32),
                    f"conv {which} q=({qa}, {qw}), {units} units")
    assert_bits(conv(tspn, device, x, w, None), br.conv_ref64(x, w).astype(np.float32) + np.float32(0.0), f"conv {which} no bias")


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("T", MEAN_T)
@pytest.mark.parametrize("kind", br.MEAN_KINDS)
def test_temporal_mean_bf16_lies_in_its_interval(tspn, device, kind, T):
    for D in (8, 40):
        x = br.make_mean_case(tspn.hashrng, kind, 3, T, D)
        got = tspn.ops.temporal_mean_bf16(dev16(x, device)).cpu().numpy()
        lo, hi = br.mean_interval(x)
        np.testing.assert_array_equal(got, br.rne_bf16(got))                    # bf16 values
        bad = ~((lo <= got) & (got <= hi))
        print(f"mean {kind} T={T} D={D}: {float((lo != hi).mean()):.3f} of the intervals hold more than one value, "
              f"{float((got != br.rne_bf16(x.astype(np.float64).mean(1).astype(np.float32))).mean()):.4f} off the rounded float64 mean")
        assert not bad.any(), f"mean {kind} T={T} D={D}: {int(bad.sum())} outside, first {got[bad][0]} not in [{lo[bad][0]}, {hi[bad][0]}]"


@pytest.mark.parametrize("T", [1, 2, 3, 4, 8])
def test_temporal_mean_bf16_exact_cases(tspn, device, T):
    """Dyadic T: exact sum, exact division, ties included.  T = 3: bf16(fl32(s / 3)), the kernel's double rounding."""
    for q in br.Q_MEAN:
        for D in (8, 40):
            x, want = br.exact_mean_case(tspn.hashrng, 3, T, D, q)
            assert_bits(tspn.ops.temporal_mean_bf16(dev16(x, device)).cpu().numpy(), want, f"mean T={T} D={D} q={q}")


# ------------------------------------------------------------------------------------------------ fused passes
@pytest.mark.parametrize("kind", ["hot_channel", "large"])
def test_fused_bf16_passes_equal_their_stages_at_cfg3_depth(tspn, device, kind):
    """(B, N, T, D) = (1, 3, 16, 1024), C = 2048: out_heads of forward_fused_bf16 is bit-equal to conv3_tc_bf16 followed by
    heads_pairgrid_bf16 stand-alone on the same operands (forward_fused_bf16_pairs: heads_pairlist_bf16), and out_logits to
    temporal_mean_bf16 followed by the predicate head on the means -- the same pass on the means as one-frame features,
    whose mean is the identity.  Teacher-forced: the stages read each other's outputs."""
    ops = tspn.ops
    B, N, T, D, K = 1, 3, 16, 1024, 132
    C = 2 * D
    x, w4, cb = br.make_conv_case(tspn.hashrng, kind, N, T, D, 2 * C)
    conv_w = np.concatenate([w4[:C], w4[C:]], 1)                                # conv.weight [C, C, 3]: U rows | V rows
    hw = br.rne_bf16(tspn.hashrng.normal(179, "hw", (H, C), std=0.1))
    hb = tspn.hashrng.normal(179, "hb", (H,), std=0.1)
    scale = np.float32(2.0 ** -13 if kind == "large" else 1.0)
    cls_w = br.rne_bf16(tspn.hashrng.normal(179, "cw", (K, C), std=0.02) * scale)
    cls_b = tspn.hashrng.normal(179, "cb", (K,), std=0.1)
    d = lambda v: t(v).to(device)   # noqa: E731
    feats = dev16(x, device)
    packed, hp = ops.pack_conv3_bf16(d(conv_w), split=D), ops.pack_heads_bf16(d(hw))
    args = (packed, d(cb[:C]), hp, d(hb), d(cls_w), d(cls_b))
    canon = ops.pair_index(N, device)
    table = torch.tensor([[0, 1], [2, 0], [1, 1], [0, 1], [2, 1]], dtype=torch.int64, device=device)
    # the stages, stand-alone
    bias2 = torch.cat([d(cb[:C]), torch.zeros(C, device=device)])               # the conv bias rides on the subject half
    y = ops.conv3_tc_bf16(feats, packed, bias2)
    assert y.shape == (N, T, 2 * C)
    means = ops.temporal_mean_bf16(feats)
    one_frame = means.to(torch.bfloat16).view(N, 1, D)
    assert torch.equal(one_frame.float().view(N, D), means)
    for pairs, canonical in ((canon, True), (table, False)):
        heads, logits = ops.forward_fused_bf16(feats, pairs, B, N, *args, canonical_pairs=canonical)
        want = (ops.heads_pairgrid_bf16(y, B, N, hp, d(hb), H) if canonical
                else ops.heads_pairlist_bf16(y, pairs, B, N, hp, d(hb), H))
        assert torch.equal(heads.view(torch.int32), want.view(torch.int32)), f"{kind} canonical={canonical}: heads"
        _, want_l = ops.forward_fused_bf16(one_frame.contiguous(), pairs, B, N, *args, canonical_pairs=canonical)
        assert torch.equal(logits.view(torch.int32), want_l.view(torch.int32)), f"{kind} canonical={canonical}: logits"
        # and the logits are the predicate head's: sigmoid(cat(mean_s, mean_o) . cls_w^T + b) in float64, at the depth-2048
        # budget of an fp32 contraction summed in any order, (C + 2) u S, through a sigmoid of slope <= 1/4, plus 2^-22 for
        # expf, the add and the division on values in (0, 1)
        m = means.cpu().numpy().astype(np.float64)
        pr = pairs.cpu().numpy()
        f = np.concatenate([m[pr[:, 0]], m[pr[:, 1]]], 1)
        z = f @ cls_w.astype(np.float64).T + cls_b.astype(np.float64)
        S = np.abs(f) @ np.abs(cls_w.astype(np.float64)).T + np.abs(cls_b.astype(np.float64))
        err = np.abs(logits.cpu().numpy().astype(np.float64) - 1.0 / (1.0 + np.exp(-z)))
        bnd = 0.25 * (C + 2) * br.U * S + 2.0 ** -22
        print(f"fused {kind} canonical={canonical}: logits worst |err| / bound = {float((err / bnd).max()):.3f}")
        assert bool((err <= bnd).all())
    a = br.pair_activations(y.cpu().numpy(), br.pair_table(B, N))
    check_budget(ops.heads_pairgrid_bf16(y, B, N, hp, d(hb), H).cpu().numpy(), br.heads_ref64(a, hw, hb),
                 br.heads_budget(a, hw, hb), f"fused {kind}: heads on the pass's own y")
