"""tests/bf16_reference.py without a device: rne_bf16 against torch's cast; three fp32 summation orders stay inside the budget
the GPU tests hold the bf16 kernels to, on every kind, and are bit-equal to the float64 reference on every exact generator
(which proves the generators' exactness condition); two planted defects leave the budget; the fp32 emulation of the mean
kernel's order lies inside the mean's interval at every T the GPU test uses."""
import numpy as np
import pytest
import torch

import bf16_reference as br

ORDERS = ("sequential", "pairwise", "blocks")
B, N, T, H = 1, 3, 4, 12
DEPTHS = (32, 96, 2048)
CONV_SHAPES = ((2, 5, 32, 8), (1, 6, 48, 12), (1, 4, 1024, 8))
MEAN_T = (1, 2, 3, 4, 5, 7, 53, 900)


def ratio(err, bnd):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))))


# ------------------------------------------------------------------------------------------------ rne_bf16
def test_rne_bf16_is_torch_cast(tspn):
    x = tspn.hashrng.normal(180, "x", (200001,), std=3.0)
    e = tspn.hashrng.integers(180, "e", x.shape, -140, 128)
    with np.errstate(over="ignore"):
        x = (x.astype(np.float64) * np.exp2(e.astype(np.float64))).astype(np.float32)  # every binade, subnormals and Inf included
    k = np.arange(1 << 16, dtype=np.uint32)
    ties = ((k << np.uint32(16)) | np.uint32(0x8000)).view(np.float32)                 # every exact tie of every bf16 value
    near = np.concatenate([((k << np.uint32(16)) | np.uint32(0x7FFF)).view(np.float32),
                           ((k << np.uint32(16)) | np.uint32(0x8001)).view(np.float32)])
    edge = np.array([0.0, -0.0, 1.0, 1.00390625, 1.001953125, 3.3895314e38, 3.3895312e38, -3.3895314e38, 3.4028235e38,
                     1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -149, np.inf, -np.inf], np.float32)
    allx = np.concatenate([x, ties, near, edge])
    want = torch.from_numpy(allx).to(torch.bfloat16).float().numpy()
    got = br.rne_bf16(allx)
    nan = np.isnan(allx)
    assert nan.any() and np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(br.bits(got)[~nan], br.bits(want)[~nan])
    top = np.array([0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000], np.uint32).view(np.float32)   # the overflow edge: the tie above the largest bf16
    assert np.array_equal(br.rne_bf16(top), np.array([np.inf, 3.3895314e38, -np.inf], np.float32))
    assert float(br.rne_bf16(np.float32(1.00390625))) == 1.0 and float(br.rne_bf16(np.float32(1.01171875))) == 1.015625
    assert np.array_equal(br.rne_bf16(got[~nan]), got[~nan])                           # idempotent


# ------------------------------------------------------------------------------------------------ the budget
@pytest.fixture(scope="module")
def pair_cases(tspn):
    out = {}
    for C in DEPTHS:
        for kind in br.KINDS:
            y, w, b = br.make_pair_case(tspn.hashrng, kind, B, N, C, T, H)
            a = br.pair_activations(y, br.pair_table(B, N))
            out[kind, C] = (y, a, w, b, br.heads_ref64(a, w, b), br.heads_budget(a, w, b))
    return out


def test_the_kinds_are_what_they_say(pair_cases):
    for C in DEPTHS:
        a = {k: pair_cases[k, C][1] for k in br.KINDS}
        ref = {k: pair_cases[k, C][4] for k in br.KINDS}
        S = {k: br.heads_S(pair_cases[k, C][1], pair_cases[k, C][2], pair_cases[k, C][3]) for k in br.KINDS}
        assert 2.0 ** 12 < float(a["large"].max()) < 2.0 ** 16 and float(a["tiny"].max()) < 2.0 ** -97
        assert float(a["subnormal"].max()) < 2.0 ** -126 and bool((a["subnormal"] > 0).any())
        hot = br.hot_index(C, br.K_PAIR)
        assert len(hot) == C // 32 and float(np.median(a["hot_channel"][:, :, hot])) > 100 * float(np.median(a["hot_channel"]))
        assert float(np.abs(ref["cancelling"]).max()) < 0.1 * float(S["cancelling"].min())
        y = pair_cases["relu_edge", C][0]
        dead = float((a["relu_edge"] == 0).mean())
        assert 0.4 < dead < 0.6 and float(a["relu_edge"].max()) < 2.0 ** -8 * float(np.abs(y).max())
        for k in br.KINDS:
            assert bool(np.isfinite(ref[k]).all()) and bool((S[k] > 0).all()), k


@pytest.mark.parametrize("C", DEPTHS)
@pytest.mark.parametrize("kind", br.KINDS)
def test_three_summation_orders_stay_inside_the_heads_budget(pair_cases, kind, C):
    _, a, w, b, ref, bnd = pair_cases[kind, C]
    for order in ORDERS:
        err = np.abs(br.heads_emulate(a, w, b, order=order).astype(np.float64) - ref)
        print(f"{kind} C={C} {order}: max err / budget = {ratio(err, bnd):.3f}")
        assert bool((err <= bnd).all()), (kind, C, order, ratio(err, bnd))


def dropped_channel(kind, a, w):
    """A channel of the last k-step: the last one, but the step's hot channel on `hot_channel` and the step's largest share
    on `wide` (bf16_reference's docstring says why)."""
    C = w.shape[1]
    if kind == "hot_channel":
        return int(br.hot_index(C, br.K_PAIR)[-1])
    if kind == "wide":
        share = np.abs(w[:, C - 32:]).max(0) * a[:, :, C - 32:].max((0, 1))
        return C - 32 + int(np.argmax(share))
    return C - 1


@pytest.mark.parametrize("C", DEPTHS)
@pytest.mark.parametrize("kind", br.KINDS)
def test_truncation_at_the_rounding_point_leaves_the_budget(pair_cases, kind, C):
    y, a, w, b, ref, bnd = pair_cases[kind, C]
    a_t = br.pair_activations(y, br.pair_table(B, N), rnd=br.trunc_bf16)
    assert not np.array_equal(a_t, a)
    err = np.abs(br.heads_emulate(a_t, w, b).astype(np.float64) - ref)
    print(f"{kind} C={C}: truncation, max err / budget = {ratio(err, bnd):.1f}")
    assert ratio(err, bnd) > 1.0


@pytest.mark.parametrize("C", DEPTHS)
@pytest.mark.parametrize("kind", br.KINDS)
def test_a_dropped_channel_of_the_last_k_step_leaves_the_budget(pair_cases, kind, C):
    _, a, w, b, ref, bnd = pair_cases[kind, C]
    err = np.abs(br.heads_emulate(a, w, b, drop=dropped_channel(kind, a, w)).astype(np.float64) - ref)
    print(f"{kind} C={C}: dropped channel, max err / budget = {ratio(err, bnd):.1f}")
    assert ratio(err, bnd) > 1.0


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", br.CONV_KINDS)
def test_three_summation_orders_stay_inside_the_conv_budget(tspn, kind, shape):
    x, w, b = br.make_conv_case(tspn.hashrng, kind, *shape)
    ref, bnd = br.conv_ref64(x, w, b), br.conv_budget(x, w, b)
    assert bool(np.isfinite(ref).all()) and bool((bnd > 0).all())
    for order in ORDERS:
        err = np.abs(br.conv_emulate(x, w, b, order=order).astype(np.float64) - ref)
        print(f"{kind} {shape} {order}: max err / budget = {ratio(err, bnd):.3f}")
        assert bool((err <= bnd).all()), (kind, shape, order, ratio(err, bnd))
    err = np.abs(br.conv_emulate(x, w, b, drop=3 * shape[2] - 1 - (0 if kind != "hot_channel" else
                                                                   15 - int(br.hot_index(shape[2], 16)[-1]) % 16)) - ref)
    print(f"{kind} {shape}: dropped channel, max err / budget = {ratio(err, bnd):.1f}")
    if kind != "wide":      # the last channel's power of two is whatever was drawn: its share of S can lie below the budget
        assert ratio(err, bnd) > 1.0, (kind, shape, ratio(err, bnd))


def test_budget_in_units_of_u_s():
    assert br.K_of(32, 32) == 70 and br.K_of(96, 32) == 74 and br.K_of(2048, 32) == 196
    assert br.K_of(3 * 1024, 16) == 2 * (16 + 192 + 2) and br.K_of(3 * 32, 16) == 48
    assert br.SUBNORMAL_FLOOR == 0.0


# ------------------------------------------------------------------------------------------------ the exact cases
@pytest.mark.parametrize("C", (32, 2048))
@pytest.mark.parametrize("which", br.EXACT_KINDS)
def test_exact_pair_and_dense_cases_are_exact_in_every_order(tspn, which, C):
    for qa, qw in br.Q_PAIRS:
        y, w, b, units = br.exact_pair_case(tspn.hashrng, which, 1, 3, C, 2, qa, qw)
        table = np.array([[0, 1], [2, 0], [1, 1]])
        a = br.pair_activations(y, table)
        want = br.heads_ref64(a, w, b).astype(np.float32)
        assert bool(np.isfinite(want).all()) and bool(((want == 0) | (np.abs(want) >= 2.0 ** -126)).all())
        assert np.array_equal(want[:, H // 2], np.broadcast_to(b[H // 2], want[:, H // 2].shape))     # the all-zero head
        for order in ORDERS:
            assert np.array_equal(br.bits(br.heads_emulate(a, w, b, order=order)), br.bits(want)), (which, C, qa, qw, order)
        if which == "ties":         # truncation gives other bits: the ties decide
            a_t = br.pair_activations(y, table, rnd=br.trunc_bf16)
            assert not np.array_equal(br.bits(br.heads_emulate(a_t, w, b)), br.bits(want))
        yd, wd, bd, _ = br.exact_dense_case(tspn.hashrng, which, 2, C, 3, qa, qw)
        ad = br.dense_activations(yd)
        for order in ORDERS:
            assert np.array_equal(br.bits(br.heads_emulate(ad, wd, bd, order=order)), br.bits(br.heads_ref64(ad, wd, bd).astype(np.float32)))
    print(f"{which} C={C}: {units} units")


@pytest.mark.parametrize("which", ("plain", "zeros"))
def test_exact_conv_cases_are_exact_in_every_order(tspn, which):
    for qa, qw in br.Q_PAIRS:
        x, w, b, units = br.exact_conv_case(tspn.hashrng, which, 1, 4, 1024, 8, qa, qw)
        want = br.conv_ref64(x, w, b).astype(np.float32)
        assert bool(np.isfinite(want).all())
        if which == "zeros":
            assert np.array_equal(want[:, :, 4], np.broadcast_to(b[4], want[:, :, 4].shape))
        for order in ORDERS:
            assert np.array_equal(br.bits(br.conv_emulate(x, w, b, order=order)), br.bits(want)), (which, qa, qw, order)
    print(f"{which}: {units} units")


# ------------------------------------------------------------------------------------------------ the mean
@pytest.mark.parametrize("T_", MEAN_T)
@pytest.mark.parametrize("kind", br.MEAN_KINDS)
def test_mean_emulation_lies_in_the_interval(tspn, kind, T_):
    x = br.make_mean_case(tspn.hashrng, kind, 3, T_, 40)
    lo, hi = br.mean_interval(x)
    got = br.mean_emulate(x)
    assert bool((lo <= hi).all()) and bool(((lo <= got) & (got <= hi)).all())
    wide = float((lo != hi).mean())
    print(f"{kind} T={T_}: {wide:.3f} of the intervals hold two or more bf16 values")
    if T_ == 1:             # the mean of one frame is the frame
        assert np.array_equal(br.bits(got), br.bits(x[:, 0])) and wide == 0.0
    if kind == "cancelling" and T_ >= 2 and T_ % 2 == 0:
        assert float(np.abs(x.astype(np.float64).mean(1)).max()) < 0.1 * float(np.abs(x).mean())


@pytest.mark.parametrize("T_", (1, 2, 3, 4, 8))
def test_exact_mean_cases(tspn, T_):
    ties = 0
    for q in br.Q_MEAN:
        x, want = br.exact_mean_case(tspn.hashrng, 3, T_, 40, q)
        assert np.array_equal(br.bits(br.mean_emulate(x)), br.bits(want)), (T_, q)
        lo, hi = br.mean_interval(x)
        assert bool(((lo <= want) & (want <= hi)).all())
        s = np.ldexp(x.astype(np.float64), -q).sum(1)
        if T_ in (2, 4, 8):     # a tie: sum / T has nine significant bits exactly
            m = np.abs(s / T_)
            sig = m / np.exp2(np.floor(np.log2(np.maximum(m, 1e-300))) - 8)
            ties += int(((sig == np.round(sig)) & (np.round(sig) % 2 == 1) & (m > 0)).sum())
    if T_ in (2, 4, 8):
        assert ties > 20, ties
