"""tests/frontend_nonfinite_reference.py without a card: the float64 conv, ReLU and pool that the front end's non-finite
tests compare against follow torch's rules, and every case of tests/test_gpu_nonfinite_frontend.py has a reference
that cannot pass emptily (a NaN came out, an infinity came out where one went in, at least half of the outputs are
finite and unchanged)."""
import numpy as np
import pytest
import torch

import conv2d_edge_cases as ce
import frontend_nonfinite_reference as fr
from oracle import roi_head_oracle as ro

GEOMS = [ce.Geom(3, 3, 1, 1, 5, 4), ce.Geom(3, 1, 2, 1, 6, 7), ce.Geom(7, 7, 2, 3, 9, 10), ce.Geom(1, 1, 3, 0, 7, 8)]


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: f"k{g.KH}x{g.KW}s{g.stride}p{g.pad}")
def test_conv2d_ref_equals_torch_float64_on_finite_inputs(g):
    """Stride, padding, bias, residual and ReLU against F.conv2d in float64; the two differ by the order of the sums."""
    x, w, b, r = ce.real_operands(16, 8, g, 2)
    w = np.where(w == 0, np.float32(0.125), w)
    for bias, res, relu in ((None, None, False), (b, None, True), (b, r, True)):
        got = fr.conv2d_ref(x, w, bias, g.stride, g.pad, res, relu)
        want = ce.reference(x, w, g, bias, res, relu).numpy()
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: f"k{g.KH}x{g.KW}s{g.stride}p{g.pad}")
def test_conv2d_bf16_ref_equals_the_oracle_bit_for_bit_on_bf16_exact_inputs(g):
    """Small-integer operands (every partial sum exact in any order): the rounding points are the oracle's."""
    x, w, b, r = ce.exact_operands(64, 32, g, 2)
    assert (w != 0).any()
    got = fr.conv2d_bf16_ref(x, w, b, g.stride, g.pad, r, True)
    want = ro.conv2d_bf16(fr.t(x).permute(0, 3, 1, 2), fr.t(w), fr.t(b), g.stride, g.pad,
                          fr.t(r).permute(0, 3, 1, 2), True).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    assert float(np.abs(got).max()) > 1


def test_inf_times_zero_is_nan_and_an_infinity_reaches_only_its_windows():
    g = ce.Geom(3, 3, 1, 1, 5, 4)
    x, w, b, _ = ce.real_operands(16, 8, g, 2)
    w = np.where(w == 0, np.float32(0.125), w)
    x = np.array(x)
    x[0, 2, 2, 5] = np.inf
    ref = fr.conv2d_ref(x, w, b, 1, 1)
    hit = np.zeros(ref.shape[:3], bool)
    hit[0, 1:4, 1:4] = True
    assert np.isinf(ref[hit]).all() and np.isfinite(ref[~hit]).all()
    np.testing.assert_array_equal(np.sign(ref[0, 2, 2]), np.sign(w[:, 5, 1, 1]))
    w[3, 5] = 0.0                                       # the one planted zero weight
    ref = fr.conv2d_ref(x, w, b, 1, 1)
    assert np.isnan(ref[hit][:, 3]).all() and np.isinf(np.delete(ref[hit], 3, axis=1)).all()
    assert np.isfinite(ref[~hit]).all()


def test_relu_keeps_nan_and_clamps_minus_infinity():
    for nan in fr.NANS:
        y = fr.conv2d_ref(np.full((1, 1, 1, 1), nan), np.ones((2, 1, 1, 1)), relu=True)
        assert np.isnan(y).all()
    v = np.array([np.nan, -np.inf, np.inf, -1.0, 2.0])
    np.testing.assert_array_equal(fr.relu64(v), torch.relu(fr.t(v)).numpy())
    assert np.isnan(fr.relu64(v)[0]) and fr.relu64(v)[1] == 0 and fr.relu64(v)[2] == np.inf


@pytest.mark.parametrize("k,s,p", fr.POOL_KSP)
def test_pool_window_rules(k, s, p):
    """A window with a NaN is NaN, a window of only -Inf is -Inf, padding does not take part; torch agrees."""
    x = np.full((1, 5, 7, 2), -2.0)
    x[0, 2, 3, 0] = np.nan
    x[0, :, :, 1] = -np.inf
    got = fr.max_pool_ref(x, k, s, p)
    want = torch.nn.functional.max_pool2d(fr.t(x).permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1).numpy()
    assert fr.same_bits(got, want).all()
    assert np.isneginf(got[..., 1]).all()
    assert np.isnan(got[..., 0]).any() and (got[..., 0][~np.isnan(got[..., 0])] == -2.0).all()


# ------------------------------------------------------------------------------------------------ the cases are not empty
@pytest.mark.parametrize("plant", fr.PLANT_IDS)
@pytest.mark.parametrize("form", fr.CONV_FORMS)
def test_conv_rule_cases_are_not_empty(form, plant):
    c = fr.conv_case(form, plant)
    fr.check_not_empty(c[-1], c[-2], True, f"{form} {plant}")
    if plant == "inf0":
        assert (c[4][0, 1] == 0).all() and int((c[4] == 0).sum()) == c[4][0, 1].size


@pytest.mark.parametrize("ksp", fr.POOL_KSP)
@pytest.mark.parametrize("C", fr.POOL_C)
@pytest.mark.parametrize("shape", fr.POOL_MAPS)
def test_pool_rule_cases_hold_every_planted_kind(shape, C, ksp):
    k, s, p = ksp
    x, xp = fr.pool_case(shape, C, ksp)
    H, W = shape[1:]
    if H + 2 * p < k or W + 2 * p < k:
        return                                          # no output: the entry refuses (tests/test_gpu_frontend_edges.py)
    ref = fr.max_pool_ref(xp, k, s, p)
    assert np.isposinf(ref).any() and np.isneginf(ref).any()
    fr.check_not_empty(ref, fr.max_pool_ref(x, k, s, p), True, f"pool {shape} C={C} {ksp}")


@pytest.mark.parametrize("shape", sorted(set(fr.STEM_SHAPES + fr.STEM_POOL_SHAPES)))
def test_stem_cases_are_not_empty(shape):
    x, xp, w, b, rc, rp, pc, pp = fr.stem_case(*shape)
    if shape in fr.STEM_SHAPES:
        fr.check_not_empty(rp, rc, True, f"stem conv {shape}")
    if shape in fr.STEM_POOL_SHAPES:
        fr.check_not_empty(pp, pc, True, f"stem pool {shape}")


@pytest.mark.parametrize("shape", fr.TAIL_SHAPES)
def test_tail_cases_are_not_empty_and_the_residual_reaches_one_element(shape):
    h1, h1p, res, resp, w2, b2, w3, b3, rc, rp = fr.tail_case(*shape)
    fr.check_not_empty(rp, rc, True, f"tail {shape}")
    at = tuple(np.argwhere(resp != res)[0])
    assert len(np.argwhere(resp != res)) == 1 and np.isposinf(rp[at])
    near = rp[at[0], at[1], at[2]]
    assert np.isfinite(np.delete(near, at[3])).all(), "the residual's element lies inside a planted pixel's neighbourhood"


@pytest.mark.parametrize("kind,shape", [("id", s) for s in fr.BLOCK_SHAPES] + [("proj", (64, 1, 11, 31)), ("res", (128, 1, 13, 61))])
def test_block_cases_are_not_empty(kind, shape):
    c = fr.block_case(kind, *shape)
    fr.check_not_empty(c["ref_p"], c["ref_c"], True, f"block {kind} {shape}")
    if kind == "res":
        odd = fr._block_ref(c["xodd"], c["res"], c["w1"], c["w2"], c["w3"], c["ws"], c["b"], c["stride"])
        assert fr.same_bits(odd, c["ref_c"]).all(), "the odd coordinate is read by a tap"
