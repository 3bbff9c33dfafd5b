"""tests/pairf16_reference.py without a device: the emulation of the split-fp16 pair stage meets the budget the GPU tests
hold the kernel to, the two defects the budget exists for break it, and the exact-case generators satisfy their own
preconditions (on which the emulation returns the correctly rounded sum bit for bit)."""
import numpy as np
import pytest

import pairf16_reference as pr

B, N, C, T, H = 2, 9, 64, 30, 12


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases(tspn):
    out = {}
    for kind in pr.KINDS:
        y, w, b = pr.make_case(tspn.hashrng, kind, B, N, C, T, H)
        a = pr.activations(y, B, N)
        out[kind] = (a, w, b, pr.ref64(a, w, b), pr.bound(a, w, b))
    return out


def test_split_carries_22_bits():
    x = np.float32(1.0) + np.arange(0, 1 << 12, 7, dtype=np.float32) * np.float32(2.0 ** -21)      # 22-bit values in [1, 2)
    hi, lo = pr.split(x)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64) / pr.LO, x.astype(np.float64))
    tiny = np.arange(1, 1 << 12, 5, dtype=np.float32) * np.float32(2.0 ** -35)                    # below fp16's normals
    hi, lo = pr.split(tiny)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64) / pr.LO, tiny.astype(np.float64))
    assert float(np.abs(hi).max()) < 2.0 ** -14 and float(np.abs(lo).max()) <= 2.0 ** -14


def test_head_scale_follows_the_scale_kernel():
    w = np.zeros((6, 32), np.float32)
    w[0, 3], w[1, 4], w[2, 5], w[3, 6], w[4, 7], w[5, 0] = 0.75, -2.0 ** -100, 2.0 ** 99 * 1.5, 1.0, -0.4999, 3e-5
    inv, flagged = pr.head_scale(w)
    assert not flagged and np.array_equal(inv, np.ldexp(np.float32(1), [0, -99, 100, 1, -1, -15]).astype(np.float32))
    for h, v in [(1, np.nextafter(np.float32(2.0 ** -100), np.float32(0))), (2, 2.0 ** 100), (0, np.inf), (3, np.nan), (4, 0.0)]:
        bad = w.copy()
        bad[h] = 0
        bad[h, 9] = v
        assert pr.head_scale(bad)[1], (h, v)


@pytest.mark.parametrize("kind", pr.KINDS)
def test_emulation_meets_the_bound(cases, kind):
    a, w, b, ref, bnd = cases[kind]
    err = np.abs(pr.emulate(a, w, b).astype(np.float64) - ref)
    print(f"{kind}: max err / bound = {(err / bnd).max():.3f}, max err / (u S) = {(err / (pr.U * pr.S(a, w, b))).max():.2f}")
    assert bool((err <= bnd).all())
    assert bool((bnd > 0).all())


@pytest.mark.parametrize("kind", ["unit", "heads_2k", "near_limit", "wide_a"])
def test_a_dropped_wl_ah_term_breaks_the_bound(cases, kind):
    a, w, b, ref, bnd = cases[kind]
    err = np.abs(pr.emulate(a, w, b, drop_wl_ah=True).astype(np.float64) - ref)
    print(f"{kind}: max err / bound = {(err / bnd).max():.1f}")
    assert float((err / bnd).max()) > 4.0


@pytest.mark.parametrize("kind", pr.KINDS)
def test_a_wrong_recombination_factor_breaks_the_bound(cases, kind):
    a, w, b, ref, bnd = cases[kind]
    err = np.abs(pr.emulate(a, w, b, lo_inv=2.0 ** -10).astype(np.float64) - ref)
    print(f"{kind}: max err / bound = {(err / bnd).max():.1f}")
    assert float((err / bnd).max()) > 4.0


@pytest.mark.parametrize("C", [32, 64, 96])
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_exact_cases_hold_their_preconditions_and_the_emulation_is_exact(tspn, which, C):
    y, w, q = pr.exact_case(tspn.hashrng, which, C)
    a, n_hi, n_lo = pr.check_exact_case(y, w, q)
    print(f"{which} C={C}: {n_hi} units in acc_hi, {n_lo} in acc_lo")
    assert set(q) == set(pr.Q_EXTREMES)
    if which == "A":
        assert float(a[a > 0].min()) >= 32 and float(a.max()) < 64
    elif which == "B":
        assert set(np.unique(a)) <= set(range(8)) and float(a.max()) == 7
    else:
        ah, al = pr.split(a)
        assert float(a[a > 0].min()) >= 2.0 ** -17 and float(a.max()) < 2.0 ** -16
        assert float(np.abs(ah).max()) < 2.0 ** -14 and float(np.abs(al).max()) <= 2.0 ** -14 and al.any()
    want = pr.ref64(a, w).astype(np.float32)
    assert np.array_equal(bits(pr.emulate(a, w)), bits(want))
    # the fp32 chain rounds the 28-bit products of A one by one: other bits (what the GPU test uses to show the MFMAs ran)
    if which == "A":
        s = np.zeros(want.shape, np.float32)
        for c in range(C):
            s = (w[None, :, c, None].astype(np.float64) * a[:, None, c, :] + s).astype(np.float32)
        assert not np.array_equal(bits(s), bits(want))
