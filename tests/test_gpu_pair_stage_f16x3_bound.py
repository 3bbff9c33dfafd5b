"""The split-fp16 pair stage (csrc/pairf16/, tspn_heads_pairgrid_f16x3) against float64 at a RELATIVE bound, and on
inputs where the split must give the correctly rounded sum bit for bit.  The budget, its derivation, the six
distributions and the exact-case generators are tests/pairf16_reference.py (host side:
tests/test_pairf16_reference_host.py).  With u = 2^-24 and S = |b_h| + sum_c |w_hc| a_c:

    MFMA path:   |got - ref64| <= (20 + C / 32) u S + 2^-35 (wmax_h sum_c a_c + sum_c |w_hc|)
    fp32 chain:  |got - ref64| <= (C + 2) u S            (set_force_exact(1): the fallback of a tile)

Measured on an MI355X (profiles/r25/README.md has the table), max |err| / (u S) at C = 64, where K = 22: unit 3.6, tiny_a
1.0, heads_2k 3.6, hot_weight 6.4, near_limit 2.7, wide_a 7.5 on the MFMA path; 4.4, 1.0, 4.4, 9.5, 4.9, 6.3 on the chain."""
import numpy as np
import pytest

import pairf16_reference as pr
from test_gpu_pair_stage_f16x3 import bits, exact, launch

pytestmark = pytest.mark.gpu

H = 12
CASES = [(kind, 2, 9, 64, 30) for kind in pr.KINDS] + [("unit", 2, 9, 32, 30), ("unit", 1, 17, 96, 36), ("unit", 2, 9, 256, 8)]


def check_bound(got, a, w, b, what):
    """|got - ref64| <= bound elementwise; prints max |err| / (u S) and returns it."""
    ref, bnd, s = pr.ref64(a, w, b), pr.bound(a, w, b), pr.S(a, w, b)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = float(np.nanmax(np.where(s > 0, err / (pr.U * s), 0.0)))
    print(f"{what}: MFMA path max |err| / (u S) = {rel:.2f}, max |err| / bound = {float((err / bnd).max()):.3f}")
    worst = np.unravel_index(np.argmax(err / bnd), err.shape)
    assert bool((err <= bnd).all()), f"{what}: |err| = {err[worst]:.3e} > bound {bnd[worst]:.3e} at (pair, head, frame) {worst}"
    return rel


def check_chain(forced, a, w, b, what):
    ref, s = pr.ref64(a, w, b), pr.S(a, w, b)
    err = np.abs(forced.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = float(np.nanmax(np.where(s > 0, err / (pr.U * s), 0.0)))
    print(f"{what}: fp32 chain max |err| / (u S) = {rel:.2f}")
    assert bool((err <= pr.chain_bound(a, w, b)).all()), f"{what}: the fp32 chain misses (C + 2) u S"
    return rel


@pytest.mark.parametrize("kind,B,N,C,T", CASES, ids=[f"{c[0]}-C{c[3]}-N{c[2]}-T{c[4]}" for c in CASES])
def test_pair_stage_f16x3_meets_the_relative_bound(tspn, device, kind, B, N, C, T):
    y, w, b = pr.make_case(tspn.hashrng, kind, B, N, C, T, H)
    a = pr.activations(y, B, N)
    got = launch(tspn, device, y, w, b, B, N)
    forced = exact(tspn, device, y, w, b, B, N)
    what = f"{kind} {(B, N, C, T)}"
    check_bound(got, a, w, b, what)
    check_chain(forced, a, w, b, what)
    assert not np.array_equal(bits(got), bits(forced)), f"{what}: the MFMA path did not run (bits of the fp32 chain)"


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_pair_stage_f16x3_is_exact_where_the_split_is(tspn, device, which, C):
    """A: activations carry 22 bits, B: weights carry 22 bits, C: ah and al are fp16 subnormals; per-head scales 2^-90 ..
    2^90 in one call.  Every addend of either accumulator is an integer multiple of one unit and their absolute sum is
    below 2^24 units (asserted in integers by check_exact_case before the launch), so any summation order is exact and
    the epilogue's one fma rounds once: the output is float32(ref64) bit for bit.  No bias."""
    N, T = 9, 32
    y, w, q = pr.exact_case(tspn.hashrng, which, C, N=N, T=T, H=H)
    a, n_hi, n_lo = pr.check_exact_case(y, w, q)
    want = pr.ref64(a, w).astype(np.float32)
    zero = np.zeros(H, np.float32)
    got = launch(tspn, device, y, w, zero, 1, N)
    off = bits(got) != bits(want)
    print(f"exact case {which} C={C}: {n_hi} / {n_lo} units, {int(off.sum())} of {off.size} outputs off")
    assert not off.any(), (f"exact case {which} C={C}: {int(off.sum())} outputs differ from float32(ref64), worst "
                           f"{np.abs(got.astype(np.float64) - want).max():.3e} at |ref| up to {np.abs(want).max():.3e}")
    assert np.array_equal(bits(launch(tspn, device, y, w, None, 1, N)), bits(want))
    if which == "A":        # the fp32 chain rounds 28-bit products one by one: the bits above are the MFMA path's
        assert not np.array_equal(bits(exact(tspn, device, y, w, zero, 1, N)), bits(want))
