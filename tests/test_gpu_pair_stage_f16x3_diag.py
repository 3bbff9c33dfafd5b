"""The diagonal tiles of the split-fp16 pair stage (csrc/pairf16/, tspn_heads_pairgrid_f16x3).  In a tile whose subject
and object block are the same, wave w walks the seven objects (w + 1 + i) & 7 into accumulator slots i = 0 .. 6 and
forms nothing for object w, whose pair (w, w) is not in the canonical table (tspn_heads_pair_f16x3_set_diag_skip, default
on); every other tile walks object i in slot i.  An output's products and their order (channels ascending; hh, hl, lh) do
not depend on the walk or on the tile, so every comparison here is on bits:

  * skip on against skip off, through the C ABI entry into sentinel-held outputs;
  * tracklets permuted so that pairs of a diagonal tile land in an off-diagonal one (which walks as it always did): a
    slot stored to the wrong object fails here;
  * 2^14, the next fp32 past it and NaN in the U and in the V half of tracklet w of a diagonal tile: wave w tracks the
    range of object row w, which it no longer multiplies, because the other waves of the tile read it;
  * the exact-integer cases of tests/pairf16_reference.py with the skip on and off: the activation chain is the one the
    parent had (no switch for it is kept), pinned bit for bit by these and by tests/test_gpu_pair_stage_f16x3_bound.py.

Tile = 8 subjects x 8 objects x 32 frames, 32 channels per k-step."""
import itertools

import numpy as np
import pytest

import pairf16_reference as pr
from test_gpu_pair_stage_f16x3 import bits, exact, launch, pair_table

pytestmark = pytest.mark.gpu

H = 12
TS, TT = 8, 32
# N: one lone diagonal tile (2, 8); a diagonal tile with a ragged off-diagonal neighbour (9); two full blocks (16); three
# blocks, the last one ragged (17).  T: one ragged frame tile; two tiles, the second ragged.  C: one k-step (prologue and
# drain only), an even count, an odd count.
SHAPES = list(itertools.product((1, 2), (2, 8, 9, 16, 17), (32, 64, 96), (6, 34)))


def skip(tspn, on):
    return tspn.ops.heads_pair_f16x3_set_diag_skip(on)


def launch_skip(tspn, device, on, *args, forced=False, **kw):
    prev = skip(tspn, on)
    try:
        return (exact if forced else launch)(tspn, device, *args, **kw)
    finally:
        skip(tspn, prev)


def make(tspn, B, N, C, T, seed=71):
    y = tspn.hashrng.uniform(seed, "y", (B * N, 2 * C, T), -1, 1)
    wh = tspn.hashrng.normal(seed, "wh", (H, C), std=0.1)
    bh = tspn.hashrng.normal(seed, "bh", (H,), std=0.1)
    return y, wh, bh


def test_diag_skip_switch_defaults_on_and_refuses_other_values(tspn, device):
    assert skip(tspn, 1) == 1                          # the default; the call returns the previous setting
    assert skip(tspn, 0) == 1 and skip(tspn, 1) == 0
    assert tspn._abi.lib().tspn_heads_pair_f16x3_set_diag_skip(2) == tspn._abi.TSPN_EINVAL
    assert skip(tspn, 1) == 1                          # a refused value changes nothing


@pytest.mark.parametrize("B,N,C,T", SHAPES, ids=[f"B{s[0]}-N{s[1]}-C{s[2]}-T{s[3]}" for s in SHAPES])
def test_diag_skip_on_equals_skip_off_bit_for_bit(tspn, device, B, N, C, T):
    y, wh, bh = make(tspn, B, N, C, T)
    off = launch_skip(tspn, device, 0, y, wh, bh, B, N)
    on = launch_skip(tspn, device, 1, y, wh, bh, B, N)          # (launch: the sentinels round the output are intact)
    assert np.isfinite(off).all()
    differ = bits(on) != bits(off)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} outputs differ, first at {np.argwhere(differ)[0]}"


def split_by_bit(N, bit):
    """new index -> old index: the tracklets whose index has `bit` clear first, in order, then the others.  Two members
    of one block of 8 that differ in that bit end up in different blocks where N reaches past one block."""
    return np.array([i for i in range(N) if not i >> bit & 1] + [i for i in range(N) if i >> bit & 1])


@pytest.mark.parametrize("B,N,C,T", [(2, 9, 64, 34), (1, 16, 96, 34), (2, 16, 32, 6), (1, 17, 64, 6), (2, 17, 96, 34)])
def test_diag_tile_pairs_keep_their_bits_in_an_off_diagonal_tile(tspn, device, B, N, C, T):
    y, wh, bh = make(tspn, B, N, C, T, seed=72)
    base = launch_skip(tspn, device, 1, y, wh, bh, B, N)
    pairs = pair_table(1, N).numpy()                                # (s, o) of one video, row = s (N - 1) + o - (o > s)
    row_of = {(int(s), int(o)): r for r, (s, o) in enumerate(pairs)}
    moved = np.zeros(len(pairs), dtype=bool)                        # by old row: was diagonal, compared off-diagonal
    for bit in (0, 1, 2):
        perm = split_by_bit(N, bit)
        yp = y.reshape(B, N, 2 * C, T)[:, perm].reshape(B * N, 2 * C, T)
        got = launch_skip(tspn, device, 1, yp, wh, bh, B, N).reshape(B, len(pairs), H, T)
        old_rows = np.array([row_of[(int(perm[s]), int(perm[o]))] for s, o in pairs])
        want = base.reshape(B, len(pairs), H, T)[:, old_rows]
        differ = bits(got) != bits(want)
        assert not differ.any(), (f"bit {bit}: {int(differ.sum())} outputs changed with the tile, first (video, new pair "
                                  f"row, head, frame) {np.argwhere(differ)[0]}")
        was_diag = perm[pairs[:, 0]] // TS == perm[pairs[:, 1]] // TS
        now_off = pairs[:, 0] // TS != pairs[:, 1] // TS
        moved[old_rows[was_diag & now_off]] = True
    diag = pairs[:, 0] // TS == pairs[:, 1] // TS
    assert moved.any() and not (moved & ~diag).any()
    if N == 16:          # two full blocks: the three splits take every pair of a diagonal tile, so every slot of every wave
        assert np.array_equal(moved, diag)


RB, RN, RC, RT = 2, 17, 64, 34
LIM = np.float32(16384.0)
PAST = np.nextafter(LIM, np.float32(np.inf))
# (video, tracklet, frame): wave 3 of block 0 in the first frame tile, wave 4 of block 1 in the ragged second one
SPOTS = [(0, 3, 2), (1, 12, 33)]
VALUES = {"2^14": (LIM, False), "-2^14": (-LIM, False), "past": (PAST, True), "-past": (-PAST, True),
          "nan": (np.float32(np.nan), True)}


@pytest.fixture(scope="module")
def range_base(tspn, device):
    """(y, wh, bh, clean MFMA launch); nobody writes to them.  Channel 5's head weights are scaled down so that a planted
    2^14 leaves the sums where the two paths can be told apart."""
    y, wh, bh = make(tspn, RB, RN, RC, RT, seed=73)
    wh[:, 5] *= np.float32(1e-5)
    return y, wh, bh, launch_skip(tspn, device, 1, y, wh, bh, RB, RN)


@pytest.mark.parametrize("half", [0, 1], ids=["U", "V"])
@pytest.mark.parametrize("name", list(VALUES))
def test_diag_tile_range_vote_is_unchanged(tspn, device, range_base, name, half):
    y, wh, bh, clean = range_base
    value, out_of_range = VALUES[name]
    pairs = pair_table(RB, RN).numpy()
    vid, s, o = pairs[:, 0] // RN, pairs[:, 0] % RN, pairs[:, 1] % RN
    for (b, trk, f) in SPOTS:
        bad = y.copy()
        bad[b * RN + trk, half * RC + 5, f] = value
        on = launch_skip(tspn, device, 1, bad, wh, bh, RB, RN)
        off = launch_skip(tspn, device, 0, bad, wh, bh, RB, RN)
        assert np.array_equal(bits(on), bits(off)), f"{name} at {(b, trk, f)}: skip on and off differ"
        forced = launch_skip(tspn, device, 1, bad, wh, bh, RB, RN, forced=True)
        rows = (vid == b) & ((o if half else s) // TS == trk // TS)        # the tiles that stage the planted value
        hit = np.zeros(on.shape, dtype=bool)
        hit[np.ix_(rows, np.arange(H), np.arange(RT) // TT == f // TT)] = True
        on_diag = hit & ((s // TS == o // TS)[:, None, None])
        assert on_diag.any() and (hit & ~on_diag).any()
        assert np.array_equal(bits(on)[~hit], bits(clean)[~hit]), f"{name}: a tile that does not stage the value changed"
        if out_of_range:
            assert np.array_equal(bits(on)[hit], bits(forced)[hit]), f"{name}: a tile that stages it kept its MFMA sums"
        else:            # in range: the diagonal tile, too, keeps its MFMA sums (the fp32 chain gives other bits at C = 64)
            assert not np.array_equal(bits(on)[on_diag], bits(forced)[on_diag]), f"{name}: the diagonal tile went exact"


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_diag_skip_keeps_the_exact_cases_exact(tspn, device, which, C):
    """N = 9: one full diagonal tile, its ragged neighbours and a lone (8, 8) tile.  float32(ref64) bit for bit, as
    tests/test_gpu_pair_stage_f16x3_bound.py argues, with the skip on and off."""
    N, T = 9, 32
    y, w, q = pr.exact_case(tspn.hashrng, which, C, N=N, T=T, H=H)
    a, _, _ = pr.check_exact_case(y, w, q)
    want = pr.ref64(a, w).astype(np.float32)
    zero = np.zeros(H, np.float32)
    for on in (1, 0):
        got = launch_skip(tspn, device, on, y, w, zero, 1, N)
        wrong = bits(got) != bits(want)
        assert not wrong.any(), f"exact case {which} C={C}, skip {on}: {int(wrong.sum())} outputs off float32(ref64)"
