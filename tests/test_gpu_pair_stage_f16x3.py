"""The fp32 path's pair stage on split-fp16 MFMAs (csrc/pairf16/, tspn_heads_pairgrid_f16x3): against float64 at the
tile edges, the per-tile fp32 chain on out-of-range and non-finite values, and the fused pass that runs it.

Tile = 8 subjects x 8 objects x 32 frames.  A tile takes the fp32 chain when a value it stages for a written output (a
real tracklet's row, a frame < T) is not <= 2^14 in magnitude -- each half of y on its own, not their sum -- and every
tile does when a head's weights are non-finite, all below 2^-100, or reach 2^100.  Rows of y are padded to ldt >=
ceil4(T) frames; the pad frames hold NaN here unless a test says otherwise and must never matter.  The tests from the
range rule's threshold on use the relative bound of tests/pairf16_reference.py (tests/test_gpu_pair_stage_f16x3_bound.py)."""
import numpy as np
import pytest
import torch

import oracle
import pairf16_reference as pr
import workspace_contract as wsc
from sentinel_buffers import assert_untouched, assert_written_inside_only, held
from test_gpu_kernel_variants import fused_weights
from test_gpu_nonfinite import assert_same_nonfinite

pytestmark = pytest.mark.gpu

ATOL = 2e-5          # the bound test_heads_pairgrid_matches_generic holds the fp32 pair stage to
TS, TO, TT = 8, 8, 32


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def pair_table(B, N):
    return torch.cat([oracle.pair_index(N) + b * N for b in range(B)])


def ref64(y, wh, bh, B, N):
    """y [B*N, 2C, T] -> float64 [P, H, T]: relu(y_s + y_o) contracted with Wh, as test_heads_pairgrid_matches_generic."""
    C = y.shape[1] // 2
    pairs, yy = pair_table(B, N), t(y).double()
    h = torch.relu(yy[pairs[:, 0], :C] + yy[pairs[:, 1], C:])
    with np.errstate(all="ignore"):
        return (torch.einsum("hc,pct->pht", t(wh).double(), h) + t(bh).double().view(1, -1, 1)).numpy()


def launch(tspn, device, y, wh, bh, B, N, ldt=None, pad=None, split_buf=None):
    """The entry on y padded to ldt (default ceil4(T)) frames per row, output held between sentinel guards.  The pad
    frames hold NaN, or `pad` [NT, 2C, ldt - T]; bh may be None (no bias)."""
    NT, C2, T = y.shape
    ldt = (T + 3) // 4 * 4 if ldt is None else ldt
    yp = torch.full((NT, C2, ldt), float("nan"))
    yp[:, :, :T] = t(y)
    if pad is not None:
        yp[:, :, T:] = t(pad)
    buf, out = held((B * N * (N - 1), wh.shape[0], T), device)
    tspn.ops.heads_pairgrid_f16x3(yp.to(device), B, N, t(wh).to(device), None if bh is None else t(bh).to(device), T=T,
                                  split_buf=split_buf, out=out)
    assert_written_inside_only(buf, out, "heads_pairgrid_f16x3")
    return out.cpu().numpy()


def exact(tspn, device, *args, **kw):
    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        return launch(tspn, device, *args, **kw)
    finally:
        tspn.ops.heads_pairgrid_f16x3_set_force_exact(prev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# (B, N, C, T): one tile with a 4-frame row; ragged subject / object blocks and a short frame block; N past two blocks and
# a second frame block; five frame blocks, the last one ragged (a second round of the workgroup map: 15 groups > 8); N past
# four blocks with a quarter frame block
SHAPES = [(1, 2, 32, 4), (2, 9, 64, 30), (1, 17, 96, 36), (3, 8, 32, 148), (2, 33, 64, 8)]


@pytest.mark.parametrize("B,N,C,T,H,kind", [s + (12, "unit") for s in SHAPES] +
                         [(2, 9, 64, 30, 1, "unit"), (2, 9, 64, 30, 5, "unit"), (2, 9, 64, 30, 16, "unit"),
                          (2, 9, 64, 30, 12, "small_w"), (2, 9, 64, 30, 12, "large_a")])
def test_pair_stage_f16x3_vs_fp64(tspn, device, B, N, C, T, H, kind):
    """`unit`: y in U(-1, 1), weights N(0, 0.1), as test_heads_pairgrid_matches_generic.  `small_w`: weights N(0, 1e-4), the
    per-head power-of-two scale at work.  `large_a`: activations near 1e4 (each half of y near 5e3, inside the MFMA
    range).  An fp32 output can meet an absolute 2e-5 only while its half ulp does, i.e. below 2^8; with a near 1e4
    that asks for weights N(0, 1e-4) (outputs near 10), so that case uses them as well."""
    y = tspn.hashrng.uniform(61, "y", (B * N, 2 * C, T), -1, 1)
    if kind == "large_a":
        y = y + np.float32(5000.0)
    wh = tspn.hashrng.normal(61, "wh", (H, C), std=0.1 if kind == "unit" else 1e-4)
    bh = tspn.hashrng.normal(61, "bh", (H,), std=0.1)
    got = launch(tspn, device, y, wh, bh, B, N)
    ref = ref64(y, wh, bh, B, N)
    print(f"{kind} {(B, N, C, T, H)}: max |err| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    if kind == "large_a":      # (the MFMA form ran: the fp32 chain gives other bits at this depth)
        assert not np.array_equal(bits(got), bits(exact(tspn, device, y, wh, bh, B, N)))


B2, N2, C2, T2, H2 = 2, 17, 64, 36, 12
# (video, tracklet, half (0 = U, 1 = V), channel, frame, value): four different tiles
PLANTS = [(0, 3, 0, 5, 2, np.float32(7e4)), (0, 12, 1, 9, 33, np.float32(np.inf)),
          (1, 16, 0, 0, 35, np.float32(-np.inf)), (1, 1, 1, 63, 0, np.float32(np.nan))]


def affected_rows(plants=None):
    """[P, T] bool: outputs of a tile that stages a planted value."""
    pairs = pair_table(B2, N2).numpy()
    vid, s, o = pairs[:, 0] // N2, pairs[:, 0] % N2, pairs[:, 1] % N2
    hit = np.zeros((pairs.shape[0], T2), dtype=bool)
    for (b, trk, half, _, f, _) in (PLANTS if plants is None else plants):
        row = (vid == b) & ((o if half else s) // (TO if half else TS) == trk // TS)
        hit[np.ix_(row, np.arange(T2) // TT == f // TT)] = True
    return hit


def test_pair_stage_f16x3_range_and_nonfinite_tiles(tspn, device):
    """7e4 (past the fp16 range), +Inf, -Inf and NaN, each in another tile.  The 7e4 sits on a channel whose head weights
    are scaled to 1e-6, so that the float64 sums stay where fp32 can meet 2e-5."""
    y = tspn.hashrng.uniform(62, "y", (B2 * N2, 2 * C2, T2), -1, 1)
    wh = tspn.hashrng.normal(62, "wh", (H2, C2), std=0.1)
    wh[:, 5] *= np.float32(1e-5)
    bh = tspn.hashrng.normal(62, "bh", (H2,), std=0.1)
    bad = y.copy()
    for (b, trk, half, c, f, v) in PLANTS:
        bad[b * N2 + trk, half * C2 + c, f] = v
    clean = launch(tspn, device, y, wh, bh, B2, N2)
    got = launch(tspn, device, bad, wh, bh, B2, N2)
    forced = exact(tspn, device, bad, wh, bh, B2, N2)
    ref = ref64(bad, wh, bh, B2, N2)
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()
    assert_same_nonfinite(got, ref, ATOL, "planted")
    assert_same_nonfinite(forced, ref, ATOL, "planted, fp32 chain")
    hit = np.broadcast_to(affected_rows()[:, None, :], got.shape)
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(got)[hit], bits(forced)[hit]), "an affected tile kept its MFMA sums"
    assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), "an untouched tile changed"
    assert not np.array_equal(bits(clean)[hit], bits(exact(tspn, device, y, wh, bh, B2, N2))[hit])   # clean: MFMA sums


@pytest.mark.parametrize("what", ["zero_head", "inf_weight"])
def test_pair_stage_f16x3_flagged_weights_take_the_fp32_chain(tspn, device, what):
    y = tspn.hashrng.uniform(63, "y", (B2 * N2, 2 * C2, T2), -1, 1)
    wh = tspn.hashrng.normal(63, "wh", (H2, C2), std=0.1)
    bh = tspn.hashrng.normal(63, "bh", (H2,), std=0.1)
    if what == "zero_head":
        wh[7, :] = 0.0
    else:
        wh[2, 40] = np.inf
    got, forced = launch(tspn, device, y, wh, bh, B2, N2), exact(tspn, device, y, wh, bh, B2, N2)
    assert np.array_equal(bits(got), bits(forced))
    assert_same_nonfinite(got, ref64(y, wh, bh, B2, N2), ATOL, what)


# ------------------------------------------------------------------------------------------------ the range rule at 2^14
LIM = np.float32(16384.0)
PAST = np.nextafter(LIM, np.float32(np.inf))
# name -> (plants (video, tracklet, half, channel, frame, value), how many of them -- the first ones -- are out of range).
# The rule is per half: |u| <= 2^14 and |v| <= 2^14, whatever u + v is.  All on channel 5, whose head weights are scaled down.
AT_THE_LIMIT = {
    "u=+2^14": ([(0, 3, 0, 5, 2, LIM)], 0),
    "u=-2^14": ([(0, 3, 0, 5, 2, -LIM)], 0),
    "v=+2^14": ([(1, 12, 1, 5, 33, LIM)], 0),
    "v=-2^14": ([(1, 12, 1, 5, 33, -LIM)], 0),
    "u=v=2^14": ([(0, 3, 0, 5, 2, LIM), (0, 10, 1, 5, 2, LIM)], 0),                # a = 2^15 on pair (3, 10)
    "u>2^14": ([(0, 3, 0, 5, 2, PAST)], 1),
    "u<-2^14": ([(0, 3, 0, 5, 2, -PAST)], 1),
    "v>2^14": ([(1, 12, 1, 5, 33, PAST)], 1),
    "v<-2^14": ([(1, 12, 1, 5, 33, -PAST)], 1),
    # u + v = 2 on pair (3, 10), u out of range: the subject block's tiles take the chain, the object block's others stay
    "u=2^14+2,v=-2^14": ([(0, 3, 0, 5, 2, LIM + np.float32(2.0)), (0, 10, 1, 5, 2, -LIM)], 1),
}


@pytest.fixture(scope="module")
def range_base(tspn, device):
    """(y, wh, bh, the clean launch, the clean launch on the fp32 chain) at (2, 17, 64, 36); nobody writes to them."""
    y = tspn.hashrng.uniform(62, "y", (B2 * N2, 2 * C2, T2), -1, 1)
    wh = tspn.hashrng.normal(62, "wh", (H2, C2), std=0.1)
    wh[:, 5] *= np.float32(1e-5)
    bh = tspn.hashrng.normal(62, "bh", (H2,), std=0.1)
    return y, wh, bh, launch(tspn, device, y, wh, bh, B2, N2), exact(tspn, device, y, wh, bh, B2, N2)


def assert_within_f16x3_bound(got, y, wh, bh, B, N, what):
    """The relative bound of tests/test_gpu_pair_stage_f16x3_bound.py (tests/pairf16_reference.py)."""
    a = pr.activations(y, B, N)
    err, bnd = np.abs(got.astype(np.float64) - pr.ref64(a, wh, bh)), pr.bound(a, wh, bh)
    print(f"{what}: max |err| / bound = {float((err / bnd).max()):.3f}")
    assert bool((err <= bnd).all()), f"{what}: max |err| / bound = {float((err / bnd).max()):.3f}"


@pytest.mark.parametrize("name", list(AT_THE_LIMIT))
def test_pair_stage_f16x3_range_rule_at_its_threshold(tspn, device, range_base, name):
    """One value (or one u and one v of the same channel and frame) per launch.  Exactly 2^14 in either half and either
    sign keeps the tile on MFMAs (a = 2^15 included); the next fp32 past it sends the tile, and only that tile, through
    the fp32 chain -- also when the other half cancels it."""
    y, wh, bh, clean, _ = range_base
    plants, n_out = AT_THE_LIMIT[name]
    bad = y.copy()
    for (b, trk, half, c, f, v) in plants:
        bad[b * N2 + trk, half * C2 + c, f] = v
    got = launch(tspn, device, bad, wh, bh, B2, N2)
    forced = exact(tspn, device, bad, wh, bh, B2, N2)
    hit = np.broadcast_to(affected_rows(plants)[:, None, :], got.shape)
    flip = np.broadcast_to(affected_rows(plants[:n_out])[:, None, :], got.shape)      # the tiles that must take the chain
    stay = hit & ~flip
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), "an untouched tile changed"
    assert np.array_equal(bits(got)[flip], bits(forced)[flip]), "a tile past 2^14 kept its MFMA sums"
    if stay.any():
        assert not np.array_equal(bits(got)[stay], bits(forced)[stay]), "a tile left the MFMAs at 2^14"
        assert not np.array_equal(bits(got)[stay], bits(clean)[stay])        # (the planted value reached its outputs)
    assert flip.any() == (n_out > 0) and stay.any() == (n_out < len(plants))
    a = pr.activations(bad, B2, N2)
    err = np.abs(got.astype(np.float64) - pr.ref64(a, wh, bh))
    bnd = np.where(flip, pr.chain_bound(a, wh, bh), pr.bound(a, wh, bh))
    print(f"{name}: max |err| / bound = {float((err / bnd).max()):.3f}")
    assert bool((err <= bnd).all()), f"{name}: max |err| / bound = {float((err / bnd).max()):.3f}"


def _tiles_differ(a, b):
    """Every tile of (a, b) [P, H, T] differs somewhere: (video, subject block, object block, frame block)."""
    pairs = pair_table(B2, N2).numpy()
    key = (pairs[:, 0] // N2) * 10000 + (pairs[:, 0] % N2 // TS) * 100 + pairs[:, 1] % N2 // TO
    for k in np.unique(key):
        for f0 in range(0, a.shape[2], TT):
            if np.array_equal(bits(a)[key == k][:, :, f0:f0 + TT], bits(b)[key == k][:, :, f0:f0 + TT]):
                return False
    return True


@pytest.mark.parametrize("pad", ["nan", "one_7e4", "all_bad"])
@pytest.mark.parametrize("ldt", [T2 + 8, 64])
def test_pair_stage_f16x3_frames_past_t_reach_nothing(tspn, device, range_base, ldt, pad):
    """ldt > ceil4(T) is legal.  Frames [T, ldt) are staged with the last frame block (T = 36: frames 32 .. 63 of the
    block, of which [36, ldt) exist) but feed no written output: whatever they hold -- NaN, one 7e4, or 7e4 / NaN / +Inf /
    -Inf on every one of them -- the output is the tight launch's bit for bit, so no tile took the fp32 chain."""
    y, wh, bh, clean, clean_chain = range_base
    assert _tiles_differ(clean, clean_chain)            # bit equality with `clean` below = every tile ran on MFMAs
    NT, n = y.shape[0], ldt - T2
    if pad == "nan":
        fill = None
    elif pad == "one_7e4":
        fill = tspn.hashrng.uniform(64, "pad", (NT, 2 * C2, n), -1, 1)
        fill[3, 5, 41 - T2] = 7e4
    else:
        vals = np.array([7e4, np.nan, np.inf, -np.inf], np.float32)
        fill = vals[tspn.hashrng.integers(64, "bad", (NT, 2 * C2, n), 0, 4)]
    got = launch(tspn, device, y, wh, bh, B2, N2, ldt=ldt, pad=fill)
    assert np.array_equal(bits(got), bits(clean))


# ------------------------------------------------------------------------------------------------ weight flags at their edges
def _edge_weights(tspn, what):
    wh = tspn.hashrng.normal(65, "wh", (H2, C2), std=0.1)
    bh = tspn.hashrng.normal(65, "bh", (H2,), std=0.1)
    top = {"2^-100": 2.0 ** -100, "below_2^-100": float(np.nextafter(np.float32(2.0 ** -100), np.float32(0))),
           "below_2^100": float(np.nextafter(np.float32(2.0 ** 100), np.float32(0))), "2^100": 2.0 ** 100}.get(what)
    if top is not None:
        row = wh[7].astype(np.float64)
        wh[7] = (row / np.abs(row).max() * top).astype(np.float32)
        bh[7] = np.float32(float(bh[7]) * top)
        assert float(np.abs(wh[7]).max()) == float(np.float32(top))
    elif what == "nan":
        wh[2, 40] = np.nan
    return wh, bh


@pytest.mark.parametrize("what,mfma", [("2^-100", True), ("below_2^-100", False), ("below_2^100", True), ("2^100", False),
                                       ("nan", False)])
def test_pair_stage_f16x3_weight_flags_at_their_edges(tspn, device, what, mfma):
    """A head whose largest |w| is exactly 2^-100, or just below 2^100, is scaled and runs on MFMAs; one ulp below
    2^-100, at 2^100, or with a NaN weight, every tile takes the fp32 chain.  Held to the relative bounds of
    tests/pairf16_reference.py (head 7's bias is scaled with its weights, so its S is the head's own)."""
    B, N, C, T = 2, 9, C2, 30
    y = tspn.hashrng.uniform(65, "y", (B * N, 2 * C, T), -1, 1)
    wh, bh = _edge_weights(tspn, what)
    assert pr.head_scale(wh)[1] == (not mfma)
    got, forced = launch(tspn, device, y, wh, bh, B, N), exact(tspn, device, y, wh, bh, B, N)
    a = pr.activations(y, B, N)
    with np.errstate(all="ignore"):
        ref = pr.ref64(a, wh, bh)
        fin = np.isfinite(ref)
        chain = pr.chain_bound(a, np.nan_to_num(wh), bh)
    assert_same_nonfinite(got, ref, np.inf, what)
    assert (what == "nan") == bool((~fin).any())
    assert bool((np.abs(forced.astype(np.float64) - ref)[fin] <= chain[fin]).all()), f"{what}: the fp32 chain misses (C + 2) u S"
    if mfma:
        assert not np.array_equal(bits(got), bits(forced)), f"{what}: the MFMA path did not run"
        assert_within_f16x3_bound(got, y, wh, bh, B, N, what)
        assert float(np.abs(got[:, 7]).max()) > 0
    else:
        assert np.array_equal(bits(got), bits(forced)), f"{what}: flagged weights kept an MFMA tile"


def test_pair_stage_f16x3_without_a_bias(tspn, device):
    """head_b = NULL is a zero bias, bit for bit, on the MFMA path and on the fp32 chain."""
    B, N, C, T = 2, 9, C2, 30
    y = tspn.hashrng.uniform(66, "y", (B * N, 2 * C, T), -1, 1)
    wh = tspn.hashrng.normal(66, "wh", (H2, C), std=0.1)
    zero = np.zeros(H2, np.float32)
    got, forced = launch(tspn, device, y, wh, None, B, N), exact(tspn, device, y, wh, None, B, N)
    assert np.array_equal(bits(got), bits(launch(tspn, device, y, wh, zero, B, N)))
    assert np.array_equal(bits(forced), bits(exact(tspn, device, y, wh, zero, B, N)))
    assert not np.array_equal(bits(got), bits(forced))
    assert_within_f16x3_bound(got, y, wh, None, B, N, "no bias")


# ------------------------------------------------------------------------------------------------ refusals and empty calls
def _offset_by_4_bytes(x, device):
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=device)
    v = flat[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# name -> (C, T, ldt, H, what is offset by 4 bytes)
REFUSED = {"odd T": (64, 31, 32, 12, None), "C % 32": (48, 30, 32, 12, None), "H = 17": (64, 30, 32, 17, None),
           "ldt % 4": (64, 30, 30, 12, None), "y misaligned": (64, 30, 32, 12, "y"), "out misaligned": (64, 30, 32, 12, "out")}


@pytest.mark.parametrize("name", list(REFUSED))
def test_pair_stage_f16x3_refuses_what_it_cannot_run(tspn, device, name):
    """TSPN_EUNSUPPORTED before any device work: the sentinel-filled output and the 0xFF split buffer keep every byte."""
    E = tspn._abi
    C, T, ldt, H, off = REFUSED[name]
    B, N = 2, 9
    y = t(tspn.hashrng.uniform(67, "y", (B * N, 2 * C, ldt), -1, 1)).to(device)
    wh = t(tspn.hashrng.normal(67, "wh", (H, C), std=0.1)).to(device)
    bh = t(tspn.hashrng.normal(67, "bh", (H,), std=0.1)).to(device)
    if off == "y":
        y = _offset_by_4_bytes(y, device)
    buf, out = held((B * N * (N - 1), H, T), device, offset=1 if off == "out" else 0)
    assert out.data_ptr() % 8 == (4 if off == "out" else 0)
    sbuf, split = wsc.guarded_ws(tspn.ops.heads_pairgrid_f16x3_split_bytes(64, 12), device, "ones")
    with pytest.raises(E.TspnError) as e:
        tspn.ops.heads_pairgrid_f16x3(y, B, N, wh, bh, T=T, split_buf=split, out=out)
    assert e.value.code == E.TSPN_EUNSUPPORTED, f"{name}: {e.value}"
    torch.cuda.synchronize(device)
    assert_untouched(buf, name)
    wsc.assert_all_ones(split, name)
    wsc.assert_guards_intact(sbuf, name)


@pytest.mark.parametrize("B,N", [(0, 9), (2, 1)])
def test_pair_stage_f16x3_empty_calls_write_nothing(tspn, device, B, N):
    """B = 0 and N = 1 have no pair: the call returns without a launch, the output and the split buffer keep every byte."""
    C, T, H = 64, 32, 12
    y = t(tspn.hashrng.uniform(68, "y", (B * N, 2 * C, T), -1, 1)).to(device)
    wh = t(tspn.hashrng.normal(68, "wh", (H, C), std=0.1)).to(device)
    buf, out = held((4, H, T), device)
    sbuf, split = wsc.guarded_ws(tspn.ops.heads_pairgrid_f16x3_split_bytes(C, H), device, "ones")
    tspn.ops.heads_pairgrid_f16x3(y, B, N, wh, None, T=T, split_buf=split, out=out)
    torch.cuda.synchronize(device)
    assert_untouched(buf, f"B={B} N={N}")
    wsc.assert_all_ones(split, f"B={B} N={N}")
    wsc.assert_guards_intact(sbuf, f"B={B} N={N}")


def _fused(tspn, device, w, feats, pairs, B, N, D, conv, canonical):
    d = lambda v: v.to(device).contiguous()   # noqa: E731
    packed = (tspn.ops.pack_conv3_wino63_f16x3 if conv == "f16x3" else tspn.ops.pack_conv3)(d(w["conv_w"]), split=D)
    hw = d(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]))
    hb = d(torch.cat([w["rel_b"], w["dur_b"]]))
    heads, logits = tspn.ops.forward_fused(d(feats), d(pairs), B, N, packed, d(w["conv_b"]), hw, hb, d(w["cls_w"]),
                                           d(w["cls_b"]), canonical_pairs=canonical)
    return heads.cpu(), logits.cpu()


@pytest.mark.parametrize("B,N,T,D", [(2, 6, 30, 128), (1, 9, 36, 64)])
def test_forward_fused_runs_the_f16x3_pair_stage_only_on_the_promoted_form(tspn, device, B, N, T, D):
    A = 4
    w = fused_weights(tspn, D, A)
    vids = [tspn.synth.make_video(90 + b, N, T, D) for b in range(B)]
    feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
    pairs = pair_table(B, N)
    # split-fp16 conv, canonical pairs: the new stage, against the dense float64 oracle at test_forward_fused_f16x3_against_
    # dense_oracle's bound; it ran (the forced fp32 chain gives other bits)
    heads, logits = _fused(tspn, device, w, feats, pairs, B, N, D, "f16x3", True)
    refs = [oracle.forward_dense(t(v["tracklet_feats"]).double(), t(v["tracklet_boxes"]).double(), oracle.pair_index(N),
                                 {k: x.double() for k, x in w.items()}) for v in vids]
    np.testing.assert_allclose(heads[:, :A].numpy(), torch.cat([r["relness"] for r in refs]).numpy(), rtol=0, atol=6e-5)
    np.testing.assert_allclose(heads[:, A:].numpy(), torch.cat([r["duration"] for r in refs]).numpy(), rtol=0, atol=6e-5)
    np.testing.assert_allclose(logits.numpy(), torch.cat([r["rel_logits"] for r in refs]).numpy(), rtol=0, atol=2e-5)
    # direct conv, canonical pairs: heads_pairgrid4_kernel as before -- its bytes are the fp32 chain of the new entry on
    # the same projections (tspn_conv3_tc_f32 with the bias on the subject half, as the fused pass forms them)
    direct, _ = _fused(tspn, device, w, feats, pairs, B, N, D, "direct", True)
    C = 2 * D
    y = tspn.ops.conv3_tc(feats.to(device), tspn.ops.pack_conv3(w["conv_w"].to(device), split=D),
                          torch.cat([w["conv_b"], torch.zeros(C)]).to(device)).cpu().numpy()
    hw = torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]).numpy()
    hb = torch.cat([w["rel_b"], w["dur_b"]]).numpy()
    assert np.array_equal(bits(direct.numpy()), bits(exact(tspn, device, y, hw, hb, B, N)))
    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        forced, _ = _fused(tspn, device, w, feats, pairs, B, N, D, "f16x3", True)
        direct1, _ = _fused(tspn, device, w, feats, pairs, B, N, D, "direct", True)
        listed1, _ = _fused(tspn, device, w, feats, pairs.flip(0).contiguous(), B, N, D, "f16x3", False)
    finally:
        tspn.ops.heads_pairgrid_f16x3_set_force_exact(prev)
    assert not torch.equal(forced, heads)
    np.testing.assert_allclose(forced.numpy(), heads.numpy(), rtol=0, atol=ATOL)
    # the switch reaches neither the direct form nor an arbitrary pair table: they do not run the new stage
    assert torch.equal(direct1, direct)
    listed, _ = _fused(tspn, device, w, feats, pairs.flip(0).contiguous(), B, N, D, "f16x3", False)
    assert torch.equal(listed1, listed)
    np.testing.assert_allclose(listed.flip(0).numpy(), heads.numpy(), rtol=0, atol=ATOL)


@pytest.mark.parametrize("B,N,T,D,A", [(2, 6, 31, 64, 4), (2, 6, 30, 64, 5), (2, 6, 30, 64, 3)])
def test_forward_fused_keeps_the_f16x3_pair_stage_off_on_odd_t_and_other_head_counts(tspn, device, B, N, T, D, A):
    """The other two branches of the fused pass's decision, behind the split-fp16 conv with canonical pairs: odd T (the
    stage stores frame pairs) and 3A != 12 (9 and 15 heads).  The force switch changes nothing -- the stage does not run
    -- and the dense float64 oracle is met at the bounds of the promoted form above."""
    w = fused_weights(tspn, D, A)
    vids = [tspn.synth.make_video(95 + b, N, T, D) for b in range(B)]
    feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
    pairs = pair_table(B, N)
    heads, logits = _fused(tspn, device, w, feats, pairs, B, N, D, "f16x3", True)
    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        heads1, logits1 = _fused(tspn, device, w, feats, pairs, B, N, D, "f16x3", True)
    finally:
        tspn.ops.heads_pairgrid_f16x3_set_force_exact(prev)
    assert heads.shape == (B * N * (N - 1), 3 * A, T)
    assert np.array_equal(bits(heads.numpy()), bits(heads1.numpy())) and np.array_equal(bits(logits.numpy()), bits(logits1.numpy()))
    refs = [oracle.forward_dense(t(v["tracklet_feats"]).double(), t(v["tracklet_boxes"]).double(), oracle.pair_index(N),
                                 {k: x.double() for k, x in w.items()}) for v in vids]
    np.testing.assert_allclose(heads[:, :A].numpy(), torch.cat([r["relness"] for r in refs]).numpy(), rtol=0, atol=6e-5)
    np.testing.assert_allclose(heads[:, A:].numpy(), torch.cat([r["duration"] for r in refs]).numpy(), rtol=0, atol=6e-5)
    np.testing.assert_allclose(logits.numpy(), torch.cat([r["rel_logits"] for r in refs]).numpy(), rtol=0, atol=2e-5)
