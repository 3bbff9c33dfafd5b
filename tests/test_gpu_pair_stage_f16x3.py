"""The fp32 path's pair stage on split-fp16 MFMAs (csrc/pairf16/, tspn_heads_pairgrid_f16x3): against float64 at the
tile edges, the per-tile fp32 chain on out-of-range and non-finite values, and the fused pass that runs it.

Tile = 8 subjects x 8 objects x 32 frames.  A tile takes the fp32 chain when a value it stages for a written output (a
real tracklet's row, a frame < T) is not <= 2^14 in magnitude, and every tile does when a head's weights are non-finite
or all zero.  Rows of y are padded to a multiple of 4 frames; the pad frames hold NaN here and must never matter."""
import numpy as np
import pytest
import torch

import oracle
from sentinel_buffers import assert_written_inside_only, held
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


def launch(tspn, device, y, wh, bh, B, N):
    """The entry on y padded to ldt = ceil4(T) frames per row (NaN in the pad), output held between sentinel guards."""
    NT, C2, T = y.shape
    ldt = (T + 3) // 4 * 4
    yp = torch.full((NT, C2, ldt), float("nan"))
    yp[:, :, :T] = t(y)
    buf, out = held((B * N * (N - 1), wh.shape[0], T), device)
    tspn.ops.heads_pairgrid_f16x3(yp.to(device), B, N, t(wh).to(device), t(bh).to(device), T=T, out=out)
    assert_written_inside_only(buf, out, "heads_pairgrid_f16x3")
    return out.cpu().numpy()


def exact(tspn, device, *args):
    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        return launch(tspn, device, *args)
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


def affected_rows():
    """[P, T] bool: outputs of a tile that stages a planted value."""
    pairs = pair_table(B2, N2).numpy()
    vid, s, o = pairs[:, 0] // N2, pairs[:, 0] % N2, pairs[:, 1] % N2
    hit = np.zeros((pairs.shape[0], T2), dtype=bool)
    for (b, trk, half, _, f, _) in PLANTS:
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
