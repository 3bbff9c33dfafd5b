"""Non-finite inputs through the split-fp16 F(6,3) conv.

F(6,3) may smear a NaN / Inf over the frames of its sextets; the split form adds its own mechanisms (a non-finite column
or row maximum leaves the column unscaled, lo = Inf - Inf is NaN, B^T d of a finite value near FLT_MAX overflows).  What
must hold: nothing leaks out of the affected sextets (inputs) or the affected row (weights) -- every other output is bit
for bit what the clean launch gives --, every output that is non-finite in float64 is non-finite here (the kind may
differ), no finite output is a wrong number, the guard reads +Inf and names the NaN's sextet, and a promoted model falls
back to the direct kernel with one warning."""
import warnings

import numpy as np
import pytest
import torch

from test_gpu_nonfinite import (DPN_PRE, NAN_NEG_PAY, NAN_PAY, NAN_POS, check_decode, conv_err_word, conv_ref, plant_frames,
                                zero_conv_words)
from test_gpu_wino63_f16x3 import _model

pytestmark = pytest.mark.gpu

CONV_TOL = 1e-4
INF = np.float32(np.inf)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def affected_sextets(clean, planted, T):
    """[B, nq] bool: sextets with a changed input frame among their 8 (6 own + halo) frames."""
    nq = -(-T // 6)
    changed = (bits(clean) != bits(planted)).any(axis=2)                      # [B,T]
    out = np.zeros((clean.shape[0], nq), dtype=bool)
    for b, f in np.argwhere(changed):
        for q in range(nq):
            if 6 * q - 1 <= f <= 6 * q + 6:
                out[b, q] = True
    return out


def frames_of(sext, T):
    """[B, nq] sextet mask -> [B, T] frame mask."""
    return np.repeat(sext, 6, axis=1)[:, :T]


def run(tspn, device, x, w, b=None, relu=False):
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device))
    return tspn.ops.conv3_tc_wino63_f16x3(t(x).to(device), pk, None if b is None else t(b).to(device), relu=relu).cpu().numpy()


def check_confined(y_clean, y_bad, ref_bad, hit, what):
    """hit [B,T]: frames of affected sextets.  Outside: bit-equal to the clean launch.  Inside: non-finite wherever float64
    is, and a finite output within 6e-5 of a finite float64 value."""
    out = ~hit[:, None, :] & np.ones_like(y_clean, dtype=bool)
    assert np.array_equal(bits(y_clean)[out], bits(y_bad)[out]), f"{what}: leaked out of the affected sextets"
    assert np.isfinite(y_clean).all()
    nonfin = ~np.isfinite(ref_bad)
    assert not (nonfin & ~hit[:, None, :]).any()
    assert not np.isfinite(y_bad[nonfin]).any(), f"{what}: finite output where float64 is NaN / Inf"
    fin = np.isfinite(y_bad) & ~out
    assert np.isfinite(ref_bad[fin]).all()
    if fin.any():
        assert np.abs(y_bad[fin] - ref_bad[fin]).max() <= 6e-5, f"{what}: a finite wrong number"


@pytest.mark.parametrize("B,T", [(5, 40), (64, 24), (3, 7)])
@pytest.mark.parametrize("relu,with_bias", [(False, False), (True, True)])
def test_f16x3_nonfinite_confined_to_its_sextets(tspn, device, B, T, relu, with_bias):
    """plant_frames' positions (frame 0, T - 1, both sides of the sextet boundary 5 | 6: each lies in its neighbour's halo
    only) plus the last frame of the last tracklet = the last real column before the padding of the 256-sextet tile
    ((64, 24): exactly 256 sextets, no padding)."""
    Cin, M = 64, 256
    x = tspn.hashrng.uniform(501, "x", (B, T, Cin), -1, 1)
    w = tspn.hashrng.normal(501, "w", (M, Cin, 3), std=0.1)
    w[0, 5, :] = 0.0
    b = tspn.hashrng.normal(501, "b", (M,), std=0.1) if with_bias else None
    bad = plant_frames(x.copy(), T, "tc")
    bad[B - 1, T - 1, 7] = NAN_PAY
    hit = frames_of(affected_sextets(x, bad, T), T)
    assert hit.any() and not hit.all()
    y_clean, y_bad = run(tspn, device, x, w, b, relu), run(tspn, device, bad, w, b, relu)
    ref = conv_ref(bad.transpose(0, 2, 1), w, b, relu)
    assert np.isnan(ref).any() and np.isinf(ref).any()
    check_confined(y_clean, y_bad, ref, hit, f"B={B} T={T}")
    np.testing.assert_allclose(y_clean, conv_ref(x.transpose(0, 2, 1), w, b, relu), rtol=0, atol=6e-5)


@pytest.mark.parametrize("val", [NAN_POS, NAN_NEG_PAY, INF, -INF])
def test_f16x3_weight_nonfinite_stays_in_its_row(tspn, device, val):
    """One NaN / Inf tap (rows 3 and 255, different taps): every other output row is bit for bit the clean launch's; the row
    itself is non-finite wherever float64 is (everywhere: the tap meets every frame, or the zero padding)."""
    B, T, Cin, M = 4, 31, 64, 256
    x = tspn.hashrng.uniform(502, "x", (B, T, Cin), -1, 1)
    w = tspn.hashrng.normal(502, "w", (M, Cin, 3), std=0.1)
    y_clean = run(tspn, device, x, w)
    for row, c, k in ((3, 9, 0), (M - 1, 63, 2)):
        wb = w.copy()
        wb[row, c, k] = val
        y_bad = run(tspn, device, x, wb)
        ref = conv_ref(x.transpose(0, 2, 1), wb, None, False)
        others = np.arange(M) != row
        assert np.array_equal(bits(y_clean[:, others]), bits(y_bad[:, others]))
        assert not np.isfinite(ref[:, row]).all()
        nonfin = ~np.isfinite(ref)
        assert not np.isfinite(y_bad[nonfin]).any()
        fin = np.isfinite(y_bad[:, row])
        assert (np.abs(y_bad[:, row][fin] - ref[:, row][fin]) <= 6e-5).all() and np.isfinite(ref[:, row][fin]).all()


def test_f16x3_inf_times_zero_and_finite_overflow(tspn, device):
    """An Inf feature whose weights are all zero (float64: NaN on the three frames it meets, finite elsewhere), and finite
    features at 3e38 on frames 6q + 1 / 6q + 2, where B^T d overflows fp32 (float64: finite everywhere, the weights are
    zero).  Every output of the affected sextets is within tolerance or non-finite; the others are bit-equal."""
    B, T, Cin, M = 4, 40, 64, 256
    x = tspn.hashrng.uniform(503, "x", (B, T, Cin), -1, 1)
    w = tspn.hashrng.normal(503, "w", (M, Cin, 3), std=0.1)
    w[:, 11, :] = 0.0
    y_clean = run(tspn, device, x, w)
    for what, plants in (("Inf x 0", [(0, 9, INF), (2, T - 1, -INF)]),
                         ("overflow in B^T d", [(1, 6 * 2 + 2, np.float32(3e38)), (3, 6 * 5 + 1, np.float32(-3e38))])):
        bad = x.copy()
        for (b, f, v) in plants:
            bad[b, f, 11] = v
        hit = frames_of(affected_sextets(x, bad, T), T)
        y_bad = run(tspn, device, bad, w)
        ref = conv_ref(bad.transpose(0, 2, 1), w, None, False)
        assert np.isnan(ref).any() == (what == "Inf x 0")
        check_confined(y_clean, y_bad, ref, hit, what)
        assert not np.isfinite(y_bad).all(), f"{what}: expected to reach the outputs as NaN / Inf"


def test_f16x3_guard_reads_inf_and_names_the_nan_sextet(tspn, device):
    """test_guard_reads_inf_on_nonfinite_launches_and_names_the_nan_sextet for conv_algo = F16X3: the split input transform
    computes the hot-sextet key in its own kernel body."""
    B, N, T, D = 2, 3, 40, 64
    sd = tspn.synth.make_weights(50, c=2 * D, bias_std=0.05)
    d = lambda a: t(a).to(device).contiguous()   # noqa: E731
    conv_w, conv_b = d(sd[DPN_PRE + "conv.weight"]), d(sd[DPN_PRE + "conv.bias"])
    hw = d(np.concatenate([sd[DPN_PRE + "relness_pred.weight"][:, :, 0], sd[DPN_PRE + "duration_pred.weight"][:, :, 0]]))
    hb = d(np.concatenate([sd[DPN_PRE + "relness_pred.bias"], sd[DPN_PRE + "duration_pred.bias"]]))
    cw, cb = d(sd["classifier.rel_predictor.weight"]), d(sd["classifier.rel_predictor.bias"])
    pairs = torch.cat([tspn.ops.pair_index(N, device, base=b * N) for b in range(B)])
    packed = tspn.ops.pack_conv3_wino63_f16x3(conv_w, split=D)
    need = tspn.ops.fused_workspace_bytes(B, N, T, D, 4, cw.shape[0], pairs.shape[0], conv_algo=tspn._abi.CONV_WINOGRAD63_F16X3)
    nq = (T + 5) // 6

    def launch(feats):
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        zero_conv_words(tspn, device)
        tspn.ops.forward_fused(d(feats), pairs, B, N, packed, conv_b, hw, hb, cw, cb, workspace=ws, canonical_pairs=True,
                               conv_weight=conv_w, conv_check=16)
        torch.cuda.synchronize(device)
        scratch = ws[need - tspn._abi.CONV_CHECK_SCRATCH_BYTES:].view(torch.int64)
        slots = scratch[tspn._abi.CONV_CHECK_HOT_OFFSET // 8::32][:64].cpu().numpy().astype(np.uint64)
        return conv_err_word(tspn, device), int(slots.max())

    try:
        # an Inf in another sextet (and a large finite outlier): the NaN still wins the key
        for trk, frame, val in ((4, 27, NAN_NEG_PAY), (2, 17, NAN_POS), (5, T - 1, NAN_PAY), (1, 12, INF)):
            feats = tspn.hashrng.uniform(7, "x", (B * N, T, D), -1, 1)
            feats[0, 3, 2] = 1e6
            if np.isnan(val):
                feats[3, 8, 20] = INF
            feats[trk, frame, 13] = val
            (err, checks), key = launch(feats)
            assert err == np.inf and checks > 0, (val, err, checks)
            assert key & 0xFFFFFFFF == trk * nq + frame // 6, (trk, frame, key & 0xFFFFFFFF)
            top = np.array([key >> 32], dtype=np.uint32).view(np.float32)[0]
            assert np.isnan(top) if np.isnan(val) else np.isposinf(top)
        (err, checks), _ = launch(tspn.hashrng.uniform(7, "x", (B * N, T, D), -1, 1))
        assert np.isfinite(err) and err <= CONV_TOL and checks > 0
    finally:
        zero_conv_words(tspn, device)


@pytest.mark.parametrize("where", ["frame0", "last", "boundary5", "boundary6", "inf_mid", "last_column"])
def test_promoted_model_falls_back_on_each_planted_position(tspn, device, where):
    """A model that runs the split form meets one planted value: the call after it warns once and runs the direct kernel,
    bit for bit a CONV_ALGO: direct model on the same (planted) features; the decode of its logits is the oracle's."""
    D, N, T = 128, 5, 33
    feats = tspn.hashrng.uniform(86, "x", (N, T, D))
    vid = tspn.synth.make_video(86, N, T, D)
    pl = lambda f: tspn.PairList.from_tracklets(t(f).to(device), t(vid["tracklet_boxes"]).to(device),   # noqa: E731
                                                t(vid["track_cls_logits"]).to(device))
    bad = feats.copy()
    trk, frame, val = {"frame0": (0, 0, NAN_POS), "last": (1, T - 1, INF), "boundary5": (2, 5, NAN_NEG_PAY),
                       "boundary6": (2, 6, -INF), "inf_mid": (1, T // 2, INF), "last_column": (N - 1, T - 1, NAN_PAY)}[where]
    bad[trk, frame, 3] = val
    try:
        model = _model(tspn, D, 86, 0.02, **{"RELPN.DPN.CONV_F16X3_AFTER": 1}).to(device)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for _ in range(3):
                model([pl(feats)], None)
                torch.cuda.synchronize(device)
            assert model.conv_promoted and not model.conv_fallback and not rec
            model([pl(bad)], None)                       # the split form on the planted features
            torch.cuda.synchronize(device)
            assert not rec
            plist = pl(bad)
            _, dp, lg = model([plist], None)             # reads +Inf: direct from here on
            torch.cuda.synchronize(device)
        msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
        assert len(msgs) == 1 and "direct kernel" in msgs[0] and model.conv_fallback
        direct = _model(tspn, D, 86, 0.02, **{"RELPN.DPN.CONV_ALGO": "direct"}).to(device)
        _, dpd, lgd = direct([pl(bad)], None)
        torch.cuda.synchronize(device)
        ib = lambda v: v.contiguous().view(torch.int32)   # noqa: E731  (bit-equal, NaN payloads included)
        assert torch.equal(ib(dp[0].heads), ib(dpd[0].heads)) and torch.equal(ib(lg[0]), ib(lgd[0]))
        assert not torch.isfinite(dp[0].heads).all()
        check_decode(model, plist, lg, vid["track_cls_logits"], N, lg[0].shape[1])
    finally:
        zero_conv_words(tspn, device)
