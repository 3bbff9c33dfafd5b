"""Winograd F(6,3) temporal conv (tspn_wino63.hip) through the C ABI: against the float64 conv for ragged shapes
(sextets masked at tracklet ends, tiles that straddle tracklets, 1 .. many super-stages, partial weight / sextet
tiles), its packed weights against the closed-form U = G g, its fp32 error next to the direct kernel at the
contraction depth of the headline config -- on the benchmark's distribution and on heavy-tailed / trained-scale
magnitudes, with a relative bound -- and the fused path / BaseModel on it against the dense oracle."""
import numpy as np
import pytest
import torch

import cases
import oracle

pytestmark = pytest.mark.gpu

DPN_PRE = "relpn.duration_proposal_network.dpn_head."


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def conv_ref(x_tc, w, b, relu):
    """x [B,T,Cin], w [M,Cin,3] -> [B,M,T] float64."""
    y = torch.nn.functional.conv1d(t(x_tc).double().transpose(1, 2), t(w).double(),
                                   None if b is None else t(b).double(), padding=1)
    return (torch.relu(y) if relu else y).numpy()


@pytest.mark.parametrize("B,Cin,T,M", [(1, 32, 1, 32), (2, 32, 5, 32), (3, 64, 30, 128), (5, 96, 33, 160),
                                       (7, 64, 150, 64), (2, 160, 257, 288), (40, 32, 30, 96), (3, 32, 7, 32),
                                       (33, 128, 13, 128), (1, 32, 6, 32), (9, 256, 150, 256), (70, 32, 6, 32),
                                       # tile map: BM = 128 rows, SWG = 64 sextets, GM = 4: M = 5 * 128 gives two groups,
                                       # the second a single panel; 27 * ceil(31 / 6) = 162 sextets = 3 column tiles;
                                       # grid 15 (> 8, 15 % 8 = 7)
                                       (27, 32, 31, 640)])
@pytest.mark.parametrize("relu", [False, True])
def test_conv3_winograd63_vs_fp64(tspn, device, B, Cin, T, M, relu):
    x = tspn.hashrng.uniform(61, "x", (B, T, Cin), -1, 1)
    w = tspn.hashrng.normal(61, "w", (M, Cin, 3), std=0.1)
    b = tspn.hashrng.normal(61, "b", (M,), std=0.1)
    fr = tspn.ops.pack_conv3_wino63(t(w).to(device))
    assert tuple(fr.shape) == (M // 32, Cin // 8, 8, 64, 4) and tspn.ops.wino63_frag_dims(fr) == (Cin, M)
    # frag[mb][c][j][32 kh + li][e] = U_j[8 c + 4 kh + e][32 mb + li], U = G g in double, rounded once
    g = w.astype(np.float64).transpose(2, 1, 0)   # [3][Cin][M]
    u = np.stack([g[0], -2 / 9 * (g[0] + g[1] + g[2]), -2 / 9 * (g[0] - g[1] + g[2]),
                  g[0] / 90 + g[1] / 45 + 2 * g[2] / 45, g[0] / 90 - g[1] / 45 + 2 * g[2] / 45,
                  (32 * g[0] + 16 * g[1] + 8 * g[2]) / 45, (32 * g[0] - 16 * g[1] + 8 * g[2]) / 45, g[2]]).astype(np.float32)
    want = u.reshape(8, Cin // 8, 2, 4, M // 32, 32).transpose(4, 1, 0, 2, 5, 3)
    np.testing.assert_array_equal(fr.cpu().numpy().reshape(M // 32, Cin // 8, 8, 2, 32, 4), want)
    for bias in (b, None):
        y = tspn.ops.conv3_tc_wino63(t(x).to(device), fr, None if bias is None else t(bias).to(device), relu=relu)
        assert y.shape == (B, M, T)
        np.testing.assert_allclose(y.cpu().numpy(), conv_ref(x, w, bias, relu), rtol=0, atol=6e-5)
    y2 = tspn.ops.conv3_tc_wino63(t(x).to(device), fr, t(b).to(device), relu=relu)
    assert torch.equal(y, y2) if bias is not None else True     # deterministic


def test_conv3_winograd63_split_packing_and_errors(tspn, device):
    """split = D packs the subject / object halves of the pair encoder as 2M rows over D channels."""
    M, D = 32, 32
    w = tspn.hashrng.normal(62, "w", (M, 2 * D, 3), std=0.1)
    fr = tspn.ops.pack_conv3_wino63(t(w).to(device), split=D)
    stacked = np.concatenate([w[:, :D], w[:, D:]], axis=0)               # [2M, D, 3]
    fr2 = tspn.ops.pack_conv3_wino63(t(stacked).to(device))
    assert torch.equal(fr, fr2) and tuple(fr.shape) == (2, 4, 8, 64, 4)
    with pytest.raises(ValueError):
        tspn.ops.pack_conv3_wino63(torch.zeros((36, 32, 3), device=device))        # M % 32
    with pytest.raises(tspn._abi.TspnError) as e:                                   # Cin % 32 != 0: refused
        tspn.ops.conv3_tc_wino63(torch.zeros((2, 9, 24), device=device),
                                 tspn.ops.pack_conv3_wino63(torch.zeros((32, 24, 3), device=device)))
    assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED
    y = tspn.ops.conv3_tc_wino63(torch.zeros((0, 9, 32), device=device), fr2)       # empty batch
    assert y.shape == (0, 64, 9)
    assert tspn._abi.lib().tspn_conv3_tc_wino63_workspace_bytes(16 * 32, 150, 2048) == 2048 // 4 * 8 * 12800 * 16


def heavy_tailed(tspn, seed, shape, scale=4.0, outlier=50.0, frac=1e-3, zeros=0.4):
    """Post-ReLU-like features: |N(0,1)| * scale, a fraction `frac` of 50x outliers, 40 % exact zeros."""
    x = np.abs(tspn.hashrng.normal(seed, "x", shape, std=1.0)) * scale
    x = np.where(tspn.hashrng.uniform(seed, "o", shape) < frac, x * outlier, x)
    return np.where(tspn.hashrng.uniform(seed, "z", shape) < zeros, 0.0, x).astype(np.float32)


def conv_errors(tspn, device, x, w):
    """max over the outputs of |err| / (eps * sum_k |x_k||w_k|) and of |err| / max|y| against float64, for the direct
    kernel and for F(6,3)."""
    ref = conv_ref(x, w, None, False)
    mag = conv_ref(np.abs(x), np.abs(w), None, False)
    xd, wd = t(x).to(device), t(w).to(device)
    out = {}
    for name, y in (("direct", tspn.ops.conv3_tc(xd, tspn.ops.pack_conv3(wd))),
                    ("F(6,3)", tspn.ops.conv3_tc_wino63(xd, tspn.ops.pack_conv3_wino63(wd)))):
        e = np.abs(y.cpu().numpy() - ref)
        out[name] = (float((e / (2.0 ** -24 * mag + 1e-300)).max()), float(e.max() / np.abs(ref).max()), float(e.max()))
    return out, float(np.abs(ref).max())


def test_conv3_winograd63_error_at_headline_depth(tspn, device):
    """fp32 error against float64 at K = 3 x 2048 channels on the benchmark's distribution (inputs in [0,1), weights
    N(0, 0.01^2)): the accumulation over the channels dominates, F(6,3) stays within 2x of the direct kernel and an
    order of magnitude inside the path's 1e-4 bound."""
    B, T, Cin, M = 3, 150, 2048, 128
    err, ymax = conv_errors(tspn, device, tspn.hashrng.uniform(48, "x", (B, T, Cin)),
                            tspn.hashrng.normal(48, "w", (M, Cin, 3), std=0.01))
    print("conv3 error vs float64 (|y| max %.3f): (e / eps sum|x||w|, e / max|y|, e)" % ymax, err)
    assert err["F(6,3)"][2] <= 2.0 * err["direct"][2] and err["F(6,3)"][2] <= 3e-5


@pytest.mark.parametrize("case", ["independent_heavy_tail", "outlier_weight_rows", "temporally_smooth"])
def test_conv3_winograd63_relative_error_on_realistic_magnitudes(tspn, device, case):
    """full-depth (K = 3 x 2048) error on post-ReLU-like heavy-tailed features (|N(0,1)| * 4, 0.1 %
    of 50x outliers, 40 % zeros, |x| up to ~500) and weights of trained scale (std 1/sqrt(3 D); or std 0.05 with 2 %
    of the rows scaled 20x).  The bound is RELATIVE -- no algorithm, the direct form included, holds an absolute
    1e-4 once |y| reaches 30 (fp32 has 6e-8 relative precision):
        |err| <= 64 eps sum_k |x_k||w_k|  and  |err| <= 2e-5 max|y|   for F(6,3)   (measured: 51, 1.3e-5)
        |err| <= 16 eps sum_k |x_k||w_k|                               for direct   (measured: 12)
    On temporally independent features F(6,3) is up to ~5x the direct kernel's error (the transforms' entries up to
    32 / 5.25 amplify); on temporally smooth features -- what consecutive frames of a tracklet are -- it is NOT worse
    than the direct kernel.  RELPN.DPN.CONV_ALGO = "direct" buys the direct bound at 2.25x the MFMA work."""
    B, T, Cin, M = 3, 150, 2048, 128
    if case == "independent_heavy_tail":
        x = heavy_tailed(tspn, 71, (B, T, Cin))
        w = tspn.hashrng.normal(71, "w", (M, Cin, 3), std=1.0 / np.sqrt(3 * Cin))
    elif case == "outlier_weight_rows":
        x = heavy_tailed(tspn, 72, (B, T, Cin))
        w = (tspn.hashrng.normal(72, "w", (M, Cin, 3), std=0.05)
             * np.where(tspn.hashrng.uniform(72, "r", (M, 1, 1)) < 0.02, 20.0, 1.0)).astype(np.float32)
    else:
        x = (heavy_tailed(tspn, 73, (B, 1, Cin)) + 0.05 * tspn.hashrng.normal(73, "n", (B, T, Cin), std=1.0)).astype(np.float32)
        w = tspn.hashrng.normal(73, "w", (M, Cin, 3), std=1.0 / np.sqrt(3 * Cin))
    err, ymax = conv_errors(tspn, device, x, w)
    print(f"{case}: max|y| {ymax:.3g}, max|x| {np.abs(x).max():.3g}; (e / eps sum|x||w|, e / max|y|, e):", err)
    assert err["direct"][0] <= 16.0
    assert err["F(6,3)"][0] <= 64.0 and err["F(6,3)"][1] <= 2e-5
    if case == "temporally_smooth":
        assert err["F(6,3)"][2] <= 1.5 * err["direct"][2]


@pytest.mark.parametrize("B,N,T,D", [(2, 5, 30, 32), (1, 9, 33, 32), (3, 4, 150, 64)])
def test_fused_winograd63_vs_dense_oracle(tspn, device, B, N, T, D):
    """tspn_forward_fused_f32 with TSPN_CONV_WINOGRAD63 against the dense oracle (1e-5) and against TSPN_CONV_DIRECT."""
    sd = tspn.synth.make_weights(50, c=2 * D, bias_std=0.05)
    w = {"conv_w": t(sd[DPN_PRE + "conv.weight"]), "conv_b": t(sd[DPN_PRE + "conv.bias"]),
         "dur_w": t(sd[DPN_PRE + "duration_pred.weight"]), "dur_b": t(sd[DPN_PRE + "duration_pred.bias"]),
         "rel_w": t(sd[DPN_PRE + "relness_pred.weight"]), "rel_b": t(sd[DPN_PRE + "relness_pred.bias"]),
         "cls_w": t(sd["classifier.rel_predictor.weight"]), "cls_b": t(sd["classifier.rel_predictor.bias"])}
    vids = [tspn.synth.make_video(60 + b, N, T, D) for b in range(B)]
    feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
    pairs = torch.cat([oracle.pair_index(N) + b * N for b in range(B)])
    d = lambda v: v.to(device).contiguous()   # noqa: E731
    hw = d(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]))
    hb = d(torch.cat([w["rel_b"], w["dur_b"]]))
    outs = []
    for packed in (tspn.ops.pack_conv3_wino63(d(w["conv_w"]), split=D),
                   tspn.ops.pack_conv3(d(w["conv_w"]), split=D)):
        outs.append(tspn.ops.forward_fused(d(feats), d(pairs), B, N, packed, d(w["conv_b"]), hw, hb,
                                           d(w["cls_w"]), d(w["cls_b"]), canonical_pairs=True))
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), outs[1][0].cpu().numpy(), rtol=0, atol=1e-5)
    assert torch.equal(outs[0][1], outs[1][1])           # the logits do not depend on the conv algorithm
    for b in range(B):
        ref = oracle.forward_dense(t(vids[b]["tracklet_feats"]), t(vids[b]["tracklet_boxes"]), oracle.pair_index(N), w)
        sl = slice(b * N * (N - 1), (b + 1) * N * (N - 1))
        np.testing.assert_allclose(outs[0][0][sl, :4].cpu().numpy(), ref["relness"].numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(outs[0][0][sl, 4:].cpu().numpy(), ref["duration"].numpy(), rtol=0, atol=1e-5)


def test_basemodel_conv_algo_config(tspn, device):
    """RELPN.DPN.CONV_ALGO = "auto" selects the F(6,3) weights when D % 32 == 0 and the direct taps otherwise;
    "direct" always selects the direct taps."""
    for D, algo, want in ((32, "auto", (2 * 64 // 32, 32 // 8, 8, 64, 4)), (16, "auto", (3, 16, 64)),
                          (32, "direct", (3, 32, 128))):
        cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                    "PREDICT.FEATURE_DIM": 2 * D, "RELPN.DPN.CONV_ALGO": algo})
        model = tspn.BaseModel(cfg)
        sd = tspn.synth.make_weights(3, c=2 * D, bias_std=0.05)
        own = model.state_dict()
        model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
        model.eval()
        v = tspn.synth.make_video(77, 6, 30, D)
        pl = tspn.PairList.from_tracklets(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), t(v["track_cls_logits"]))
        _, dp, logits = model([pl], None)
        caches = model.relpn.duration_proposal_network._cache._store
        packed = [val[1][0] for key, val in caches.items() if key.startswith("conv_split")]
        assert len(packed) == 1 and tuple(packed[0].shape) == want
        w = {"conv_w": t(sd[DPN_PRE + "conv.weight"]), "conv_b": t(sd[DPN_PRE + "conv.bias"]),
             "dur_w": t(sd[DPN_PRE + "duration_pred.weight"]), "dur_b": t(sd[DPN_PRE + "duration_pred.bias"]),
             "rel_w": t(sd[DPN_PRE + "relness_pred.weight"]), "rel_b": t(sd[DPN_PRE + "relness_pred.bias"]),
             "cls_w": t(sd["classifier.rel_predictor.weight"]), "cls_b": t(sd["classifier.rel_predictor.bias"])}
        ref = oracle.forward_dense(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), oracle.pair_index(6), w)
        np.testing.assert_allclose(dp[0].duration.numpy(), ref["duration"].numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(logits[0].numpy(), ref["rel_logits"].numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("B,Cin,T,M", [(5, 96, 33, 160), (9, 256, 150, 256), (70, 32, 6, 32)])
def test_conv3_winograd63_buffer_and_pointer_pieces_are_bit_identical(tspn, device, B, Cin, T, M):
    """The V pieces of conv3_wino63_kernel go out as buffer loads (one descriptor, 32-bit offsets) where the workspace is
    below 4 GB and as global_load_lds with 64-bit pointers otherwise (ops.wino63_set_piece_form(1) forces that form): the same bytes
    land in LDS, so the results are the same bits."""
    x = t(tspn.hashrng.uniform(62, "x", (B, T, Cin), -1, 1)).to(device)
    w = t(tspn.hashrng.normal(62, "w", (M, Cin, 3), std=0.1)).to(device)
    b = t(tspn.hashrng.normal(62, "b", (M,), std=0.1)).to(device)
    fr = tspn.ops.pack_conv3_wino63(w)
    assert tspn.ops.wino63_set_piece_form(0) == 0
    y_buf = tspn.ops.conv3_tc_wino63(x, fr, bias=b, relu=True)
    try:
        tspn.ops.wino63_set_piece_form(1)
        y_ptr = tspn.ops.conv3_tc_wino63(x, fr, bias=b, relu=True)
    finally:
        assert tspn.ops.wino63_set_piece_form(0) == 1
    assert torch.equal(y_buf, y_ptr)
