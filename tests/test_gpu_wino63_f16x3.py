"""Split-fp16 Winograd F(6,3) temporal conv (TSPN_CONV_WINOGRAD63_F16X3, tspn_wino63.hip) through the C ABI: against
the float64 conv at ragged shapes and the gate's minimum tiles, at the headline contraction depth on the four
distributions of tests/test_gpu_wino63.py (held to the fp32 F(6,3) bounds), on features spanning 1e-30 .. 1e6 in one
launch, at the full cfg2 step against the fp32 form, bit-identical under concurrent traffic, and the promotion /
fallback sequence of BaseModel."""
import warnings

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

DPN_PRE = "relpn.duration_proposal_network.dpn_head."


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def conv_ref(x_tc, w, b=None, relu=False):
    """x [B,T,Cin], w [M,Cin,3] -> [B,M,T] float64."""
    y = torch.nn.functional.conv1d(t(x_tc).double().transpose(1, 2), t(w).double(),
                                   None if b is None else t(b).double(), padding=1)
    return (torch.relu(y) if relu else y).numpy()


def heavy_tailed(tspn, seed, shape, scale=4.0, outlier=50.0, frac=1e-3, zeros=0.4):
    x = np.abs(tspn.hashrng.normal(seed, "x", shape, std=1.0)) * scale
    x = np.where(tspn.hashrng.uniform(seed, "o", shape) < frac, x * outlier, x)
    return np.where(tspn.hashrng.uniform(seed, "z", shape) < zeros, 0.0, x).astype(np.float32)


@pytest.mark.parametrize("B,Cin,T,M", [(1, 32, 1, 256), (2, 32, 33, 256), (3, 64, 30, 512), (9, 128, 150, 256),
                                       (40, 32, 7, 256), (11, 96, 257, 768)])
@pytest.mark.parametrize("relu", [False, True])
def test_conv3_wino63_f16x3_vs_fp64(tspn, device, B, Cin, T, M, relu):
    x = tspn.hashrng.uniform(81, "x", (B, T, Cin), -1, 1)
    w = tspn.hashrng.normal(81, "w", (M, Cin, 3), std=0.1)
    b = tspn.hashrng.normal(81, "b", (M,), std=0.1)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device))
    assert pk.dtype == torch.int16 and tspn.ops.wino63_f16x3_dims(pk) == (Cin, M)
    for bias in (b, None):
        y = tspn.ops.conv3_tc_wino63_f16x3(t(x).to(device), pk, None if bias is None else t(bias).to(device), relu=relu)
        assert y.shape == (B, M, T)
        np.testing.assert_allclose(y.cpu().numpy(), conv_ref(x, w, bias, relu), rtol=0, atol=6e-5)
    y2 = tspn.ops.conv3_tc_wino63_f16x3(t(x).to(device), pk, None, relu=relu)
    assert torch.equal(y, y2)


def test_conv3_wino63_f16x3_packing_and_errors(tspn, device):
    M, D = 128, 32
    w = tspn.hashrng.normal(82, "w", (M, 2 * D, 3), std=0.1)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device), split=D)
    stacked = np.concatenate([w[:, :D], w[:, D:]], axis=0)
    assert torch.equal(pk, tspn.ops.pack_conv3_wino63_f16x3(t(stacked).to(device)))
    assert tuple(pk.shape) == (8, 2 * D // 8 + 1, 2 * M, 8)
    # hi + lo, unscaled, reproduces U = G g to ~2^-22 of the row maximum
    g = stacked.astype(np.float64).transpose(2, 1, 0)   # [3][Cin][M]
    u = np.stack([g[0], -2 / 9 * (g[0] + g[1] + g[2]), -2 / 9 * (g[0] - g[1] + g[2]),
                  g[0] / 90 + g[1] / 45 + 2 * g[2] / 45, g[0] / 90 - g[1] / 45 + 2 * g[2] / 45,
                  (32 * g[0] + 16 * g[1] + 8 * g[2]) / 45, (32 * g[0] - 16 * g[1] + 8 * g[2]) / 45, g[2]])  # [8][Cin][M]
    raw = pk.cpu().numpy()
    ncg = D // 8
    hi = raw[:, :ncg].view(np.float16).astype(np.float64)            # [8][ncg][M][8]
    lo = raw[:, ncg:2 * ncg].view(np.float16).astype(np.float64)
    e = raw[:, 2 * ncg, :, :2].copy().view(np.int32)[..., 0]          # [8][M]
    rec = (hi + lo).transpose(0, 1, 3, 2).reshape(8, D, 2 * M) * np.ldexp(1.0, -e)[:, None, :]
    rowmax = np.abs(u).max(axis=1, keepdims=True)
    assert (np.abs(rec - u) <= 2.0 ** -21 * rowmax).all()
    assert ((np.abs(u).max(axis=1) * np.ldexp(1.0, e) >= 2 ** 14) & (np.abs(u).max(axis=1) * np.ldexp(1.0, e) < 2 ** 15)).all()
    with pytest.raises(ValueError):
        tspn.ops.pack_conv3_wino63_f16x3(torch.zeros((128, 32, 3), device=device))     # M % 256
    y = tspn.ops.conv3_tc_wino63_f16x3(torch.zeros((0, 9, 32), device=device), pk)     # empty batch
    assert y.shape == (0, 2 * M, 9)


def _errors(tspn, device, x, w):
    ref = conv_ref(x, w)
    mag = conv_ref(np.abs(x), np.abs(w))
    xd, wd = t(x).to(device), t(w).to(device)
    out = {}
    for name, y in (("F(6,3)", tspn.ops.conv3_tc_wino63(xd, tspn.ops.pack_conv3_wino63(wd))),
                    ("f16x3", tspn.ops.conv3_tc_wino63_f16x3(xd, tspn.ops.pack_conv3_wino63_f16x3(wd)))):
        e = np.abs(y.cpu().numpy() - ref)
        out[name] = (float((e / (2.0 ** -24 * mag + 1e-300)).max()), float(e.max() / np.abs(ref).max()), float(e.max()))
    return out


@pytest.mark.parametrize("case", ["bench", "independent_heavy_tail", "outlier_weight_rows", "temporally_smooth"])
def test_conv3_wino63_f16x3_error_at_headline_depth(tspn, device, case):
    """K = 3 x 2048: the split form within the fp32 F(6,3) bounds (64 eps sum|x||w|, 2e-5 max|y|)."""
    B, T, Cin, M = 3, 150, 2048, 256
    if case == "bench":
        x = tspn.hashrng.uniform(48, "x", (B, T, Cin))
        w = tspn.hashrng.normal(48, "w", (M, Cin, 3), std=0.01)
    elif case == "independent_heavy_tail":
        x = heavy_tailed(tspn, 71, (B, T, Cin))
        w = tspn.hashrng.normal(71, "w", (M, Cin, 3), std=1.0 / np.sqrt(3 * Cin))
    elif case == "outlier_weight_rows":
        x = heavy_tailed(tspn, 72, (B, T, Cin))
        w = (tspn.hashrng.normal(72, "w", (M, Cin, 3), std=0.05)
             * np.where(tspn.hashrng.uniform(72, "r", (M, 1, 1)) < 0.02, 20.0, 1.0)).astype(np.float32)
    else:
        x = (heavy_tailed(tspn, 73, (B, 1, Cin)) + 0.05 * tspn.hashrng.normal(73, "n", (B, T, Cin), std=1.0)).astype(np.float32)
        w = tspn.hashrng.normal(73, "w", (M, Cin, 3), std=1.0 / np.sqrt(3 * Cin))
    err = _errors(tspn, device, x, w)
    print(f"{case}: (e / eps sum|x||w|, e / max|y|, e):", err)
    assert err["f16x3"][0] <= 64.0 and err["f16x3"][1] <= 2e-5
    if case == "bench":
        assert err["f16x3"][2] <= 3e-5


def test_conv3_wino63_f16x3_feature_scales(tspn, device):
    """Tracklets whose features sit at 1e-30 .. 1e6 in ONE launch: the per-column scales keep every one of them at the
    relative accuracy of the others."""
    scales = [1e-30, 1e-20, 1e-8, 1e-3, 1.0, 1e3, 1e6]
    B, T, Cin, M = len(scales), 36, 64, 256
    x = (tspn.hashrng.uniform(83, "x", (B, T, Cin), -1, 1) * np.array(scales)[:, None, None]).astype(np.float32)
    w = tspn.hashrng.normal(83, "w", (M, Cin, 3), std=0.1)
    y = tspn.ops.conv3_tc_wino63_f16x3(t(x).to(device), tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device))).cpu().numpy()
    ref = conv_ref(x, w)
    mag = conv_ref(np.abs(x), np.abs(w))
    for bi, s in enumerate(scales):
        rel = np.abs(y[bi] - ref[bi]) / (2.0 ** -24 * mag[bi])
        assert rel.max() <= 64.0, (s, rel.max())


def test_conv3_wino63_f16x3_cfg2_step_against_fp32(tspn, device):
    """The full cfg2 step shape (16 videos x 32 tracklets, T = 150, D = 2048 -> 2C = 8192 rows, split halves): every
    output of the split form within 1e-4 of the fp32 F(6,3) form, and float64 on sampled rows of one video."""
    D, NT, T = 2048, 16 * 32, 150
    x = tspn.hashrng.uniform(84, "x", (NT, T, D))
    w = tspn.hashrng.normal(84, "w", (2 * D, 2 * D, 3), std=0.01)
    b = tspn.hashrng.normal(84, "b", (4 * D,), std=0.05)
    xd, wd, bd = t(x).to(device), t(w).to(device), t(b).to(device)
    y32 = tspn.ops.conv3_tc_wino63(xd, tspn.ops.pack_conv3_wino63(wd, split=D), bd)
    y16 = tspn.ops.conv3_tc_wino63_f16x3(xd, tspn.ops.pack_conv3_wino63_f16x3(wd, split=D), bd)
    d = (y16 - y32).abs().max().item()
    print(f"cfg2 step: max |f16x3 - fp32 F(6,3)| = {d:.3g}")
    assert d <= 1e-4
    rows = [0, 1, 2047, 4095, 4096, 6000, 8191]
    stacked = np.concatenate([w[:, :D], w[:, D:]], axis=0)[rows]
    for tr in (0, NT - 1):
        ref = conv_ref(x[tr:tr + 1], stacked, b[rows])[0]
        got = y16[tr, rows].cpu().numpy()
        e = np.abs(got - ref).max()
        print(f"tracklet {tr}: max |f16x3 - float64| over {len(rows)} rows = {e:.3g}")
        assert e <= 1e-4


def test_conv3_wino63_f16x3_bit_identical_under_concurrent_traffic(tspn, device):
    """24 launches while another stream runs GEMMs: every result equal to the first, bit for bit (each workgroup owns
    its tile and reads back only its own parked points)."""
    B, T, Cin, M = 24, 150, 256, 512
    x = t(tspn.hashrng.uniform(85, "x", (B, T, Cin))).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(tspn.hashrng.normal(85, "w", (M, Cin, 3), std=0.05)).to(device))
    first = tspn.ops.conv3_tc_wino63_f16x3(x, pk)
    side = torch.cuda.Stream(device)
    a = torch.randn(2048, 2048, device=device)
    outs = []
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a).clamp_(-1, 1)
    for _ in range(24):
        outs.append(tspn.ops.conv3_tc_wino63_f16x3(x, pk))
    torch.cuda.synchronize(device)
    assert all(torch.equal(o, first) for o in outs)


def _model(tspn, D, seed, std, **over):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D, **over})
    model = tspn.BaseModel(cfg)
    sd = tspn.synth.make_weights(seed, c=2 * D, bias_std=0.05)
    sd[DPN_PRE + "conv.weight"] = (tspn.hashrng.normal(seed, "cw", sd[DPN_PRE + "conv.weight"].shape, std=std)
                                   .astype(np.float32))
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.eval()


def test_basemodel_promotes_to_f16x3_and_falls_back_on_nonfinite(tspn, device):
    """First call: fp32 F(6,3), spot-checked.  Calls 2 .. 4 each read a measurement within CONV_TOL and still run fp32
    (bit for bit the first call); call 5 is the CONV_F16X3_AFTER = 4th such reading, so it runs the split form (its own
    cache entry, not a conv_split* one) -- close to the fp32 calls and spot-checked in the same words.  A NaN / Inf in
    the features then reads +Inf and the next call runs the direct kernel with the usual warning; CONV_F16X3 = False
    never promotes, CONV_F16X3_AFTER = 1 promotes at the second call."""
    D, N, T = 128, 5, 33
    feats = tspn.hashrng.uniform(86, "x", (N, T, D))
    vid = tspn.synth.make_video(86, N, T, D)
    mk = lambda f: [tspn.PairList.from_tracklets(t(f).to(device), t(vid["tracklet_boxes"]).to(device),  # noqa: E731
                                                 t(vid["track_cls_logits"]).to(device))]
    model = _model(tspn, D, 86, 0.02).to(device)
    store = model.relpn.duration_proposal_network._cache._store
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _, dp1, lg1 = model(mk(feats), None)
        torch.cuda.synchronize(device)
        assert not model.conv_promoted and not any(k.startswith("wino63_f16x3") for k in store)
        assert model.conv_f16x3_after == 4
        for k in range(2, 5):
            _, dpk, _ = model(mk(feats), None)
            torch.cuda.synchronize(device)
            assert model.conv_clean_reads == k - 1 and not model.conv_promoted
            assert torch.equal(dpk[0].heads, dp1[0].heads)
        _, dp2, lg2 = model(mk(feats), None)
        torch.cuda.synchronize(device)
        assert model.conv_promoted and any(k.startswith("wino63_f16x3") for k in store)
        assert sum(k.startswith("conv_split") for k in store) == 1
        d = (dp2[0].heads - dp1[0].heads).abs().max().item()
        print(f"promoted call vs first call: max |diff| = {d:.3g}")
        assert d <= 1e-4 and torch.equal(lg1[0], lg2[0])
        _, dp3, _ = model(mk(feats), None)
        torch.cuda.synchronize(device)
        assert torch.equal(dp2[0].heads, dp3[0].heads) and not rec
        bad = feats.copy()
        bad[2, 17, 5] = np.nan
        bad[3, 0, 9] = np.inf
        model(mk(bad), None)
        torch.cuda.synchronize(device)
        assert not rec
        _, dp5, _ = model(mk(feats), None)
        torch.cuda.synchronize(device)
    msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(msgs) == 1 and "direct kernel" in msgs[0] and model.conv_fallback
    direct = _model(tspn, D, 86, 0.02, **{"RELPN.DPN.CONV_ALGO": "direct"}).to(device)
    _, dpd, _ = direct(mk(feats), None)
    assert torch.equal(dp5[0].heads, dpd[0].heads)

    off = _model(tspn, D, 86, 0.02, **{"RELPN.DPN.CONV_F16X3": False}).to(device)
    for _ in range(6):
        off(mk(feats), None)
        torch.cuda.synchronize(device)
    assert not off.conv_promoted
    assert not any(k.startswith("wino63_f16x3") for k in off.relpn.duration_proposal_network._cache._store)

    early = _model(tspn, D, 86, 0.02, **{"RELPN.DPN.CONV_F16X3_AFTER": 1}).to(device)
    early(mk(feats), None)
    torch.cuda.synchronize(device)
    assert not early.conv_promoted
    _, dpe, _ = early(mk(feats), None)
    torch.cuda.synchronize(device)
    assert early.conv_promoted and torch.equal(dpe[0].heads, dp2[0].heads)
