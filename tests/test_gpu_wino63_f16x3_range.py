"""Split-fp16 F(6,3) on inputs with a wide dynamic range inside one scaled column.

The split form scales each (point, sextet) column of the transformed input over ALL channels, and each (point, row) of the
transformed weights over all channels, so that the largest value lies in [2^14, 2^15), and keeps v ~ hi + lo in fp16.  lo
is a multiple of fp16's subnormal spacing 2^-24, so one element keeps
    |dv| <= 2^-22 |v| + 2^-25 2^-e,   2^-40 colmax < 2^-25 2^-e <= 2^-39 colmax
(and the same for a weight against its row maximum); the product drops lo.lo <= 2^-22 |u||v|.  Per point j this gives,
with the floor at its typical 2^-40 (the constant c below absorbs the factor of up to 2),
    |err_j| <= 3 2^-22 sum_c |U||V|  +  2^-40 (colmax_j sum_c |U_jc| + rowmax_j sum_c |V_jc|)
The first term is relative, like fp32's own rounding; the second is an ABSOLUTE floor set by the largest value of the column:
a channel far above the others that the weights ignore (a dead hot channel) costs every other channel its low bits.  The
fp32 form has no such term.  After the inverse transform the norm-wise bound of output frame i is
    N_i = 2^-40 sum_j |A^T_ij| (colmax_j sum_c |U_jc| + rowmax_j sum_c |V_jc|)
Here the hot channel is multiplied by `hot` and its weights are zero (and the mirrored case: a hot weight column meeting
a zero feature channel).  Checked against float64 conv1d:
  * the fp32 F(6,3) form stays inside 64 eps sum|x||w| on every one of these inputs;
  * the split form stays inside it wherever the float64 restatement below does with a margin of 4 (hot <= 1e6);
  * elsewhere |err| <= c N + 64 eps sum|x||w| with c = 4 x the restatement's own largest err / N on the same inputs, over
    the outputs where the restatement is NOT inside 16 eps sum|x||w| (the others say nothing about the floor: their
    error is the relative term); 4: the kernel transforms in fp32 and accumulates in fp32 in the MFMA's order;
  * from hot = 1e8 on the error is above CONV_TOL = 1e-4, and the guard sees that: a spot-checked fused pass reads more
    than CONV_TOL, and a promoted BaseModel falls back to the direct kernel with its one warning.
Measured figures: profiles/r9/f16x3_range.md."""
import warnings

import numpy as np
import pytest
import torch

import cases

DPN_PRE = "relpn.duration_proposal_network.dpn_head."
EPS = 2.0 ** -24
CONV_TOL = 1e-4
HOTS = [1e2, 1e4, 1e6, 1e8, 1e10]

# F(6,3) with the points of tspn_wino63.hip: V = BT d (8 frames 6q-1 .. 6q+6), U = G g, y = AT (U . V)
BT = np.array([[1, 0, -5.25, 0, 5.25, 0, -1, 0],
               [0, 1, 1, -4.25, -4.25, 1, 1, 0],
               [0, -1, 1, 4.25, -4.25, -1, 1, 0],
               [0, .5, .25, -2.5, -1.25, 2, 1, 0],
               [0, -.5, .25, 2.5, -1.25, -2, 1, 0],
               [0, 2, 4, -2.5, -5, .5, 1, 0],
               [0, -2, 4, 2.5, -5, -.5, 1, 0],
               [0, -1, 0, 5.25, 0, -5.25, 0, 1]], dtype=np.float64)
G = np.array([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
              [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1] + [1, 1, 1, 1, 1, 1] + [0]] +
              [[0, 1, (-1) ** i, 2 ** i, (-2) ** i, 2.0 ** -i, (-2.0) ** -i, 1 if i == 5 else 0] for i in range(1, 6)],
              dtype=np.float64)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def conv_ref(x_tc, w):
    """x [B,T,Cin], w [M,Cin,3] -> (conv, sum|x||w|), float64 [B,M,T]."""
    xt, wt = t(x_tc).double().transpose(1, 2), t(w).double()
    return (torch.nn.functional.conv1d(xt, wt, padding=1).numpy(),
            torch.nn.functional.conv1d(xt.abs(), wt.abs(), padding=1).numpy())


def split_fp16(u, axis):
    """Scale by the power of two that puts max|u| along `axis` into [2^14, 2^15) (0 for a zero maximum), then
    hi = fp16(u), lo = fp16(u - hi): (hi, lo, exponent), float64 / int."""
    mx = np.abs(u).max(axis=axis, keepdims=True)
    e = np.where(mx > 0, 15 - np.frexp(mx)[1], 0)
    s = np.ldexp(u, e)
    hi = s.astype(np.float32).astype(np.float16).astype(np.float64)
    lo = (s - hi).astype(np.float32).astype(np.float16).astype(np.float64)
    return hi, lo, e


def split_restated(x, w):
    """The split algorithm in float64, from DESIGN.md §4: transforms in float64 (V rounded to the fp32 it is held in), one
    power-of-two scale per (point, sextet) column and per (point, row), hi / lo rounded to fp16, the three products and
    their sums exact (float64), unscaled, inverse transform in float64.  x [B,T,Cin], w [M,Cin,3] ->
    (y [B,M,T], N [B,M,T] = the norm-wise bound of the docstring)."""
    B, T, Cin = x.shape
    M = w.shape[0]
    nq = -(-T // 6)
    xp = np.zeros((B, 6 * nq + 2, Cin))
    xp[:, 1:T + 1] = x
    d = np.stack([xp[:, 6 * q:6 * q + 8] for q in range(nq)], axis=1)              # [B,nq,8,Cin]
    V = np.einsum("ji,bqic->jbqc", BT, d).astype(np.float32).astype(np.float64)    # [8,B,nq,Cin]
    U = np.einsum("jk,mck->jmc", G, w.astype(np.float64))                           # [8,M,Cin]
    vh, vl, ve = split_fp16(V, 3)
    uh, ul, ue = split_fp16(U, 2)
    acc = np.einsum("jmc,jbqc->jbmq", uh, vh) + np.einsum("jmc,jbqc->jbmq", uh, vl) + np.einsum("jmc,jbqc->jbmq", ul, vh)
    Mj = np.ldexp(acc, -(ue[:, None, :, :] + ve.transpose(0, 1, 3, 2)))            # [8,B,M,nq]
    y = np.einsum("ij,jbmq->bmqi", AT, Mj).reshape(B, M, 6 * nq)[:, :, :T]
    colmax, rowmax = np.abs(V).max(axis=3), np.abs(U).max(axis=2)                   # [8,B,nq], [8,M]
    su, sv = np.abs(U).sum(axis=2), np.abs(V).sum(axis=3)                           # [8,M], [8,B,nq]
    per_point = colmax[:, :, None, :] * su[:, None, :, None] + rowmax[:, None, :, None] * sv[:, :, None, :]
    N = 2.0 ** -40 * np.einsum("ij,jbmq->bmqi", np.abs(AT), per_point).reshape(B, M, 6 * nq)[:, :, :T]
    return y, N


def range_case(tspn, kind, Cin, hot, B=2, T=40, M=256):
    """x uniform(0, 1), w ~ N(0, 0.01 sqrt(2048 / Cin)) (the benchmark's distribution at Cin = 2048, the same output
    magnitude at a small Cin).  all_frames / one_frame: channel 5 of x times `hot` (everywhere / at one frame of each
    tracklet), its weights zero.  hot_weight: the weights of channel 5 times `hot`, that feature channel zero."""
    seed = 900 + Cin
    x = tspn.hashrng.uniform(seed, "x", (B, T, Cin)).astype(np.float32)
    w = tspn.hashrng.normal(seed, "w", (M, Cin, 3), std=0.01 * np.sqrt(2048.0 / Cin)).astype(np.float32)
    c = 5
    if kind == "all_frames":
        x[:, :, c] *= np.float32(hot)
        w[:, c, :] = 0
    elif kind == "one_frame":
        x[:, :, c] = 0
        x[:, 16, c] = np.float32(hot) * (0.5 + 0.5 * x[:, 16, c + 1])
        w[:, c, :] = 0
    else:
        w[:, c, :] *= np.float32(hot)
        x[:, :, c] = 0
    return x, w


def ratios(y, ref, mag, N):
    """(largest err / eps sum|x||w|, largest err, largest err / N over the outputs outside 16 eps sum|x||w|)."""
    e = np.abs(np.asarray(y, np.float64) - ref)
    out = e > 16.0 * EPS * mag
    return float((e / (EPS * mag)).max()), float(e.max()), float((e[out] / N[out]).max()) if out.any() else 0.0


def test_restatement_is_f63_and_its_split_holds_the_stated_element_bound(tspn):
    """Without a GPU: the matrices above are an exact F(6,3) (float64 error at rounding level), hi + lo keeps every element
    within 2^-22 |v| + 2^-39 colmax, and on the benign case the restated split form is well inside 64 eps sum|x||w|."""
    x, w = range_case(tspn, "all_frames", 64, 1.0, B=2, T=20, M=32)
    ref, mag = conv_ref(x, w)
    nq = 4
    xp = np.zeros((2, 6 * nq + 2, 64))
    xp[:, 1:21] = x
    d = np.stack([xp[:, 6 * q:6 * q + 8] for q in range(nq)], axis=1)
    exact = np.einsum("ij,jbmq->bmqi", AT, np.einsum("jmc,jbqc->jbmq", np.einsum("jk,mck->jmc", G, w.astype(np.float64)),
                                                     np.einsum("ji,bqic->jbqc", BT, d))).reshape(2, 32, 24)[:, :, :20]
    assert np.abs(exact - ref).max() <= 1e-12
    v = tspn.hashrng.normal(1, "v", (50, 64), std=1.0) * np.array([1e6] + [1.0] * 63)
    hi, lo, e = split_fp16(v, 1)
    err = np.abs(np.ldexp(hi + lo, -e) - v)
    assert (err <= 2.0 ** -22 * np.abs(v) + 2.0 ** -39 * np.abs(v).max(axis=1, keepdims=True)).all()
    assert (err > 2.0 ** -22 * np.abs(v) + 2.0 ** -42 * np.abs(v).max(axis=1, keepdims=True)).any()   # the floor is real
    y, N = split_restated(x, w)
    assert ratios(y, ref, mag, N)[0] <= 16.0


@pytest.mark.gpu
@pytest.mark.parametrize("hot", HOTS)
@pytest.mark.parametrize("kind", ["all_frames", "one_frame", "hot_weight"])
@pytest.mark.parametrize("Cin", [2048, 64])
def test_f16x3_wide_in_column_range(tspn, device, Cin, kind, hot):
    x, w = range_case(tspn, kind, Cin, hot)
    ref, mag = conv_ref(x, w)
    xd, wd = t(x).to(device), t(w).to(device)
    y32 = tspn.ops.conv3_tc_wino63(xd, tspn.ops.pack_conv3_wino63(wd)).cpu().numpy()
    y16 = tspn.ops.conv3_tc_wino63_f16x3(xd, tspn.ops.pack_conv3_wino63_f16x3(wd)).cpu().numpy()
    yr, N = split_restated(x, w)
    r32, r16, rr = ratios(y32, ref, mag, N), ratios(y16, ref, mag, N), ratios(yr, ref, mag, N)
    c = 4.0 * rr[2]
    print(f"RANGE Cin={Cin} kind={kind} hot={hot:g} max|y|={np.abs(ref).max():.3g} | (err/eps sum|x||w|, abs err, err/N): "
          f"fp32 F(6,3) {r32[0]:.3g} {r32[1]:.3g} - | f16x3 {r16[0]:.3g} {r16[1]:.3g} {r16[2]:.3g} | "
          f"restated {rr[0]:.3g} {rr[1]:.3g} {rr[2]:.3g} | c={c:.3g}")
    assert np.isfinite(y16).all() and np.isfinite(y32).all()
    assert r32[0] <= 64.0, "fp32 F(6,3) outside 64 eps sum|x||w|"
    if hot <= 1e6 and Cin == 2048:     # (at Cin = 64 with its larger weights hot = 1e6 is already past it: 19 .. 32)
        assert rr[0] <= 16.0, "the restatement was expected inside 64 eps sum|x||w| with a margin of 4 up to hot = 1e6"
    if rr[0] <= 16.0:
        assert r16[0] <= 64.0, "split form outside 64 eps sum|x||w| where its float64 restatement is inside with margin"
    else:
        bound = c * N + 64.0 * EPS * mag
        worst = float((np.abs(y16 - ref) / bound).max())
        assert worst <= 1.0, f"split form at {worst:.3g} of the norm-wise bound (c = {c:.3g})"
    if hot >= 1e8:
        assert r16[1] > CONV_TOL          # what the guard has to see (test_f16x3_guard_trips_on_a_dead_hot_channel)


def fused_operands(tspn, device, D, hot, kind, B=2, N=3, T=40):
    """A fused pass whose two conv halves are the dead-hot-channel case: feature channel 5 times `hot`, conv.weight zero
    on that channel in both halves (columns 5 and D + 5)."""
    sd = tspn.synth.make_weights(51, c=2 * D, bias_std=0.05)
    cw = tspn.hashrng.normal(51, "cw", sd[DPN_PRE + "conv.weight"].shape, std=0.01 * np.sqrt(2048.0 / D)).astype(np.float32)
    cw[:, 5, :] = 0
    cw[:, D + 5, :] = 0
    feats = tspn.hashrng.uniform(52, "x", (B * N, T, D)).astype(np.float32)
    if kind == "all_frames":
        feats[:, :, 5] *= np.float32(hot)
    else:
        feats[:, :, 5] = 0
        feats[4, 16, 5] = np.float32(hot)
    return sd, cw, feats


@pytest.mark.gpu
@pytest.mark.parametrize("hot", [1e8, 1e10])
@pytest.mark.parametrize("kind", ["all_frames", "one_frame"])
def test_f16x3_guard_trips_on_a_dead_hot_channel(tspn, device, kind, hot):
    """ops.forward_fused with split weights and the spot check on: float64 says the split conv is off by more than
    CONV_TOL on these features, and the guard's error word says so too (the fp32 form on the same features reads
    clean, which is why a model gets promoted on them)."""
    from test_gpu_nonfinite import conv_err_word, zero_conv_words
    B, N, T, D = 2, 3, 40, 256
    sd, cw, feats = fused_operands(tspn, device, D, hot, kind)
    stacked = np.concatenate([cw[:, :D], cw[:, D:]], axis=0)
    ref, mag = conv_ref(feats, stacked)
    d = lambda a: t(a).to(device).contiguous()   # noqa: E731
    conv_w, conv_b = d(cw), d(sd[DPN_PRE + "conv.bias"])
    y16 = tspn.ops.conv3_tc_wino63_f16x3(d(feats), tspn.ops.pack_conv3_wino63_f16x3(conv_w, split=D)).cpu().numpy()
    e16 = float(np.abs(y16 - ref).max())
    assert e16 > CONV_TOL, f"float64: the split conv is within CONV_TOL here ({e16:.3g})"
    hw = d(np.concatenate([sd[DPN_PRE + "relness_pred.weight"][:, :, 0], sd[DPN_PRE + "duration_pred.weight"][:, :, 0]]))
    hb = d(np.concatenate([sd[DPN_PRE + "relness_pred.bias"], sd[DPN_PRE + "duration_pred.bias"]]))
    clw, clb = d(sd["classifier.rel_predictor.weight"]), d(sd["classifier.rel_predictor.bias"])
    pairs = torch.cat([tspn.ops.pair_index(N, device, base=b * N) for b in range(B)])
    read = {}
    try:
        for name, packed in (("fp32 F(6,3)", tspn.ops.pack_conv3_wino63(conv_w, split=D)),
                             ("f16x3", tspn.ops.pack_conv3_wino63_f16x3(conv_w, split=D))):
            zero_conv_words(tspn, device)
            tspn.ops.forward_fused(d(feats), pairs, B, N, packed, conv_b, hw, hb, clw, clb, canonical_pairs=True,
                                   conv_weight=conv_w, conv_check=128)
            torch.cuda.synchronize(device)
            read[name] = conv_err_word(tspn, device)
    finally:
        zero_conv_words(tspn, device)
    print(f"GUARD D={D} kind={kind} hot={hot:g}: float64 max err of the split conv {e16:.3g}; guard reads "
          f"fp32 F(6,3) {read['fp32 F(6,3)'][0]:.3g}, f16x3 {read['f16x3'][0]:.3g} ({read['f16x3'][1]} outputs)")
    assert read["fp32 F(6,3)"][0] <= CONV_TOL and read["fp32 F(6,3)"][1] > 0
    assert read["f16x3"][0] > CONV_TOL and read["f16x3"][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("hot", [1e8, 1e10])
def test_promoted_model_falls_back_on_a_dead_hot_channel(tspn, device, hot):
    """A model promoted on its own (hot) features: the fp32 form reads clean on them, the split form does not.  The call
    after the first split call warns once and runs the direct kernel, bit-equal to a CONV_ALGO: direct model, whose conv
    is within 16 eps sum|x||w| of float64 on the same features."""
    D, N, T = 128, 5, 40
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D, "RELPN.DPN.CONV_F16X3_AFTER": 1})
    sd = tspn.synth.make_weights(53, c=2 * D, bias_std=0.05)
    cw = tspn.hashrng.normal(53, "cw", sd[DPN_PRE + "conv.weight"].shape, std=0.01 * np.sqrt(2048.0 / D)).astype(np.float32)
    cw[:, 5, :] = 0
    cw[:, D + 5, :] = 0
    sd[DPN_PRE + "conv.weight"] = cw

    def make(**over):
        c = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                  "PREDICT.FEATURE_DIM": 2 * D, "RELPN.DPN.CONV_F16X3_AFTER": 1, **over})
        m = tspn.BaseModel(c)
        own = m.state_dict()
        m.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
        return m.eval().to(device)

    del cfg
    feats = tspn.hashrng.uniform(54, "x", (N, T, D)).astype(np.float32)
    feats[:, :, 5] *= np.float32(hot)
    vid = tspn.synth.make_video(54, N, T, D)
    mk = lambda: [tspn.PairList.from_tracklets(t(feats).to(device), t(vid["tracklet_boxes"]).to(device),   # noqa: E731
                                               t(vid["track_cls_logits"]).to(device))]
    stacked = np.concatenate([cw[:, :D], cw[:, D:]], axis=0)
    ref, mag = conv_ref(feats, stacked)
    y16 = tspn.ops.conv3_tc_wino63_f16x3(t(feats).to(device), tspn.ops.pack_conv3_wino63_f16x3(t(cw).to(device), split=D))
    e16 = float(np.abs(y16.cpu().numpy() - ref).max())
    assert e16 > CONV_TOL, f"float64: the split conv is within CONV_TOL here ({e16:.3g})"
    yd = tspn.ops.conv3_tc(t(feats).to(device), tspn.ops.pack_conv3(t(cw).to(device), split=D)).cpu().numpy()
    assert (np.abs(yd - ref) <= 16.0 * EPS * mag + 1e-30).all()
    from test_gpu_nonfinite import zero_conv_words
    try:
        model = make()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            model(mk(), None)                       # fp32 F(6,3), spot-checked
            torch.cuda.synchronize(device)
            model(mk(), None)                       # reads a clean fp32 measurement: promoted, runs the split form
            torch.cuda.synchronize(device)
            assert model.conv_promoted and not model.conv_fallback and not rec
            _, dp3, lg3 = model(mk(), None)         # reads the split form's measurement
            torch.cuda.synchronize(device)
            _, dp4, _ = model(mk(), None)
            torch.cuda.synchronize(device)
        msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
        print(f"MODEL hot={hot:g}: float64 max err of the split conv {e16:.3g}; model.conv_err_seen = {model.conv_err_seen:.3g}")
        assert model.conv_fallback and len(msgs) == 1 and "direct kernel" in msgs[0]
        assert model.conv_err_seen > CONV_TOL
        direct = make(**{"RELPN.DPN.CONV_ALGO": "direct"})
        _, dpd, lgd = direct(mk(), None)
        torch.cuda.synchronize(device)
        assert torch.equal(dp3[0].heads, dpd[0].heads) and torch.equal(dp4[0].heads, dpd[0].heads)
        assert torch.equal(lg3[0], lgd[0])
    finally:
        zero_conv_words(tspn, device)
