"""Non-finite inputs through the scoring path (DESIGN.md §2 "Non-finite values").

Elementwise and contraction kernels: on inputs that are finite except for planted +-Inf / NaN values (either sign, any
payload), every output is NaN, +Inf or -Inf exactly where the float64 reference's is, and within the usual tolerance
elsewhere.  The references here multiply and sum elementwise (no BLAS), so Inf * 0 = NaN holds in them by construction.
Selection (PPN top-k, decode_topk, the class argmax) follows torch: NaN ranks above +Inf, ties go to the lower index,
argmax returns the first NaN.  Span decode skips a candidate with a NaN logit, d_c or d_w (oracle.decode_spans).
The accuracy guard of the Winograd conv reads +Inf for a non-finite deviation and names the NaN's sextet hot."""
import warnings

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DPN_PRE = "relpn.duration_proposal_network.dpn_head."
PPN_PRE = "relpn.pair_proposal_network.ppn_head."
NAN_POS = np.uint32(0x7fc00000).view(np.float32)
NAN_NEG = np.uint32(0xffc00000).view(np.float32)
NAN_PAY = np.uint32(0x7f800123).view(np.float32)        # signalling payload
NAN_NEG_PAY = np.uint32(0xffc0abcd).view(np.float32)
NANS = (NAN_POS, NAN_NEG, NAN_PAY, NAN_NEG_PAY)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def assert_same_nonfinite(got, ref, atol, what=""):
    """NaN / +Inf / -Inf at the same places, finite values within atol."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    for f in (np.isnan, np.isposinf, np.isneginf):
        bad = np.argwhere(f(got) != f(ref))
        assert bad.size == 0, f"{what}: {f.__name__} differs at {bad[:5].tolist()} (got {got[tuple(bad[0])]}, " \
                              f"ref {ref[tuple(bad[0])]})"
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=0, atol=atol, err_msg=what)


def assert_scores_equal(got, ref):
    """Bit-equal, except that any NaN equals any NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    np.testing.assert_array_equal(got[fin].view(np.uint32), ref[fin].view(np.uint32))


def conv_ref(x, w, b, relu):
    """x [B,Cin,T], w [M,Cin,3] -> float64 [B,M,T]: products and sums elementwise (padding 1)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, C, T = x.shape
    xp = np.zeros((B, C, T + 2))
    xp[:, :, 1:T + 1] = x
    with np.errstate(invalid="ignore", over="ignore"):
        y = sum((w[None, :, :, k, None] * xp[:, None, :, k:k + T]).sum(axis=2) for k in range(3))
        if b is not None:
            y = y + np.asarray(b, np.float64)[None, :, None]
        if relu:
            y = np.where(np.isnan(y), y, np.maximum(y, 0.0))
    return y


def heads_ref(h, wh, bh):
    """h [P,C,T] float64, wh [H,C] -> [P,H,T] = wh . h + bh, elementwise products and sums."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(wh, np.float64)[None, :, :, None] * h[:, None]).sum(axis=2) + \
            np.asarray(bh, np.float64)[None, :, None]


def relu64(x):
    return np.where(np.isnan(x), x, np.maximum(x, 0.0))


def plant_frames(x, T, layout):
    """Planted values at frame 0, T-1 and on a sextet boundary (frames 5 / 6), in different tracklets and channels.
    x is [B,C,T] (layout 'cf') or [B,T,C] ('tc')."""
    def put(b, c, f, v):
        if layout == "cf":
            x[b, c, f] = v
        else:
            x[b, f, c] = v
    B = x.shape[0]
    put(0, 1, 0, NAN_POS)
    put(1 % B, 2, T - 1, np.float32(np.inf))
    put(2 % B, 3, min(6, T - 1), -np.float32(np.inf))
    put(2 % B, 4, min(5, T - 1), NAN_NEG_PAY)
    put(1 % B, 5, T // 2, np.float32(np.inf))       # channel 5 has a zero weight in row 0: Inf * 0 = NaN
    return x


# ------------------------------------------------------------------------------ ops: conv3 / conv3_tc
@pytest.mark.parametrize("T", [7, 30, 150])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("layout", ["cf", "tc"])
def test_conv3_nonfinite_positions(tspn, device, T, relu, with_bias, layout):
    B, Cin, M = 3, 32, 40
    x = tspn.hashrng.uniform(301, "x", (B, Cin, T) if layout == "cf" else (B, T, Cin), -1, 1)
    x = plant_frames(x, T, layout)
    w = tspn.hashrng.normal(301, "w", (M, Cin, 3), std=0.1)
    w[0, 5, :] = 0.0
    b = tspn.hashrng.normal(301, "b", (M,), std=0.1) if with_bias else None
    packed = tspn.ops.pack_conv3(t(w).to(device))
    bd = t(b).to(device) if with_bias else None
    if layout == "cf":
        y = tspn.ops.conv3(t(x).to(device), packed, bd, relu=relu)
        ref = conv_ref(x, w, b, relu)
    else:
        y = tspn.ops.conv3_tc(t(x).to(device), packed, bd, relu=relu)
        ref = conv_ref(x.transpose(0, 2, 1), w, b, relu)
    assert np.isnan(ref).any() and np.isinf(ref).any()
    assert_same_nonfinite(y.cpu().numpy(), ref, 2e-5, f"conv3 {layout}")


# ------------------------------------------------------------------------------ bf16
def test_cast_bf16_nonfinite(tspn, device):
    fmax = np.finfo(np.float32).max
    x = np.array([np.inf, -np.inf, fmax, -fmax, 3.3961776e38, 1.0, *NANS], dtype=np.float32)
    got = tspn.ops.cast_bf16(t(x).to(device)).cpu()
    ref = t(x).to(torch.bfloat16)
    g, r = got.float().numpy(), ref.float().numpy()
    assert np.isnan(g[6:]).all()                                    # NaN in -> NaN out (any sign / payload)
    np.testing.assert_array_equal(got[:6].view(torch.int16).numpy(), ref[:6].view(torch.int16).numpy())
    assert np.isposinf(g[2]) and np.isneginf(g[3]) and np.array_equal(g[:6], r[:6])


def test_conv3_tc_bf16_nonfinite(tspn, device):
    B, T, Cin, M = 3, 30, 32, 36
    x = tspn.hashrng.uniform(302, "x", (B, T, Cin), -1, 1)
    x = plant_frames(x, T, "tc")
    xb = t(x).to(torch.bfloat16)
    w = tspn.hashrng.normal(302, "w", (M, Cin, 3), std=0.1)
    w[0, 5, :] = 0.0
    b = tspn.hashrng.normal(302, "b", (M,), std=0.1)
    y = tspn.ops.conv3_tc_bf16(xb.to(device), tspn.ops.pack_conv3_bf16(t(w).to(device)), t(b).to(device))
    wb = oracle.bf16_round(t(w)).numpy()
    ref = conv_ref(xb.float().numpy().transpose(0, 2, 1), wb, b, False).transpose(0, 2, 1)     # [B,T,M]
    assert_same_nonfinite(y.cpu().numpy(), ref, 2e-5, "conv3_tc_bf16")


@pytest.mark.parametrize("B,N,T,C", [(1, 3, 30, 32), (2, 8, 33, 64)])
def test_heads_pairgrid_bf16_nonfinite(tspn, device, B, N, T, C):
    """0xffc00000 (negative quiet NaN) planted directly in y: relu keeps it (F.relu(NaN) = NaN)."""
    y = tspn.hashrng.normal(303, "y", (B * N, T, 2 * C), std=1.0)
    y[0, 3, 1] = NAN_NEG
    y[1, T - 1, C + 2] = NAN_NEG_PAY
    y[N - 1, 0, 4] = np.inf
    y[N - 1, 7, 5] = -np.inf
    hw = oracle.bf16_round(t(tspn.hashrng.normal(303, "hw", (12, C), std=0.1))).numpy()
    hw[3, 4] = 0.0
    hb = tspn.hashrng.normal(303, "hb", (12,), std=0.1)
    out = tspn.ops.heads_pairgrid_bf16(t(y).to(device), B, N, tspn.ops.pack_heads_bf16(t(hw).to(device)),
                                       t(hb).to(device), 12).cpu().numpy()
    refs = []
    for b in range(B):
        yy = y[b * N:(b + 1) * N]
        pairs = oracle.pair_index(N).numpy()
        with np.errstate(invalid="ignore"):
            a = relu64((yy[pairs[:, 0], :, :C] + yy[pairs[:, 1], :, C:]).astype(np.float32).astype(np.float64))
        a = oracle.bf16_round(t(a.astype(np.float32))).double().numpy().transpose(0, 2, 1)     # [P,C,T]
        refs.append(heads_ref(a, hw, hb))
    ref = np.concatenate(refs)
    assert np.isnan(ref).any()
    assert_same_nonfinite(out, ref, 3e-5, "heads_pairgrid_bf16")


# ------------------------------------------------------------------------------ fp32 heads (three forms)
def test_heads_three_forms_nonfinite(tspn, device):
    P, C, T, H = 6, 64, 30, 12
    a = tspn.hashrng.uniform(304, "a", (P, C, T), -1, 1)
    b = tspn.hashrng.uniform(304, "b", (P, C, T), -1, 1)
    a[0, 1, 0] = NAN_NEG
    a[2, 3, T - 1] = np.inf
    b[1, 4, 6] = -np.inf
    b[3, 5, 5] = NAN_PAY
    wh = tspn.hashrng.normal(304, "wh", (H, C), std=0.1)
    wh[2, 3] = 0.0
    bh = tspn.hashrng.normal(304, "bh", (H,), std=0.1)
    bias = tspn.hashrng.normal(304, "bias", (C,), std=0.3)
    ia = tspn.hashrng.integers(304, "ia", (2 * P,), 0, P)
    ib = tspn.hashrng.integers(304, "ib", (2 * P,), 0, P)
    d = lambda v: t(v).to(device)   # noqa: E731
    out0 = tspn.ops.heads(d(a), d(wh), d(bh)).cpu().numpy()
    assert_same_nonfinite(out0, heads_ref(a.astype(np.float64), wh, bh), 2e-5, "dense heads")
    with np.errstate(invalid="ignore"):
        h = relu64(a.astype(np.float64)[ia] + b.astype(np.float64)[ib] + bias[None, :, None])
    out1 = tspn.ops.heads(d(a), d(wh), d(bh), b=d(b), ia=d(ia), ib=d(ib), bias=d(bias)).cpu().numpy()
    assert_same_nonfinite(out1, heads_ref(h, wh, bh), 2e-5, "factorised heads")
    # pair grid: y [B*N, 2C, T] (subject rows | object rows), canonical pairs
    N = 4
    y = tspn.hashrng.uniform(304, "y", (N, 2 * C, T), -1, 1)
    y[0, 1, 0] = NAN_NEG
    y[1, C + 2, T - 1] = np.inf
    y[2, 3, 6] = -np.inf
    pairs = oracle.pair_index(N).numpy()
    out2 = tspn.ops.heads_pairgrid(d(y), 1, N, d(wh), d(bh)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        h2 = relu64(y.astype(np.float64)[pairs[:, 0], :C] + y.astype(np.float64)[pairs[:, 1], C:])
    assert_same_nonfinite(out2, heads_ref(h2, wh, bh), 2e-5, "pair-grid heads")


# ------------------------------------------------------------------------------ predicate head, PPN, preprocess
@pytest.mark.parametrize("P,F,K", [(5, 31, 7), (4, 3000, 132)])
def test_predicate_head_nonfinite(tspn, device, P, F, K):
    x = tspn.hashrng.uniform(305, "x", (P, F), -1, 1)
    x[0, 3] = NAN_NEG_PAY
    x[1, F - 1] = np.inf
    x[2, 0] = -np.inf
    x[3, F // 2] = np.inf
    w = tspn.hashrng.normal(305, "w", (K, F), std=0.05)
    w[0, F // 2] = 0.0
    b = tspn.hashrng.normal(305, "b", (K,), std=0.1)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (x.astype(np.float64)[:, None, :] * w.astype(np.float64)[None]).sum(-1) + b
    for sig in (False, True):
        got = tspn.ops.predicate_head(t(x).to(device), t(w).to(device), t(b).to(device), apply_sigmoid=sig)
        ref = torch.sigmoid(t(z)).numpy() if sig else z
        assert_same_nonfinite(got.cpu().numpy(), ref, 1e-5, f"predicate head sigmoid={sig}")


def test_ppn_nonfinite_ranking(tspn, device):
    B, N = 2, 8
    sd = tspn.synth.make_weights(3, c=8, bias_std=0.1)
    w_np = {k[len(PPN_PRE):]: v for k, v in sd.items() if k.startswith(PPN_PRE)}
    cls = 6.0 * tspn.hashrng.uniform(306, "cls", (B, N, 35))
    cls[0, 2, :] = NAN_NEG                                          # one tracklet with NaN classeme logits
    cls[1, 5, 7] = NAN_PAY
    cls[1, 1, 3] = np.inf
    w = {k: t(v).to(device) for k, v in w_np.items()}
    mat, idx = tspn.ops.ppn_pair_matrix_topk(t(cls).to(device), w, N * N)
    for b in range(B):
        ref = oracle.ppn_pair_matrix(t(cls[b]).double(), {k: t(v).double() for k, v in w_np.items()})
        m = mat[b].cpu().numpy()
        assert_same_nonfinite(m, ref.numpy(), 2e-6, f"ppn matrix {b}")
        got = idx[b].cpu().numpy()
        np.testing.assert_array_equal(got, oracle.ppn_topk(mat[b].cpu(), N * N).numpy())
        flat = m.reshape(-1)
        nan = np.flatnonzero(np.isnan(flat))
        assert nan.size > 0
        np.testing.assert_array_equal(got[:nan.size], nan)          # NaN first, by index
        fin = got[nan.size:]
        assert np.all(np.diff(flat[fin]) <= 0)                     # finite order survives the NaN rows


def test_feature_preprocess_nonfinite(tspn, device):
    x = tspn.hashrng.uniform(307, "pre", (6, 11070), -1, 1)
    x[0, 100] = NAN_NEG
    x[1, 2500] = np.inf
    x[2, 5000] = -np.inf
    x[3, 8069] = NAN_PAY
    x[4, 2070:3070] = 0
    x[4, 2100] = np.inf
    ref = oracle.feature_preprocess(t(x).double()).numpy()
    got = tspn.ops.feature_preprocess_(t(x).to(device)).cpu().numpy()
    assert_same_nonfinite(got, ref, 1e-7, "feature_preprocess_")


# ------------------------------------------------------------------------------ decode_topk
def decode_logits(S, P, K):
    logit = np.round(uniform(308, (S, P, K)) * 16) / 16
    for s in range(S):
        logit[s, 0, :] = NANS[s % 4]                               # all-NaN row
        logit[s, 1, :K - 3] = np.nan                               # fewer than R finite values
        logit[s, 1, 2] = NAN_NEG
        logit[s, 2, 5] = np.inf                                    # +-Inf ties
        logit[s, 3, 5] = np.inf
        logit[s, 3, 6] = -np.inf
        logit[s, 2, 7] = -np.inf
        logit[s, 4 % P, 9] = NAN_NEG_PAY
        logit[s, 4 % P, 11] = NAN_PAY
        logit[s, 4 % P, 12] = -0.0
        logit[s, 4 % P, 13] = 0.0
    return logit.astype(np.float32)


def uniform(seed, shape):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


@pytest.mark.parametrize("S,N,K,kp,ks", [(2, 3, 20, 20, 200), (2, 3, 132, 20, 200), (2, 8, 132, 20, 200),
                                         (1, 12, 70, 7, 33), (1, 3, 16, 20, 200)])
def test_decode_topk_nonfinite(tspn, device, S, N, K, kp, ks):
    P = N * (N - 1)
    logit = decode_logits(S, P, K)
    feat = uniform(309, (S, P, 75))
    feat[0, 0, 3] = NAN_NEG                                        # argmax -> the first NaN
    feat[0, 0, 5] = NAN_POS
    feat[0, 0, 40] = np.inf
    feat[S - 1, (N - 1) % P, 35:70] = NAN_PAY
    pairs = np.stack([oracle.pair_index(N).numpy()] * S)
    sc, trip, tids = tspn.ops.decode_topk(t(logit).to(device), t(pairs).to(device), t(feat).to(device),
                                          row_mul=N - 1, topk_per_pair=kp, topk_per_seg=ks)
    for s in range(S):
        rs, rt, ri = oracle.decode_topk(t(logit[s]), t(feat[s, :, :70]), t(pairs[s]), N, kp, ks)
        assert sc[s].shape == rs.shape
        assert_scores_equal(sc[s].cpu().numpy(), rs.numpy())
        np.testing.assert_array_equal(trip[s].cpu().numpy(), rt.numpy())
        np.testing.assert_array_equal(tids[s].cpu().numpy(), ri.numpy())
        tr = trip[s].cpu().numpy()
        assert tr[:, 1].min() >= 0 and tr[:, 1].max() < K
        assert tr[:, [0, 2]].min() >= 0 and tr[:, [0, 2]].max() < 35


# ------------------------------------------------------------------------------ decode_spans
@pytest.mark.parametrize("P,A,T,top_k,pre", [(6, 4, 30, 64, 1024), (5, 4, 150, 64, 40), (3, 2, 7, 16, 1024)])
def test_decode_spans_nonfinite(tspn, device, P, A, T, top_k, pre):
    sizes = [4.0, 8.0, 16.0, 32.0][:A]
    heads = tspn.hashrng.normal(309, "spans", (P, 3 * A, T), std=1.0)
    heads[:, :A] = np.round(heads[:, :A] * 8) / 8
    heads[:, A:] *= 0.4
    heads[0, :A] = np.nan                                          # no proposal at all
    heads[1, 0, 0] = NAN_NEG                                       # NaN logit
    heads[1, A + 0, 1] = NAN_PAY                                   # NaN d_c
    heads[1, A + 1, 2] = np.nan                                    # NaN d_w
    heads[1, 1, 3] = np.inf                                        # +-Inf logits rank normally
    heads[1, 1, 4] = np.inf
    heads[1, 0, 5] = -np.inf
    heads[2, A + 2, 1] = np.inf                                    # +-Inf regressions: clamp and clip
    heads[2, A + 3, 2] = np.inf
    heads[2, A + 2, 3] = -np.inf
    heads[2, A + 1, 4] = -np.inf
    heads[2, 1, 1:5] = 9.0                                         # ... and ranked first
    heads[P - 1, :A, : T - 2] = NAN_NEG_PAY                        # fewer proposals than pre_nms / top_k
    got = tspn.ops.decode_spans(t(heads).to(device), sizes, top_k=top_k, pre_nms=pre)
    ref = oracle.decode_spans(t(heads[:, :A]), t(heads[:, A:]), sizes, top_k=top_k, pre_nms=pre)
    assert int(ref["count"][0]) == 0
    for k in ("count", "anchor", "span"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k].numpy(), err_msg=k)
    np.testing.assert_array_equal(got["span_f"].cpu().numpy(), ref["span_f"].numpy())
    np.testing.assert_allclose(got["score"].cpu().numpy(), ref["score"].numpy(), rtol=0, atol=1e-7)


# ------------------------------------------------------------------------------ accuracy guard (ops level)
def conv_err_word(tspn, device):
    w = tspn.ops.status_words(device)
    return float(w[tspn._abi.STATUS_CONV_ERR:tspn._abi.STATUS_CONV_ERR + 1].view(np.float32)[0]), \
        int(w[tspn._abi.STATUS_CONV_CHECKS])


def zero_conv_words(tspn, device):
    w = tspn.ops.status_words(device)
    w[tspn._abi.STATUS_CONV_ERR] = 0
    w[tspn._abi.STATUS_CONV_CHECKS] = 0


def test_guard_reads_inf_on_nonfinite_launches_and_names_the_nan_sextet(tspn, device):
    B, N, T, D = 2, 3, 40, 64
    sd = tspn.synth.make_weights(50, c=2 * D, bias_std=0.05)
    d = lambda a: t(a).to(device).contiguous()   # noqa: E731
    conv_w, conv_b = d(sd[DPN_PRE + "conv.weight"]), d(sd[DPN_PRE + "conv.bias"])
    hw = d(np.concatenate([sd[DPN_PRE + "relness_pred.weight"][:, :, 0], sd[DPN_PRE + "duration_pred.weight"][:, :, 0]]))
    hb = d(np.concatenate([sd[DPN_PRE + "relness_pred.bias"], sd[DPN_PRE + "duration_pred.bias"]]))
    cw, cb = d(sd["classifier.rel_predictor.weight"]), d(sd["classifier.rel_predictor.bias"])
    pairs = torch.cat([tspn.ops.pair_index(N, device, base=b * N) for b in range(B)])
    packed = tspn.ops.pack_conv3_wino63(conv_w, split=D)
    need = tspn.ops.fused_workspace_bytes(B, N, T, D, 4, cw.shape[0], pairs.shape[0])
    nq = (T + 5) // 6
    try:
        # frame 17 is the last frame of sextet 2 and the halo of sextet 3: the sextet that holds it is the hot one
        for trk, frame, val in ((4, 27, NAN_NEG_PAY), (2, 17, NAN_POS), (1, 12, np.float32(np.inf))):
            feats = tspn.hashrng.uniform(7, "x", (B * N, T, D), -1, 1)
            feats[0, 3, 2] = 1e6                                   # a large finite outlier elsewhere: NaN still wins
            feats[trk, frame, 13] = val
            ws = torch.zeros(need, dtype=torch.uint8, device=device)
            zero_conv_words(tspn, device)
            tspn.ops.forward_fused(d(feats), pairs, B, N, packed, conv_b, hw, hb, cw, cb, workspace=ws,
                                   canonical_pairs=True, conv_weight=conv_w, conv_check=16)
            torch.cuda.synchronize(device)
            err, checks = conv_err_word(tspn, device)
            assert err == np.inf and checks > 0, (val, err, checks)
            if np.isnan(val):
                scratch = ws[need - tspn._abi.CONV_CHECK_SCRATCH_BYTES:].view(torch.int64)
                slots = scratch[tspn._abi.CONV_CHECK_HOT_OFFSET // 8::32][:64].cpu().numpy().astype(np.uint64)
                key = int(slots.max())
                assert key & 0xFFFFFFFF == trk * nq + frame // 6
                assert np.isnan(np.array([key >> 32], dtype=np.uint32).view(np.float32)[0])
        # the direct check on an ops-level launch: NaN and Inf in y where float64 is finite read +Inf
        x = tspn.hashrng.uniform(310, "x", (3, 30, 32), -1, 1)
        wt = tspn.hashrng.normal(310, "w", (32, 32, 3), std=0.1)
        xd, wd = t(x).to(device), t(wt).to(device)
        y = tspn.ops.conv3_tc_wino63(xd, tspn.ops.pack_conv3_wino63(wd))
        for bad in (NAN_POS, np.float32(np.inf)):
            y2 = y.clone()
            y2[:, :, :] = float(bad)
            zero_conv_words(tspn, device)
            tspn.ops.conv3_spot_check(xd, wd, y2, rows=32)
            torch.cuda.synchronize(device)
            assert conv_err_word(tspn, device)[0] == np.inf
        # equal non-finite values are error 0: a NaN input whose outputs the direct kernel got right
        x[1, 4, 7] = NAN_NEG
        xd = t(x).to(device)
        yd = tspn.ops.conv3_tc(xd, tspn.ops.pack_conv3(wd))
        zero_conv_words(tspn, device)
        tspn.ops.conv3_spot_check(xd, wd, yd, rows=32, hot=torch.tensor([(0x7fc00000 << 32) | (5 + 0)],
                                                                         dtype=torch.int64, device=device))
        torch.cuda.synchronize(device)
        err, checks = conv_err_word(tspn, device)
        assert np.isfinite(err) and err < 1e-5 and checks > 0
        # after zeroing, a finite launch reads a finite value again
        zero_conv_words(tspn, device)
        xf = t(tspn.hashrng.uniform(311, "x", x.shape, -1, 1)).to(device)
        tspn.ops.conv3_spot_check(xf, wd, tspn.ops.conv3_tc(xf, tspn.ops.pack_conv3(wd)), rows=32)
        torch.cuda.synchronize(device)
        err, checks = conv_err_word(tspn, device)
        assert np.isfinite(err) and err < 1e-5 and checks > 0
    finally:
        zero_conv_words(tspn, device)


# ------------------------------------------------------------------------------ model level
def model_weights(tspn, D, seed=0):
    sd = tspn.synth.make_weights(seed, c=2 * D, bias_std=0.05)
    w = {"conv_w": t(sd[DPN_PRE + "conv.weight"]), "conv_b": t(sd[DPN_PRE + "conv.bias"]),
         "dur_w": t(sd[DPN_PRE + "duration_pred.weight"]), "dur_b": t(sd[DPN_PRE + "duration_pred.bias"]),
         "rel_w": t(sd[DPN_PRE + "relness_pred.weight"]), "rel_b": t(sd[DPN_PRE + "relness_pred.bias"]),
         "cls_w": t(sd["classifier.rel_predictor.weight"]), "cls_b": t(sd["classifier.rel_predictor.bias"])}
    return sd, w


def make_model(tspn, sd, D, algo):
    cfg = tspn.load_cfg(None, **{"RELPN.USE_PPN": True, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                 "PREDICT.FEATURE_DIM": 2 * D, "RELPN.DPN.CONV_ALGO": algo})
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.eval()


def nonfinite_video(tspn, N, T, D):
    v = tspn.synth.make_video(97, N, T, D)
    f = v["tracklet_feats"]
    f[0, 5, :] = NAN_NEG                                          # a NaN frame
    f[1, T - 1, 3] = np.inf                                       # an Inf value on the last frame
    v["track_cls_logits"][N - 1, :] = NAN_PAY                     # one tracklet with a NaN classeme
    return v


def check_decode(model, pl, logits, cls, N, K):
    sc, trip, tids = model.decode([pl], logits)[0]
    lg = logits[0].cpu()
    feat70 = torch.cat([t(cls), t(cls)], dim=1)                   # row_mul = 1: num_tracklets - 1 == 1
    rs, rt, ri = oracle.decode_topk(lg, feat70, oracle.pair_index(N), 2)
    assert_scores_equal(sc.cpu().numpy(), rs.numpy())
    np.testing.assert_array_equal(trip.cpu().numpy(), rt.numpy())
    np.testing.assert_array_equal(tids.cpu().numpy(), ri.numpy())
    tr = trip.cpu().numpy()
    assert tr[:, 1].min() >= 0 and tr[:, 1].max() < K and tr[:, [0, 2]].min() >= 0 and tr[:, [0, 2]].max() < 35
    assert tids.min() >= 0 and tids.max() < N


@pytest.mark.parametrize("N,T,D,bf16", [(3, 30, 64, False), (8, 30, 64, False), (3, 30, 2048, False),
                                        (3, 30, 64, True), (8, 33, 64, True)])
def test_model_direct_and_bf16_nonfinite(tspn, device, N, T, D, bf16):
    sd, w = model_weights(tspn, D)
    model = make_model(tspn, sd, D, "direct").to(device)
    v = nonfinite_video(tspn, N, T, D)
    feats = t(v["tracklet_feats"])
    fd = feats.to(torch.bfloat16) if bf16 else feats
    pl = tspn.PairList.from_tracklets(fd.to(device), t(v["tracklet_boxes"]).to(device),
                                      t(v["track_cls_logits"]).to(device))
    pp, dp, logits = model([pl], None)
    torch.cuda.synchronize(device)
    pairs = oracle.pair_index(N)
    if bf16:
        ref = oracle.forward_bf16(feats, pairs, w)
    else:
        ref = oracle.forward_factorised(feats, t(v["tracklet_boxes"]), pairs, w, dtype=torch.float64)
    for k, got in (("relness", dp[0].relness), ("duration", dp[0].duration), ("rel_logits", logits[0])):
        r = ref[k].double().numpy()
        # bf16: one flipped bf16 activation moves a head output by ~2^-8 |a| |w| (test_gpu_bf16's bound)
        tol = 2e-3 * max(float(np.abs(r[np.isfinite(r)]).max()), 1e-3) if bf16 else 1e-4
        assert_same_nonfinite(got.cpu().numpy(), r, tol, k)
    assert torch.isnan(logits[0]).any()
    # PPN: the NaN tracklet's row and column lead, by index; every id in range
    p = pp[0].cpu().numpy()
    nan_idx = np.array(sorted(set(range((N - 1) * N, N * N)) | set(range(N - 1, N * N, N))))
    np.testing.assert_array_equal(p[:nan_idx.size], nan_idx)
    assert p.min() >= 0 and p.max() < N * N
    check_decode(model, pl, logits, v["track_cls_logits"], N, logits[0].shape[1])


def test_model_auto_falls_back_on_nonfinite_features(tspn, device):
    N, T, D = 3, 30, 64
    sd, _ = model_weights(tspn, D)
    v = nonfinite_video(tspn, N, T, D)
    mk = lambda: [tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(device), t(v["tracklet_boxes"]).to(device),  # noqa: E731
                                               t(v["track_cls_logits"]).to(device))]
    try:
        model = make_model(tspn, sd, D, "auto").to(device)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            model(mk(), None)
            torch.cuda.synchronize(device)
            assert not model.conv_fallback and not rec
            _, dp2, lg2 = model(mk(), None)
            _, dp3, _ = model(mk(), None)
            torch.cuda.synchronize(device)
        msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
        assert len(msgs) == 1 and "direct kernel" in msgs[0] and "NaN" in msgs[0]
        assert model.conv_fallback
        direct = make_model(tspn, sd, D, "direct").to(device)
        _, dpd, lgd = direct(mk(), None)
        torch.cuda.synchronize(device)
        bits = lambda x: x.contiguous().view(torch.int32)   # noqa: E731  (bit-equal, NaN payloads included)
        assert torch.equal(bits(dp2[0].heads), bits(dpd[0].heads)) and torch.equal(bits(dp3[0].heads), bits(dpd[0].heads))
        assert torch.equal(bits(lg2[0]), bits(lgd[0]))
    finally:
        zero_conv_words(tspn, device)
