"""Span-restricted RelOIPool + predicate head (`tspn_span_predicate_f32`: the split-K GEMM over every (tracklet, frame)
row, `span_prefix_kernel`, `span_combine_kernel`) against a plain float64 reference

    out[p, k] = sigmoid(b[k] + cat(mean_{t in [a,e)} f[s,t,:], mean_{t in [a,e)} f[o,t,:]) . w[k,:])

with [a, e) = oracle.span_frames(spans[p]) -- at product shapes, with several videos in one call, with every span
rewrite rule, with non-finite features, and through BaseModel.forward under RELPN.DPN.POOL_TOP_SPAN.

Tolerance (derived): the GEMM's error per (tracklet, frame, column) is within the direct-contraction bound
16 eps sum_c |f||w|; the float64 prefix sums add nothing visible in fp32; sigmoid has slope <= 1/4; the output is rounded
once to fp32 (<= eps for a value in (0, 1)).  So |got - ref| <= 0.25 * 16 eps * S + eps, S = the span mean of
sum_c |f||w| over both halves, eps = 2^-24."""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_nonfinite import NAN_NEG, NAN_NEG_PAY, NAN_PAY, NAN_POS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
INF = np.float32(np.inf)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def dot_rows(m, wh):
    """[P,D] x [K,D] -> [P,K] float64, products and sums elementwise (no BLAS), a block of rows at a time."""
    P, D = m.shape
    K = wh.shape[0]
    out = np.empty((P, K))
    step = max(1, (1 << 23) // (K * D))
    for lo in range(0, P, step):
        out[lo:lo + step] = (m[lo:lo + step, None, :] * wh[None]).sum(axis=2)
    return out


def span_predicate_ref(f, pairs, spans, w, b):
    """(ref [P,K], z [P,K] = the value before the sigmoid, S [P,K], frames [P,2]) in float64.  S = span mean of
    sum_c |f||w| over both halves, with non-finite |f| counted as 0 (it only scales the tolerance of finite outputs)."""
    NT, T, D = f.shape
    w = np.asarray(w, np.float64)
    frames = np.array([oracle.span_frames(a, e, T) for a, e in spans], dtype=np.int64).reshape(-1, 2)
    P, K = len(pairs), w.shape[0]
    z, S = np.zeros((P, K)), np.zeros((P, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for h in (0, 1):
            m, ma = np.empty((P, D)), np.empty((P, D))
            for p in range(P):
                a, e = frames[p]
                x = f[pairs[p, h], a:e].astype(np.float64)
                m[p] = x.sum(axis=0) / (e - a)
                ma[p] = np.where(np.isfinite(x), np.abs(x), 0.0).sum(axis=0) / (e - a)
            wh = w[:, h * D:(h + 1) * D]
            z += dot_rows(m, wh)
            S += dot_rows(ma, np.abs(wh))
        if b is not None:
            z = z + np.asarray(b, np.float64)[None]
        ref = 1.0 / (1.0 + np.exp(-z))
    return ref, z, S, frames


def check_against_ref(got, ref, z, S, what):
    """NaN exactly where the reference is NaN, 1 / 0 where it is +Inf / -Inf before the sigmoid, the derived tolerance
    elsewhere.  Returns the largest error in units of the tolerance."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(z)), \
        f"{what}: NaN positions differ at {np.argwhere(np.isnan(got) != np.isnan(z))[:5].tolist()}"
    assert (got[np.isposinf(z)] == 1.0).all() and (got[np.isneginf(z)] == 0.0).all(), f"{what}: +-Inf logits"
    fin = np.isfinite(z)
    tol = 0.25 * 16 * EPS * S + EPS
    ratio = np.abs(got - ref)[fin] / tol[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: max |got - ref| = {float(np.abs(got - ref)[fin].max()) if ratio.size else 0.0:.3g}, "
          f"{worst:.3f} of the tolerance (S up to {float(S.max()):.3g})")
    assert worst <= 1.0, f"{what}: error {worst:.3f} x the tolerance 0.25 * 16 eps S + eps"
    return worst


def rule_rows(T):
    """One row per rewrite rule of oracle.span_frames, the one-frame span at 0 and at T-1, the whole segment."""
    h = T // 2
    return [(-1, -1), (-3, 0), (-1, 10), (h, h), (h + 2, h - 1), (T - 1, T), (T, T + 4), (T + 5, T + 9), (0, T + 1),
            (0, T), (0, 1)]


def draw_spans(rs, P, T):
    """Random valid spans; the first rows are rule_rows(T); every fourth row after them is a whole-segment row in one of
    its four spellings."""
    rules = rule_rows(T)
    assert P >= len(rules) + 8
    a = rs.randint(0, T, size=P)
    e = np.minimum(a + 1 + rs.randint(0, T, size=P), T)
    spans = np.stack([a, e], axis=1).astype(np.int64)
    spans[:len(rules)] = rules
    whole = [(0, T), (-1, -1), (0, T + 1), (-3, 0)]
    for j, p in enumerate(range(len(rules), P, 4)):
        spans[p] = whole[j % 4]
    return spans


def make_operands(seed, NT, T, D, K):
    rs = np.random.RandomState(seed)
    f = rs.uniform(-1.0, 1.0, size=(NT, T, D)).astype(np.float32)
    w = (0.05 * rs.standard_normal((K, 2 * D))).astype(np.float32)
    b = (0.1 * rs.standard_normal(K)).astype(np.float32)
    return rs, f, w, b


def all_pairs_with_self(NT, rows):
    """Every ordered pair of NT tracklets, (i, i) included, repeated until there are at least `rows` rows."""
    base = np.array([(s, o) for s in range(NT) for o in range(NT)], dtype=np.int64)
    return np.tile(base, (-(-rows // len(base)), 1))


def fused_logits(tspn, device, fd, pd, B, N, wd, bd):
    """rel_logits of ops.forward_fused on the same features, pairs and predicate head (the encoder's weights are zero:
    the logits do not depend on them)."""
    D = fd.shape[2]
    C = 2 * D
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)   # noqa: E731
    packed = tspn.ops.pack_conv3(z(C, C, 3), split=D)
    return tspn.ops.forward_fused(fd, pd, B, N, packed, z(C), z(3, C), z(3), wd, bd)[1]


def run_case(tspn, device, what, f, pairs, spans, w, b, fused=None):
    fd, pd, sd_, wd, bd = (t(x).to(device) for x in (f, pairs, spans, w, b))
    got = tspn.ops.span_predicate(fd, pd, sd_, wd, bd).cpu().numpy()
    ref, z, S, frames = span_predicate_ref(f, pairs, spans, w, b)
    check_against_ref(got, ref, z, S, what)
    if fused is not None:
        # whole-segment rows against the fused pass of the same call.  The fused pass takes the segment mean in fp32
        # first (T sequential adds: worst case (T - 1) eps of sum|f|, one rounding for the division), runs the same
        # GEMM on it (16 eps), adds the two halves and the bias in fp32 (two roundings of at most eps (S + |b|)) and
        # evaluates the sigmoid in fp32 (expf, an add, a division: 4 eps of a value <= 1)
        T = f.shape[1]
        lg = fused_logits(tspn, device, fd, pd, fused[0], fused[1], wd, bd).cpu().numpy().astype(np.float64)
        rows = np.flatnonzero((frames[:, 0] == 0) & (frames[:, 1] == T))
        assert rows.size >= 8
        tol_f = 0.25 * (18 + T) * EPS * (S + np.abs(np.asarray(b, np.float64))[None]) + 4 * EPS
        tol_s = 0.25 * 16 * EPS * S + EPS
        assert (np.abs(lg - ref)[rows] <= tol_f[rows]).all(), f"{what}: fused logits against float64"
        assert (np.abs(lg - got)[rows] <= (tol_f + tol_s)[rows]).all(), f"{what}: whole-segment spans against fused"
    return got


# ------------------------------------------------------------------------------------------------ product shapes
def test_span_predicate_cfg2_video_all_pairs(tspn, device):
    """One cfg2 video (N = 32, T = 150, D = 2048, K = 132), all 992 pairs: 4800 GEMM rows = 75 row tiles, two column tiles
    (2K = 264 > 144), one split."""
    N, T, D, K = 32, 150, 2048, 132
    rs, f, w, b = make_operands(701, N, T, D, K)
    pairs = oracle.pair_index(N).numpy()
    run_case(tspn, device, "cfg2 video", f, pairs, draw_spans(rs, len(pairs), T), w, b, fused=(1, N))


def test_span_predicate_four_videos_global_ids_shuffled_table(tspn, device):
    """Four cfg2 videos in one call, as forward() batches them: global tracklet ids, the pair table in shuffled order
    (1200 of the 3968 in-video pairs; the float64 reference is what bounds the count)."""
    B, N, T, D, K = 4, 32, 150, 2048, 132
    rs, f, w, b = make_operands(702, B * N, T, D, K)
    pairs = np.concatenate([oracle.pair_index(N).numpy() + v * N for v in range(B)])
    pairs = pairs[rs.permutation(len(pairs))[:1200]]
    assert len({int(p) // N for p in pairs[:, 0]}) == B
    run_case(tspn, device, "4 videos", f, pairs, draw_spans(rs, len(pairs), T), w, b, fused=(B, N))


def test_span_predicate_cfg3_shape_sampled_pairs(tspn, device):
    """The cfg3 shape (N = 64, T = 900, D = 1024): 57600 GEMM rows, prefix sums over 900 frames; 96 sampled pairs."""
    N, T, D, K = 64, 900, 1024, 132
    rs, f, w, b = make_operands(703, N, T, D, K)
    allp = oracle.pair_index(N).numpy()
    pairs = allp[rs.permutation(len(allp))[:96]]
    run_case(tspn, device, "cfg3 shape", f, pairs, draw_spans(rs, len(pairs), T), w, b)


@pytest.mark.parametrize("NT,T,D,K,with_fused", [
    (5, 7, 13, 1, True),         # D not a multiple of 32 (nor of 4), K = 1
    (4, 6, 40, 145, True),       # 2K = 290: two 144-column tiles plus two columns
    (3, 1, 16, 3, True),         # T = 1: every span is the one frame
    (1, 9, 8, 5, False),         # NT = 1: the pair (0, 0) only
    (6, 33, 100, 132, True),     # odd T, D % 32 = 4
])
def test_span_predicate_ragged_small_shapes(tspn, device, NT, T, D, K, with_fused):
    rs, f, w, b = make_operands(704 + NT, NT, T, D, K)
    pairs = all_pairs_with_self(NT, 40)
    if NT == 1:
        assert (pairs == 0).all()
    run_case(tspn, device, f"NT={NT} T={T} D={D} K={K}", f, pairs, draw_spans(rs, len(pairs), T), w, b,
             fused=(1, NT) if with_fused else None)


def test_span_predicate_prefix_and_combine_grids_stride(tspn, device):
    """NT * 2K > 8192 * 256 and P * K > 8192 * 256: both grids are capped at 8192 blocks and stride."""
    NT, T, D, K, P = 8000, 3, 4, 132, 16000
    assert NT * 2 * K > 8192 * 256 and P * K > 8192 * 256
    rs, f, w, b = make_operands(705, NT, T, D, K)
    pairs = rs.randint(0, NT, size=(P, 2)).astype(np.int64)
    pairs[-1] = (NT - 1, NT - 1)
    run_case(tspn, device, "strided grids", f, pairs, draw_spans(rs, P, T), w, b)


# ------------------------------------------------------------------------------------------------ non-finite features
PLANTED = [("+inf", INF, False), ("-inf", -INF, False), ("nan", NAN_POS, False), ("-nan", NAN_NEG, False),
           ("nan payload", NAN_PAY, False), ("-nan payload", NAN_NEG_PAY, False), ("inf * 0", INF, True)]


@pytest.mark.parametrize("NT,T,D,K", [(6, 12, 24, 9), (8, 150, 64, 132)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("name,value,zero_weight", PLANTED, ids=[p[0].replace(" ", "") for p in PLANTED])
def test_span_predicate_nonfinite_stays_in_the_spans_that_hold_it(tspn, device, NT, T, D, K, where, name, value,
                                                                  zero_weight):
    """One non-finite value in one channel of one frame of one tracklet.  (a) NaN exactly where the float64 reference has
    NaN, 0 / 1 where it has -Inf / +Inf, the tolerance elsewhere; (b) every output of a pair that does not use the
    tracklet, and of a pair whose span excludes the frame, is bit for bit the clean launch's -- the running prefix sum
    of span_prefix_kernel is non-finite from the planted frame on, and must not reach the spans behind it."""
    trk, ch = 2, 3
    frame = {"first": 0, "middle": T // 2, "last": T - 1}[where]
    rs, f, w, b = make_operands(710, NT, T, D, K)
    if zero_weight:
        w[1, ch] = 0.0           # subject half of predicate 1, object half of predicate K - 1: Inf * 0 = NaN there
        w[K - 1, D + ch] = 0.0
    pairs = all_pairs_with_self(NT, 6 * NT * NT)
    spans = draw_spans(rs, len(pairs), T)
    bad = f.copy()
    bad[trk, frame, ch] = value
    d = lambda x: t(x).to(device)   # noqa: E731
    clean = tspn.ops.span_predicate(d(f), d(pairs), d(spans), d(w), d(b)).cpu().numpy()
    got = tspn.ops.span_predicate(d(bad), d(pairs), d(spans), d(w), d(b)).cpu().numpy()
    ref, z, S, frames = span_predicate_ref(bad, pairs, spans, w, b)
    uses = (pairs == trk).any(axis=1)
    holds = uses & (frames[:, 0] <= frame) & (frame < frames[:, 1])
    assert holds.any() and (uses & ~holds).any() and (~uses).any()
    if frame < T - 1:
        assert (uses & (frames[:, 0] > frame)).any()          # spans that start behind the planted frame
    assert np.isfinite(z[~holds]).all() and not np.isfinite(z[holds]).any()
    if zero_weight:
        assert np.isnan(z[holds][:, [1, K - 1]]).any() and np.isinf(z[holds]).any()
    check_against_ref(got, ref, z, S, f"{name} at frame {frame}")
    assert np.isfinite(clean).all()
    leaked = np.argwhere(bits(got)[~holds] != bits(clean)[~holds])
    assert leaked.size == 0, (f"{name} at frame {frame}: {len(leaked)} outputs of pairs / spans that do not hold the "
                              f"planted value differ from the clean launch, first {got[~holds][tuple(leaked[0])]}")


# ------------------------------------------------------------------------------------------------ model level
def _temporal_model(tspn, D, sd, pool_top_span):
    import cases
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D})
    cfg.RELPN.DPN.POOL_TOP_SPAN = pool_top_span
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.eval()


def test_pool_top_span_forward_on_a_batch_of_three_videos(tspn, device):
    """RELPN.DPN.POOL_TOP_SPAN through BaseModel.forward on three equal-shape videos (one fused pass, the batched pair
    table with global ids, one span_predicate call): per video the logits equal the float64 reference pooled over the
    spans oracle.decode_spans picks from the returned heads.  The third video holds a tracklet that is NaN throughout:
    its pairs have no proposal (span -1 -> the whole segment -> NaN logits), every other pair is untouched."""
    D, n, T = 24, 7, 30
    sd = tspn.synth.make_weights(0, c=2 * D, bias_std=0.05)
    model = _temporal_model(tspn, D, sd, True)
    vids = [tspn.synth.make_video(760 + k, n, T, D) for k in range(3)]
    vids[2]["tracklet_feats"][4] = NAN_POS
    pls = [tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(device), t(v["tracklet_boxes"]).to(device),
                                        t(v["track_cls_logits"]).to(device)) for v in vids]
    _, dp, lg = model(pls, None)
    w, b = sd["classifier.rel_predictor.weight"], sd["classifier.rel_predictor.bias"]
    pairs = oracle.pair_index(n).numpy()
    for k, v in enumerate(vids):
        sp = oracle.decode_spans(dp[k].relness.cpu(), dp[k].duration.cpu(), model.anchor_sizes(T), top_k=1)["span"][:, 0]
        sp = sp.numpy()
        np.testing.assert_array_equal(model.decode_spans([dp[k]], top_k=1)[0]["span"][:, 0].cpu().numpy(), sp)
        ref, z, S, _ = span_predicate_ref(v["tracklet_feats"], pairs, sp, w, b)
        no_proposal = (pairs == 4).any(axis=1) if k == 2 else np.zeros(len(pairs), bool)
        assert ((sp == -1).all(axis=1) == no_proposal).all()
        assert np.isnan(z[no_proposal]).all() and np.isfinite(z[~no_proposal]).all()
        check_against_ref(lg[k].cpu().numpy(), ref, z, S, f"POOL_TOP_SPAN video {k}")


def test_pair_without_a_proposal_pools_over_the_whole_segment(tspn, device):
    """A pair whose heads are all NaN has no span proposal: decode_spans writes (-1, -1), and classify_spans pools such a
    row over the whole segment -- the logits forward() gives that pair without spans."""
    D, n, T = 24, 5, 30
    sd = tspn.synth.make_weights(1, c=2 * D, bias_std=0.05)
    model = _temporal_model(tspn, D, sd, False)
    v = tspn.synth.make_video(770, n, T, D)
    pl = tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(device), t(v["tracklet_boxes"]).to(device),
                                      t(v["track_cls_logits"]).to(device))
    _, dp, lg = model([pl], None)
    heads = dp[0].heads.clone()
    heads[3] = float("nan")
    doctored = [model.relpn.duration_proposal_network._wrap(heads)]
    sp = model.decode_spans(doctored, top_k=1)[0]["span"][:, 0]
    assert sp[3].tolist() == [-1, -1] and (sp[[0, 1, 2, 4]] >= 0).all()
    got = model.classify_spans([pl], [sp])[0].cpu().numpy()
    pairs = oracle.pair_index(n).numpy()
    ref, z, S, frames = span_predicate_ref(v["tracklet_feats"], pairs, sp.cpu().numpy(), sd["classifier.rel_predictor.weight"],
                                           sd["classifier.rel_predictor.bias"])
    assert frames[3].tolist() == [0, T]
    check_against_ref(got, ref, z, S, "classify_spans")
    tol = 0.25 * (18 + T + 16) * EPS * (S[3] + np.abs(sd["classifier.rel_predictor.bias"])) + 5 * EPS   # see run_case
    assert (np.abs(got[3].astype(np.float64) - lg[0][3].cpu().numpy()) <= tol).all()
