"""Relations decoded with their temporal spans (`tspn_decode_span_relations_f32`: the shared GEMM + prefix stage,
`span_row_topk_kernel`, `segment_span_topk_kernel`) against the unfused composition
(tests/span_relations_reference.py: `ops.span_predicate` on the flattened (pair, span) rows, two stable torch sorts,
gathers).  Compare and integer work only after the shared per-(row, k) expression, so equality is asked TO THE BIT:
scores as int32 views, every index as it is.  Outputs are pre-filled with a sentinel; rows past `valid` must keep it."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import span_relations_reference as ref

pytestmark = pytest.mark.gpu

SENT_I = -7777
SENT_F_BITS = -559038737          # 0xdeadbeef as int32
NAMES = ("scores", "triplets", "pair_tids", "spans", "span_rank")


def all_pairs(n):
    return torch.tensor([(i, j) for i in range(n) for j in range(n) if i != j], dtype=torch.int64).view(-1, 2)


def make_case(device, S, N, T, D, K, J, seed, NO=35, A=4, pairs=None):
    """Random features / weights / class logits and the `decode_spans(top_k=J)` of random DPN heads for S segments."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g) * 2 - 1   # noqa: E731
    pairs = all_pairs(N) if pairs is None else pairs
    P = pairs.shape[0]
    c = {"S": S, "N": N, "T": T, "D": D, "K": K, "J": J, "P": P, "NO": NO,
         "feats": u(S * N, T, D).to(device), "w": (u(K, 2 * D) * 0.5).to(device), "b": (u(K) * 0.2).to(device),
         "cls": u(S, N, NO).to(device), "pairs": pairs.unsqueeze(0).repeat(S, 1, 1).contiguous().to(device),
         "heads": u(S * P, 3 * A, T), "sizes": [(a + 1) * float(T) / A for a in range(A)]}
    return c


def with_spans(tspn, c, heads=None):
    sp = tspn.ops.decode_spans((c["heads"] if heads is None else heads).to(c["feats"].device), c["sizes"], top_k=c["J"])
    c["spans"], c["score"], c["count"] = sp["span"], sp["score"], sp["count"]
    return c


def sentinel_out(c, R, M, device):
    S = c["S"]
    Mc = min(M, c["P"] * c["J"] * min(R, c["K"]))
    out = (torch.full((S, Mc), SENT_F_BITS, dtype=torch.int32, device=device).view(torch.float32),
           torch.full((S, Mc, 3), SENT_I, dtype=torch.int64, device=device),
           torch.full((S, Mc, 2), SENT_I, dtype=torch.int64, device=device),
           torch.full((S, Mc, 2), SENT_I, dtype=torch.int64, device=device),
           torch.full((S, Mc), SENT_I, dtype=torch.int64, device=device),
           torch.full((S,), SENT_I, dtype=torch.int64, device=device))
    return out


def fused(tspn, c, R, M):
    out = sentinel_out(c, R, M, c["feats"].device)
    res = tspn.ops.decode_span_relations(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["w"], c["b"],
                                         c["cls"], topk_per_span=R, topk_per_seg=M, out=out)
    assert all(a is b for a, b in zip(res, out))
    return [r.cpu().numpy() for r in res]


def composition(tspn, c, R, M):
    rp, rs = ref.span_rows(c["pairs"], c["N"], c["spans"])
    q = tspn.ops.span_predicate(c["feats"], rp, rs, c["w"], c["b"])
    return ref.compose(q, c["pairs"], c["spans"], c["score"], c["count"], c["cls"], R, M), q


def assert_equal(got, want):
    """got: the six fused arrays [S, Mc, ...]; want: compose's per-segment dicts.  Bit equality on the first `valid`
    rows, the sentinel behind them."""
    for s, w in enumerate(want):
        v = w["valid"]
        assert int(got[5][s]) == v, (s, int(got[5][s]), v)
        assert np.array_equal(got[0][s, :v].view(np.int32), w["scores"].view(np.int32)), f"segment {s}: scores"
        for a, name in zip(got[1:5], NAMES[1:]):
            assert a.dtype == np.int64 and np.array_equal(a[s, :v], w[name]), f"segment {s}: {name}"
        assert (got[0][s, v:].view(np.int32) == SENT_F_BITS).all()
        assert all((a[s, v:] == SENT_I).all() for a in got[1:5])


SHAPES = [(1, 2, 1, 16, 1, 1, 1, 1), (1, 5, 7, 16, 64, 3, 20, 200), (3, 5, 12, 32, 132, 4, 20, 200),
          (2, 6, 9, 16, 256, 2, 256, 1024), (1, 32, 6, 16, 132, 4, 20, 200), (1, 4, 5, 24, 65, 16, 70, 50)]


@pytest.mark.parametrize("S,N,T,D,K,J,R,M", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_equals_the_composition(tspn, device, S, N, T, D, K, J, R, M):
    """One lane to four values per lane (K = 1 ... 256), R clamped to K (70 -> 65), one to three segments, P = 992 pairs
    in one segment, M = 1024 (the LDS sort at its capacity), J = 16 with the NMS leaving ragged counts."""
    c = with_spans(tspn, make_case(device, S, N, T, D, K, J, seed=100 + K + J))
    got = fused(tspn, c, R, M)
    want, _ = composition(tspn, c, R, M)
    assert_equal(got, want)
    assert sum(w["valid"] for w in want) > 0


def test_ragged_counts_and_fewer_candidates_than_topk(tspn, device):
    """All-NaN heads -> count 0 for those pairs; segment 1 keeps one pair only, so its candidates (<= J R = 8) are fewer
    than M = 40: `valid` says so and the tail keeps the sentinel."""
    S, N, T, D, K, J, R, M = 2, 3, 8, 16, 8, 2, 4, 40
    c = make_case(device, S, N, T, D, K, J, seed=7)
    P = c["P"]
    heads = c["heads"].clone()
    heads[1] = float("nan")
    heads[P + 1:] = float("nan")
    with_spans(tspn, c, heads)
    count = c["count"].cpu().numpy()
    assert count[1] == 0 and (count[P + 1:] == 0).all() and count[P] > 0 and (count[:P] > 0).sum() == P - 1
    got = fused(tspn, c, R, M)
    want, _ = composition(tspn, c, R, M)
    assert_equal(got, want)
    assert int(got[5][1]) == int(count[P]) * R < M and int(got[5][0]) == min(M, int(count[:P].sum()) * R)
    assert not (got[2][0, :int(got[5][0])] == np.array([0, 2])).all(axis=1).any()        # pair 1 = (0, 2) has no span
    # no proposal anywhere: nothing is written but valid = 0
    with_spans(tspn, c, torch.full_like(heads, float("nan")))
    got = fused(tspn, c, R, M)
    assert (got[5] == 0).all() and (got[0].view(np.int32) == SENT_F_BITS).all() and (got[4] == SENT_I).all()


def direct_spans(c, rows, scores=None):
    """The same J span rows (and scores) for every pair, all counted."""
    dev = c["feats"].device
    SP, J = c["S"] * c["P"], c["J"]
    sp = torch.tensor(rows, dtype=torch.int64).view(1, J, 2).repeat(SP, 1, 1).contiguous()
    sc = torch.tensor(scores if scores is not None else [0.9 - 0.1 * j for j in range(J)], dtype=torch.float32)
    c["spans"], c["score"] = sp.to(dev), sc.view(1, J).repeat(SP, 1).contiguous().to(dev)
    c["count"] = torch.full((SP,), J, dtype=torch.int64, device=dev)
    return c


def test_duplicated_tracklets_tie_by_flat_index(tspn, device):
    """Tracklets 0, 1 and 2 are copies with equal spans and span scores: the candidates of pairs (0,3), (1,3), (2,3)
    tie exactly; the lower flat index ((p J + j) R + r) wins, also where the tie straddles the M-th place."""
    S, N, T, D, K, J, R = 1, 4, 6, 16, 12, 2, 3
    c = make_case(device, S, N, T, D, K, J, seed=21)
    c["feats"][1] = c["feats"][0]
    c["feats"][2] = c["feats"][0]
    direct_spans(c, [(0, 4), (2, 6)], scores=[0.75, 0.75])
    full, _ = composition(tspn, c, R, 1024)
    sc = full[0]["scores"]
    ties = [m for m in range(1, len(sc)) if sc[m] == sc[m - 1]]
    assert len(ties) >= 6
    for M in (1024, ties[0], ties[2], ties[-1], 1):                 # cut inside runs of equal scores
        assert_equal(fused(tspn, c, R, M), composition(tspn, c, R, M)[0])


def test_custom_pair_table_with_repeated_and_reversed_pairs(tspn, device):
    pairs = torch.tensor([[0, 1], [1, 0], [0, 1], [2, 0], [0, 1], [2, 2]], dtype=torch.int64)
    c = with_spans(tspn, make_case(device, 2, 3, 9, 16, 20, 3, seed=33, pairs=pairs))
    c["pairs"][1] = c["pairs"][1].flip(0)                            # another table in the second segment
    got = fused(tspn, c, 5, 60)
    assert_equal(got, composition(tspn, c, 5, 60)[0])
    with pytest.raises(IndexError):
        bad = dict(c, pairs=c["pairs"].clone())
        bad["pairs"][0, 0, 0] = 3
        fused(tspn, bad, 5, 60)


def test_spans_given_directly_with_rewritten_rows(tspn, device):
    """Rows `decode_spans` never writes inside the count: (-1, -1) (whole segment), empty, reversed, past the end,
    straddling the end.  The pooled value follows span pooling's row rewrite; the row comes back as it was given."""
    S, N, T, D, K, J, R, M = 2, 3, 7, 16, 10, 6, 4, 200
    c = make_case(device, S, N, T, D, K, J, seed=44)
    rows = [(-1, -1), (3, 3), (5, 2), (T + 2, T + 9), (2, T + 5), (1, 4)]
    direct_spans(c, rows)
    c["count"][2] = 3                                                # only the first three rows of pair 2
    got = fused(tspn, c, R, M)
    assert_equal(got, composition(tspn, c, R, M)[0])
    v = int(got[5][0])
    assert v == (c["P"] * J - 3) * R and {tuple(r) for r in got[3][0, :v].tolist()} == set(rows)


def test_nonfinite_frames_rank_first_and_stay_in_their_spans(tspn, device):
    """A NaN in one frame of tracklet 1 and a +Inf in one frame of tracklet 2: the candidates whose span holds the NaN
    frame score NaN and lead the segment (torch's sort order: equality with the composition); every candidate that
    does not touch either frame has the bits of a clean launch."""
    S, N, T, D, K, J, R = 1, 4, 10, 16, 9, 2, 5
    c = with_spans(tspn, make_case(device, S, N, T, D, K, J, seed=55))
    Q = c["P"] * J * R
    clean = fused(tspn, c, R, 1024)
    assert int(clean[5][0]) <= Q <= 1024
    key = lambda a, m: (tuple(a[2][0, m]), int(a[4][0, m]), int(a[1][0, m, 1]))   # noqa: E731
    clean_bits = {key(clean, m): int(clean[0][0, m:m + 1].view(np.int32)[0]) for m in range(int(clean[5][0]))}
    planted = {1: 4, 2: 7}                                           # tracklet -> frame
    c["feats"][1, 4, 3] = float("nan")
    c["feats"][2, 7, 5] = float("inf")
    for M in (1024, 17):
        got = fused(tspn, c, R, M)
        assert_equal(got, composition(tspn, c, R, M)[0])
        v = int(got[5][0])
        touched = np.zeros(v, dtype=bool)
        nan_touched = np.zeros(v, dtype=bool)
        for m in range(v):
            a, e = got[3][0, m]
            for trk, frame in planted.items():
                if trk in got[2][0, m] and a <= frame < e:
                    touched[m] = True
                    nan_touched[m] |= trk == 1
        is_nan = np.isnan(got[0][0, :v])
        assert nan_touched.any() and np.array_equal(is_nan, nan_touched)
        assert is_nan[:is_nan.sum()].all()                           # NaN above everything else
        if M == 1024:
            assert (~touched).any()
            for m in np.nonzero(~touched)[0]:
                assert clean_bits[key(got, m)] == int(got[0][0, m:m + 1].view(np.int32)[0])


def test_refusals_leave_the_outputs_untouched(tspn, device):
    """K = 257, topk_per_seg = 1025, J = 17 -> TSPN_EUNSUPPORTED; a workspace one byte short -> TSPN_EWORKSPACE; a null
    pointer -> TSPN_EINVAL.  Nothing is launched: the sentinels stay."""
    A = tspn._abi
    lib = A.lib()
    c = with_spans(tspn, make_case(device, 1, 3, 6, 16, 8, 2, seed=66))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    need = lib.tspn_decode_span_relations_workspace_bytes(1, 3, 6, 16, c["P"], 2, 8, 4)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K=8, J=2, M=16, ws_bytes=need, feats=None):
        out = sentinel_out(c, 4, 16, device)
        rc = lib.tspn_decode_span_relations_f32(p(c["feats"]) if feats is None else feats, 1, 3, 6, 16, p(c["pairs"]), c["P"],
                                                p(c["spans"]), p(c["score"]), p(c["count"]), J, p(c["w"]), p(c["b"]), K,
                                                p(c["cls"]), 35, 4, M, *[p(t) for t in out], p(ws), ws_bytes, stream)
        torch.cuda.synchronize()
        if rc != A.TSPN_OK:
            assert (out[0].view(torch.int32) == SENT_F_BITS).all() and all(bool((o == SENT_I).all()) for o in out[1:])
        return rc, lib.tspn_last_error().decode()

    assert call()[0] == A.TSPN_OK
    rc, msg = call(K=257)
    assert rc == A.TSPN_EUNSUPPORTED and "K=257" in msg
    rc, msg = call(M=1025)
    assert rc == A.TSPN_EUNSUPPORTED and "topk_per_seg=1025" in msg
    rc, msg = call(J=17)
    assert rc == A.TSPN_EUNSUPPORTED and "J=17" in msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc == A.TSPN_EWORKSPACE and "workspace" in msg
    rc, msg = call(feats=ctypes.c_void_p(0))
    assert rc == A.TSPN_EINVAL and "null pointer" in msg
    with pytest.raises(tspn._abi.TspnError):
        tspn.ops.decode_span_relations(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["w"], c["b"],
                                       c["cls"], topk_per_seg=1025)


# ------------------------------------------------------------------------------------------------ through the model
def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def temporal_model(tspn, D):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": True, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D})
    sd = tspn.synth.make_weights(0, c=2 * D, bias_std=0.05)
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.eval()


def plist_of(tspn, seed, n, tt, D, **kw):
    v = tspn.synth.make_video(seed, n, tt, D)
    return tspn.PairList.from_tracklets(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), t(v["track_cls_logits"]), **kw)


def test_model_decode_span_relations_batches_equal_shapes(tspn, device):
    """Three equal-shape videos (one launch), an odd-shaped one, one with a custom pair table and one with a single
    tracklet: the same as one call per video; spans inside [0, T]; every span is one of its pair's `count` proposals."""
    D, J = 24, 3
    model = temporal_model(tspn, D)
    custom = torch.tensor([[1, 0], [0, 1], [1, 0], [2, 3]], dtype=torch.int64)
    plists = [plist_of(tspn, 80, 5, 20, D), plist_of(tspn, 81, 4, 13, D), plist_of(tspn, 82, 5, 20, D),
              plist_of(tspn, 83, 5, 20, D), plist_of(tspn, 84, 4, 13, D, tracklet_pairs=custom), plist_of(tspn, 85, 1, 20, D)]
    _, dp, _ = model(plists, None)
    kw = dict(spans_per_pair=J, topk_per_span=6, topk_per_seg=50)
    got = model.decode_span_relations(plists, dp, **kw)
    spans = model.decode_spans(dp[:5], top_k=J)
    for i, (pl, g) in enumerate(zip(plists, got)):
        one = model.decode_span_relations([pl], [dp[i]], **kw)[0]
        assert len(g) == 4 and all(torch.equal(a, b) and a.device.type == "cpu" for a, b in zip(g, one))
        if i == 5:
            assert [tuple(a.shape) for a in g] == [(0,), (0, 3), (0, 2), (0, 2)]
            continue
        sc, trip, tid, sp = g
        tt = pl.get_field("tracklet_feats").shape[1]
        assert 0 < sc.shape[0] <= 50 and (sc[:-1] >= sc[1:]).all()
        assert (sp[:, 0] >= 0).all() and (sp[:, 0] < sp[:, 1]).all() and (sp[:, 1] <= tt).all()
        table = custom if i == 4 else all_pairs(pl.get_field("tracklet_feats").shape[0])
        for m in range(sc.shape[0]):
            rows = [r for r in range(table.shape[0]) if torch.equal(table[r], tid[m])]
            assert rows and any(any(torch.equal(spans[i]["span"][r, j], sp[m]) for j in range(int(spans[i]["count"][r])))
                                for r in rows)
        cls = pl.get_field("track_cls_logits").argmax(dim=1)
        assert torch.equal(trip[:, 0], cls[tid[:, 0]]) and torch.equal(trip[:, 2], cls[tid[:, 1]])


def test_predict_associate_evaluate_with_spans(tspn, device):
    """predict_short_term_relations(spans_per_pair=2) -> greedy_relational_association -> evaluation.evaluate on a
    two-segment video: durations inside the union of the segments, trajectories as long as their durations; with
    spans_per_pair=0 the function returns what its loop returned before span mode (restated here)."""
    D, n, tt = 24, 4, 30
    model = temporal_model(tspn, D)
    index = [("v0", 0, 30), ("v0", 15, 45)]
    vids = [tspn.synth.make_video(90 + i, n, tt, D) for i in range(2)]
    plists = [tspn.PairList.from_tracklets(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), t(v["track_cls_logits"])) for v in vids]
    loader = [(plists, None, index)]
    rel = tspn.predict.predict_short_term_relations(model, loader, topk_per_pair=5, topk_per_seg=40, spans_per_pair=2)
    assert sorted(rel) == index
    for preds, _, _ in rel.values():
        assert 0 < len(preds) <= 40 and all(len(p) == 4 and 0 <= p[3][0] < p[3][1] <= tt for p in preds)
    trajs = {ix: v["tracklet_boxes"].astype(np.float64) for ix, v in zip(index, vids)}
    out = tspn.association.greedy_relational_association(None, list(rel.items()), trajectories=trajs)
    assert out
    for r in out:
        b, e = r["duration"]
        assert 0 <= b < e <= 45 and len(r["sub_traj"]) == e - b and len(r["obj_traj"]) == e - b
    gt = {"v0": [dict(out[0], triplet=list(out[0]["triplet"])), dict(out[-1])]}
    mean_ap, rec, prec = tspn.evaluation.evaluate(gt, {"v0": out})
    assert 0 < mean_ap <= 1 and rec[50] > 0
    # spans_per_pair = 0: today's structure, value for value
    base = tspn.predict.predict_short_term_relations(model, loader, topk_per_pair=5, topk_per_seg=40)
    with torch.no_grad():
        _, _, logits = model(plists, None)
        dec = model.decode(plists, logits, topk_per_pair=5, topk_per_seg=40)
    assert sorted(base) == index
    for ix, (score, trip, tid) in zip(index, dec):
        preds, iou, trackid = base[ix]
        want = [(np.array(s), np.array(a), np.array(b)) for s, a, b in zip(score.numpy(), trip.numpy(), tid.numpy())]
        assert len(preds) == len(want) and iou.shape == (0, 0) and trackid.shape == (0,)
        for p, w in zip(preds, want):
            assert type(p) is tuple and len(p) == 3
            assert all(type(a) is np.ndarray and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
                       for a, b in zip(p, w))
