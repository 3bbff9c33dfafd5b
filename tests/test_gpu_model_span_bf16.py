"""Spans on bf16 segments through BaseModel: RELPN.DPN.POOL_TOP_SPAN in `forward`, `classify_spans` and
`decode_span_relations` (DESIGN.md §2 "bf16 semantics").  D = 32, n = 7, T = 30, weights from synth.make_weights
(unrounded: the packing rounds them)."""
import numpy as np
import pytest
import torch

import cases
import oracle
import span_bf16_reference as ref

pytestmark = pytest.mark.gpu

D, N, T = 32, 7, 30


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def temporal_model(tspn, sd, pool_top_span, use_ppn=False):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": use_ppn, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D})
    cfg.RELPN.DPN.POOL_TOP_SPAN = pool_top_span
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.eval()


def video16(tspn, seed, n=N, tt=T):
    """A synthetic video whose features are bf16 values (kept in fp32 here)."""
    v = tspn.synth.make_video(seed, n, tt, D)
    v["tracklet_feats"] = ref.bf16(v["tracklet_feats"])
    return v


def plist16(tspn, v, device, **kw):
    return tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(torch.bfloat16).to(device), t(v["tracklet_boxes"]).to(device),
                                        t(v["track_cls_logits"]).to(device), **kw)


def test_pool_top_span_forward_on_bf16_segments(tspn, device):
    """Three equal-shape bf16 videos (one fused pass, the canonical table) and a fourth segment with its own
    'tracklet_pairs' (a shuffled subset with a duplicate row: the pair-list stage): per segment the logits are the
    restatement pooled over the spans oracle.decode_spans picks from the returned heads.  The third video holds an
    all-NaN tracklet: its pairs have no proposal (-1 -> the whole segment -> NaN logits), no other pair is touched."""
    sd = tspn.synth.make_weights(0, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, sd, True)
    vids = [video16(tspn, 860 + k) for k in range(4)]
    vids[2]["tracklet_feats"][4] = np.nan
    allp = oracle.pair_index(N).numpy()
    rs = np.random.RandomState(5)
    custom = allp[rs.permutation(len(allp))[:17]]
    custom = np.concatenate([custom, custom[3:4]])                     # a duplicate row
    tables = [allp, allp, allp, custom]
    pls = [plist16(tspn, v, device, **({"tracklet_pairs": t(custom)} if k == 3 else {})) for k, v in enumerate(vids)]
    _, dp, lg = model(pls, None)
    w, b = sd["classifier.rel_predictor.weight"], sd["classifier.rel_predictor.bias"]
    for k, v in enumerate(vids):
        pairs = tables[k]
        assert tuple(lg[k].shape) == (len(pairs), w.shape[0])
        sp = oracle.decode_spans(dp[k].relness.cpu(), dp[k].duration.cpu(), model.anchor_sizes(T), top_k=1)["span"][:, 0]
        sp = sp.numpy()
        np.testing.assert_array_equal(model.decode_spans([dp[k]], top_k=1)[0]["span"][:, 0].cpu().numpy(), sp)
        r, z, S, frames = ref.span_predicate_ref(v["tracklet_feats"], pairs, sp, w, b)
        no_proposal = (pairs == 4).any(axis=1) if k == 2 else np.zeros(len(pairs), bool)
        assert ((sp == -1).all(axis=1) == no_proposal).all()
        assert np.isnan(z[no_proposal]).all() and np.isfinite(z[~no_proposal]).all()
        assert (frames[~no_proposal, 1] - frames[~no_proposal, 0] < T).any()       # real spans, not the whole segment
        ref.check_against_ref(lg[k].cpu().numpy(), r, z, S, D, f"POOL_TOP_SPAN bf16 segment {k}")


def test_classify_spans_on_a_bf16_segment_equals_forward(tspn, device):
    """classify_spans on the spans forward pooled over gives forward's POOL_TOP_SPAN logits bit for bit; a (-1, -1) row
    pools the whole segment; a bf16 segment with D % 16 != 0 raises forward's ValueError."""
    sd = tspn.synth.make_weights(1, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, sd, True)
    v = video16(tspn, 870)
    pl = plist16(tspn, v, device)
    _, dp, lg = model([pl], None)
    sp = model.decode_spans(dp, top_k=1)[0]["span"][:, 0]
    got = model.classify_spans([pl], [sp])[0]
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), lg[0].view(torch.int32))
    sp2 = sp.clone()
    sp2[3] = -1
    got2 = model.classify_spans([pl], [sp2])[0].cpu().numpy()
    pairs = oracle.pair_index(N).numpy()
    w, b = sd["classifier.rel_predictor.weight"], sd["classifier.rel_predictor.bias"]
    r, z, S, frames = ref.span_predicate_ref(v["tracklet_feats"], pairs, sp2.cpu().numpy(), w, b)
    assert frames[3].tolist() == [0, T]
    ref.check_against_ref(got2, r, z, S, D, "classify_spans bf16")
    keep = np.arange(len(pairs)) != 3
    assert np.array_equal(got2[keep].view(np.uint32), got.cpu().numpy()[keep].view(np.uint32))
    odd = tspn.PairList.from_tracklets(torch.zeros((3, 5, 24), dtype=torch.bfloat16, device=device),
                                       torch.zeros((3, 5, 4), device=device), torch.zeros((3, 35), device=device))
    with pytest.raises(ValueError, match="D % 16 == 0"):
        model.classify_spans([odd], [torch.zeros((6, 2), dtype=torch.int64)])


def test_decode_span_relations_on_bf16_segments(tspn, device):
    """A batch of three bf16 segments (one launch) gives per segment exactly what a call on that segment alone gives; a
    mixed list of one fp32 and one bf16 segment of equal shape is grouped apart, and the fp32 one is bit-identical to a
    call without the bf16 neighbour."""
    sd = tspn.synth.make_weights(2, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, sd, False, use_ppn=True)
    vids = [video16(tspn, 880 + k) for k in range(3)]
    pls = [plist16(tspn, v, device) for v in vids]
    _, dp, _ = model(pls, None)
    kw = dict(spans_per_pair=3, topk_per_span=6, topk_per_seg=50)
    got = model.decode_span_relations(pls, dp, **kw)
    for i, g in enumerate(got):
        one = model.decode_span_relations([pls[i]], [dp[i]], **kw)[0]
        assert len(g) == 4 and 0 < g[0].shape[0] <= 50 and all(torch.equal(a, b) for a, b in zip(g, one))
        assert torch.equal(g[0].view(torch.int32), one[0].view(torch.int32))
        assert (g[0][:-1] >= g[0][1:]).all() and (g[3][:, 0] < g[3][:, 1]).all() and (g[3][:, 1] <= T).all()
    # the same video as fp32 and as bf16, side by side
    v = vids[0]
    pl32 = tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(device), t(v["tracklet_boxes"]).to(device),
                                        t(v["track_cls_logits"]).to(device))
    _, dp32, _ = model([pl32], None)
    alone = model.decode_span_relations([pl32], dp32, **kw)[0]
    mixed = model.decode_span_relations([pl32, pls[0]], [dp32[0], dp[0]], **kw)
    assert all(torch.equal(a, b) for a, b in zip(mixed[0], alone))
    assert torch.equal(mixed[0][0].view(torch.int32), alone[0].view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(mixed[1], got[0]))
