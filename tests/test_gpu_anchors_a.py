"""RELPN.DPN.NUM_ANCHORS_PER_LOCATION off 4: the fused bf16 entries with A in {1, 3, 5} (H = 3A = 3, 9, 15 heads) and
BaseModel with A in {1, 5} on one bf16 and one fp32 segment.

References and bounds are the ones these paths already have at A = 4: `oracle.forward_bf16` at `check_against_oracle`'s
bound (tests/test_gpu_bf16.py) for bf16 operands, `oracle.forward_dense` at atol = 1e-5 for fp32 ones
(test_random_shapes_fp32_and_bf16_paths_vs_oracle); rows of an arbitrary table equal the canonical call's rows bit for
bit (test_forward_fused_bf16_on_a_pair_table).  The oracle and `synth.make_weights` take A from the weights' shapes."""
import numpy as np
import pytest
import torch

import cases
import oracle
import pairlist_reference as ref
from test_gpu_bf16 import check_against_oracle, oracle_weights, r16, t

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("A", [1, 3, 5])
def test_forward_fused_bf16_canonical_and_pair_table_off_four_anchors(tspn, device, A):
    """B = 2, N = 20, D = 32, T = 37.  The table has unequal axes (9 subjects x 3 objects in video 0, 4 x 11 in video 1),
    repeated rows, and its rows shuffled across the videos."""
    B, N, T, D, K = 2, 20, 37, 32, 132
    C = 2 * D
    sd = tspn.synth.make_weights(0, c=C, a=A, bias_std=0.05)
    w_host = {k: r16(x.numpy()) for k, x in oracle_weights(sd).items()}
    assert w_host["rel_w"].shape == (A, C, 1) and w_host["dur_w"].shape == (2 * A, C, 1)
    w = {k: x.to(device) for k, x in w_host.items()}
    vids = [r16(tspn.synth.make_video(95 + b, N, T, D)["tracklet_feats"]) for b in range(B)]
    feats = torch.cat(vids).to(device).to(torch.bfloat16)
    hw = torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]).contiguous()
    hb = torch.cat([w["rel_b"], w["dur_b"]]).contiguous()
    args = (tspn.ops.pack_conv3_bf16(w["conv_w"], split=D), w["conv_b"], tspn.ops.pack_heads_bf16(hw), hb, w["cls_w"], w["cls_b"])
    canon = torch.cat([tspn.ops.pair_index(N, device, base=b * N) for b in range(B)])
    h_can, l_can = tspn.ops.forward_fused_bf16(feats, canon, B, N, *args)
    P1 = N * (N - 1)
    assert h_can.shape == (B * P1, 3 * A, T) and l_can.shape == (B * P1, K)
    want = [oracle.forward_bf16(v, oracle.pair_index(N), w_host) for v in vids]
    for b in range(B):
        sl = slice(b * P1, (b + 1) * P1)
        assert want[b]["relness"].shape == (P1, A, T) and want[b]["duration"].shape == (P1, 2 * A, T)
        check_against_oracle(h_can[sl, :A].cpu(), want[b]["relness"], f"relness A={A} video {b}")
        check_against_oracle(h_can[sl, A:].cpu(), want[b]["duration"], f"duration A={A} video {b}")
        check_against_oracle(l_can[sl].cpu(), want[b]["rel_logits"], f"rel_logits A={A} video {b}")

    table = np.concatenate([ref.cross([0, 1, 4, 6, 9, 12, 15, 18, 19], [2, 9, 17]),
                            ref.cross([3, 5, 16, 19], [0, 1, 2, 5, 7, 8, 11, 13, 14, 16, 18], base=N)])
    table = table[table[:, 0] != table[:, 1]]
    table = np.concatenate([table, table[::4]])
    table = table[np.random.RandomState(A).permutation(len(table))]
    b_, s_, o_ = table[:, 0] // N, table[:, 0] % N, table[:, 1] % N
    rows = torch.from_numpy(b_ * P1 + s_ * (N - 1) + np.where(o_ < s_, o_, o_ - 1))
    assert torch.equal(canon.cpu()[rows], torch.from_numpy(table))
    h, l = tspn.ops.forward_fused_bf16(feats, torch.from_numpy(table).to(device), B, N, *args, canonical_pairs=False)
    assert h.shape == (len(table), 3 * A, T) and l.shape == (len(table), K)
    assert torch.equal(h.cpu(), h_can.cpu()[rows])
    for b in range(B):
        m = torch.from_numpy(b_ == b)
        local = rows[m] - b * P1
        check_against_oracle(h[m.to(device), :A].cpu(), want[b]["relness"][local], f"table relness A={A} video {b}")
        check_against_oracle(h[m.to(device), A:].cpu(), want[b]["duration"][local], f"table duration A={A} video {b}")
        check_against_oracle(l[m.to(device)].cpu(), want[b]["rel_logits"][local], f"table rel_logits A={A} video {b}")


@pytest.mark.parametrize("A", [1, 5])
def test_model_with_one_and_five_anchors_per_location(tspn, device, A):
    """BaseModel on an fp32 and a bf16 segment (different N and T): relness [P,A,T] and duration [P,2A,T] (the [:A] /
    [A:] split of DPN._wrap) against the oracle, and both span decodes run on them."""
    D = 32
    sd = tspn.synth.make_weights(0, c=2 * D, a=A, bias_std=0.05)
    model = tspn.BaseModel(cases.baseline_cfg(**{"RELPN.USE_PPN": True, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                                 "PREDICT.FEATURE_DIM": 2 * D, "RELPN.DPN.NUM_ANCHORS_PER_LOCATION": A}))
    assert model.relpn.duration_proposal_network.dpn_head.num_windows == A
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    model.eval()
    w = oracle_weights(sd)
    spec = [(6, 30, torch.float32), (9, 17, torch.bfloat16)]
    vids = [tspn.synth.make_video(90 + i, n, tt, D) for i, (n, tt, _) in enumerate(spec)]
    plists = [tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(dt).to(device), t(v["tracklet_boxes"]).to(device),
                                           (8.0 * t(v["track_cls_logits"])).to(device))
              for v, (_, _, dt) in zip(vids, spec)]
    _, dp, logits = model(plists, None)
    for i, (v, (n, tt, dt)) in enumerate(zip(vids, spec)):
        P = n * (n - 1)
        assert dp[i].relness.shape == (P, A, tt) and dp[i].duration.shape == (P, 2 * A, tt)
        assert dp[i].heads.shape == (P, 3 * A, tt) and logits[i].shape == (P, 132)
        got = {"relness": dp[i].relness.cpu(), "duration": dp[i].duration.cpu(), "rel_logits": logits[i].cpu()}
        if dt == torch.float32:
            want = oracle.forward_dense(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), oracle.pair_index(n), w)
            for key, val in got.items():
                np.testing.assert_allclose(val.numpy(), want[key].numpy(), rtol=0, atol=1e-5, err_msg=f"{key} A={A}")
        else:
            want = oracle.forward_bf16(t(v["tracklet_feats"]), oracle.pair_index(n), w)
            for key, val in got.items():
                check_against_oracle(val, want[key], f"{key} A={A}")
    spans = model.decode_spans(dp, top_k=4)
    rel = model.decode_span_relations(plists, dp, spans_per_pair=3, topk_per_span=6, topk_per_seg=50)
    for i, (n, tt, _) in enumerate(spec):
        sp, cnt = spans[i]["span"].cpu(), spans[i]["count"].cpu()
        assert sp.shape == (n * (n - 1), 4, 2) and int(cnt.min()) >= 1 and int(cnt.max()) <= 4
        ok = sp[..., 0] >= 0
        anchor = spans[i]["anchor"].cpu()[ok]
        assert bool((anchor >= 0).all()) and bool((anchor < A * tt).all())            # one of the A * T candidates
        assert bool((sp[..., 1][ok] <= tt).all()) and bool((sp[..., 0][ok] < sp[..., 1][ok]).all())
        score, trip, tid, rsp = (x.cpu() for x in rel[i])
        assert score.shape[0] == trip.shape[0] == tid.shape[0] == rsp.shape[0] > 0
        assert bool((rsp[:, 0] >= 0).all()) and bool((rsp[:, 1] <= tt).all()) and bool((rsp[:, 0] < rsp[:, 1]).all())
