"""The bf16 pair-list stage on the GPU (csrc/pairlist/): arbitrary [P,2] pair tables on the bf16-operand path.

Inputs follow tests/test_gpu_bf16.py (hashrng: y std 1, head weights bf16-rounded std 0.1, H = 12), so its bound carries
over: the kernel differs from a float64 evaluation of the same bf16 operands by fp32 accumulation order only,
atol = 3e-5.  Against the grid kernel the requirement is equality of bits: same channel order, same fragment positions,
one accumulator."""
import numpy as np
import pytest
import torch

import oracle
import pairlist_reference as ref
from sentinel_buffers import SENTINEL
from test_gpu_bf16 import check_against_oracle, oracle_weights, r16, t, temporal_cfg
from test_gpu_nonfinite import assert_same_nonfinite

pytestmark = pytest.mark.gpu

H = 12
ATOL = 3e-5


def operands(tspn, B, N, T, C):
    y = t(tspn.hashrng.normal(83, "y", (B * N, T, 2 * C), std=1.0))
    hw = r16(tspn.hashrng.normal(83, "hw", (H, C), std=0.1))
    hb = t(tspn.hashrng.normal(83, "hb", (H,), std=0.1))
    return y, hw, hb


def run_list(tspn, device, y, pairs, B, N, hw, hb, **kw):
    pairs = torch.as_tensor(np.asarray(pairs), dtype=torch.int64).reshape(-1, 2).to(device)
    return tspn.ops.heads_pairlist_bf16(y.to(device), pairs, B, N, tspn.ops.pack_heads_bf16(hw.to(device)), hb.to(device), H,
                                        **kw)


def canonical_row(pairs, N):
    """Row of the canonical table that holds (s, o), global ids."""
    pairs = np.asarray(pairs)
    b, s, o = pairs[:, 0] // N, pairs[:, 0] % N, pairs[:, 1] % N
    return b * N * (N - 1) + s * (N - 1) + np.where(o < s, o, o - 1)


# ------------------------------------------------------------------------------------------------ equality with the grid
GRID_SHAPES = [(1, 2, 1, 32), (2, 5, 30, 64), (1, 11, 37, 96), (1, 17, 20, 32), (3, 9, 150, 64)]
_grid = {}


def grid_rows(tspn, device, shape):
    if shape not in _grid:
        B, N, T, C = shape
        y, hw, hb = operands(tspn, *shape)
        _grid[shape] = tspn.ops.heads_pairgrid_bf16(y.to(device), B, N, tspn.ops.pack_heads_bf16(hw.to(device)),
                                                    hb.to(device), H).cpu()
    return _grid[shape]


@pytest.mark.parametrize("order", ["canonical", "shuffled"])
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_list_rows_equal_the_grid_rows(tspn, device, shape, order):
    """Both forms (<4,8,2> for N <= 12, <8,16,2> above), T % 16 != 0, compact extents of 1, 11 and 17 slots: the
    canonical table passed as a list, in its own order and with its rows shuffled across videos."""
    B, N, T, C = shape
    y, hw, hb = operands(tspn, *shape)
    table = ref.canonical_table(B, N)
    if order == "shuffled":
        table = table[np.random.RandomState(7).permutation(len(table))]
    out = run_list(tspn, device, y, table, B, N, hw, hb).cpu()
    want = grid_rows(tspn, device, shape)[torch.from_numpy(canonical_row(table, N))]
    assert out.shape == want.shape == (B * N * (N - 1), H, T)
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ arbitrary tables
TABLES, SCATTERED17 = ref.TABLES, ref.SCATTERED17


@pytest.mark.parametrize("name", list(TABLES))
def test_arbitrary_tables_vs_fp64(tspn, device, name):
    B, N, T, C, table = TABLES[name]
    y, hw, hb = operands(tspn, B, N, T, C)
    out = run_list(tspn, device, y, table, B, N, hw, hb)
    torch.cuda.synchronize(device)                    # P = 0 included: no launch error is left behind
    want = ref.heads_list_ref64(y, table, hw, hb)
    assert out.shape == want.shape == (len(table), H, T) and out.dtype == torch.float32
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=0, atol=ATOL)


@pytest.mark.parametrize("name", list(TABLES) + ["cross_video_and_out_of_range_rows"])
def test_plan_equals_the_numpy_restatement(tspn, device, name):
    if name in TABLES:
        B, N, _, _, table = TABLES[name]
    else:
        B, N, table = ref.CROSS_VIDEO
    plan = tspn.ops.pair_plan(torch.as_tensor(table, dtype=torch.int64).reshape(-1, 2).to(device), B, N)
    assert all(v.dtype == torch.int32 for v in plan.values())
    ref.check_plan({k: v.cpu().numpy() for k, v in plan.items()}, table, B, N)


# ------------------------------------------------------------------------------------------------ extent of the stores
def test_stores_cover_the_given_rows_and_nothing_else(tspn, device):
    B, N, T, C, table = TABLES["among_17_scattered_of_40"]
    P = len(table)
    y, hw, hb = operands(tspn, B, N, T, C)
    buf = torch.full((P + 1, H, T), SENTINEL, dtype=torch.float32, device=device)
    out = run_list(tspn, device, y, table, B, N, hw, hb, out=buf[:P])
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu()
    assert bool((got[P] == SENTINEL).all()), "wrote past the last row"
    assert int((got[:P] == SENTINEL).sum()) == 0, "rows not fully written"
    np.testing.assert_allclose(got[:P].numpy(), ref.heads_list_ref64(y, table, hw, hb).numpy(), rtol=0, atol=ATOL)


def test_a_cross_video_row_is_skipped_and_keeps_its_output_row(tspn, device):
    B, N, T, C = 2, 5, 18, 32
    table = np.concatenate([ref.among([0, 2, 3]), [[1, 7]], ref.among([1, 4], base=5)])        # row 6 joins two videos
    P, bad = len(table), 6
    y, hw, hb = operands(tspn, B, N, T, C)
    with pytest.raises(IndexError):
        run_list(tspn, device, y, table, B, N, hw, hb)
    buf = torch.full((P + 1, H, T), SENTINEL, dtype=torch.float32, device=device)
    run_list(tspn, device, y, table, B, N, hw, hb, out=buf[:P], check_pairs=False)
    got = buf.cpu()
    assert bool((got[bad] == SENTINEL).all()) and bool((got[P] == SENTINEL).all())
    keep = [p for p in range(P) if p != bad]
    np.testing.assert_allclose(got[keep].numpy(), ref.heads_list_ref64(y, table[keep], hw, hb).numpy(), rtol=0, atol=ATOL)


def test_two_launches_agree_bit_for_bit(tspn, device):
    """The plan links its chains with atomics: their order may differ from launch to launch, the result may not."""
    B, N, T, C, table = TABLES["every_row_three_times"]
    y, hw, hb = operands(tspn, B, N, T, C)
    a = run_list(tspn, device, y, table, B, N, hw, hb)
    b = run_list(tspn, device, y, table, B, N, hw, hb)
    assert torch.equal(a, b)
    B, N, T, C, table = TABLES["among_17_scattered_of_40"]
    y, hw, hb = operands(tspn, B, N, T, C)
    assert torch.equal(run_list(tspn, device, y, table, B, N, hw, hb), run_list(tspn, device, y, table, B, N, hw, hb))


# ------------------------------------------------------------------------------------------------ confinement
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_activation_stays_in_its_subject_rows_and_frame(tspn, device, value):
    B, N, T, C = 1, 9, 20, 32
    s, frame, chan = 4, 13, 21                                    # U half: channel < C
    table = np.concatenate([ref.among([1, 4, 6, 8]), [[4, 4], [4, 1], [0, 4], [2, 2]], ref.among([4, 6])])
    y, hw, hb = operands(tspn, B, N, T, C)
    assert bool((hw[:, chan] != 0).all())                         # Inf * w is +-Inf for every head
    clean = run_list(tspn, device, y, table, B, N, hw, hb).cpu()
    y = y.clone()
    y[s, frame, chan] = value
    got = run_list(tspn, device, y, table, B, N, hw, hb).cpu()
    assert_same_nonfinite(got.numpy(), ref.heads_list_ref64(y, table, hw, hb).numpy(), ATOL, "planted " + str(value))
    hit = torch.zeros(got.shape, dtype=torch.bool)
    hit[torch.from_numpy(table[:, 0] == s), :, frame] = True
    assert int(hit.sum()) > 0 and torch.equal(~torch.isfinite(got), hit)
    assert torch.equal(got[~hit], clean[~hit])


# ------------------------------------------------------------------------------------------------ argument checks
def test_operands_the_entries_cannot_take_are_unsupported(tspn, device):
    ops, abi = tspn.ops, tspn._abi
    B, N, T, C = 1, 5, 18, 32
    y, hw, hb = operands(tspn, B, N, T, C)
    y, hb = y.to(device), hb.to(device)
    hp = ops.pack_heads_bf16(hw.to(device))
    pairs = torch.tensor([[0, 1], [3, 2]], dtype=torch.int64, device=device)

    def unsupported(fn):
        with pytest.raises(abi.TspnError) as e:
            fn()
        assert e.value.code == abi.TSPN_EUNSUPPORTED, e.value

    unsupported(lambda: ops.heads_pairlist_bf16(y.double(), pairs, B, N, hp, hb, H))                    # dtype
    unsupported(lambda: ops.heads_pairlist_bf16(y, pairs.int(), B, N, hp, hb, H))
    unsupported(lambda: ops.heads_pairlist_bf16(y, pairs, B, N, hp.float(), hb, H))
    unsupported(lambda: ops.heads_pairlist_bf16(y.cpu(), pairs, B, N, hp, hb, H))                       # device
    unsupported(lambda: ops.heads_pairlist_bf16(y, pairs.cpu(), B, N, hp, hb, H))
    unsupported(lambda: ops.pair_plan(pairs.cpu(), B, N))
    unsupported(lambda: ops.pair_plan(pairs.int(), B, N))
    wide = torch.zeros((2, 3), dtype=torch.int64, device=device)
    unsupported(lambda: ops.heads_pairlist_bf16(y, wide[:, :2], B, N, hp, hb, H))                       # layout
    unsupported(lambda: ops.pair_plan(wide[:, :2], B, N))
    unsupported(lambda: ops.heads_pairlist_bf16(y.transpose(0, 1), pairs, B, N, hp, hb, H))
    unsupported(lambda: ops.heads_pairlist_bf16(y[:, :, :2 * C - 4].contiguous(), pairs, B, N, hp, hb, H))   # ld < 2C
    base = torch.zeros(y.numel() + 1, dtype=torch.float32, device=device)
    off = base[1:].view(y.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    unsupported(lambda: ops.heads_pairlist_bf16(off, pairs, B, N, hp, hb, H))                           # misaligned y
    big = torch.zeros((2049, 1, 2 * C), dtype=torch.float32, device=device)
    unsupported(lambda: ops.heads_pairlist_bf16(big, pairs, 1, 2049, hp, hb, H))                        # N = 2049
    unsupported(lambda: ops.pair_plan(pairs, 1, 2049))
    ok = ops.heads_pairlist_bf16(big[:2048], pairs, 1, 2048, hp, hb, H)                                  # the limit itself
    assert ok.shape == (2, H, 1) and bool(torch.isfinite(ok).all())


# ------------------------------------------------------------------------------------------------ the fused pass
def test_forward_fused_bf16_on_a_pair_table(tspn, device):
    """N = 16, T = 150, D = 128 on a 60-row table (a scattered subset with repeated rows): heads equal the same rows of the
    canonical call bit for bit; logits within 2^-8 of the fp32 path on the rounded operands, as in
    test_forward_fused_bf16_matches_fp32_path_on_rounded_operands."""
    N, T, D = 16, 150, 128
    C = 2 * D
    v = tspn.synth.make_video(95, N, T, D)
    sd = tspn.synth.make_weights(0, c=C, bias_std=0.05)
    w = {k: r16(x.numpy()).to(device) for k, x in oracle_weights(sd).items()}
    feats = r16(v["tracklet_feats"]).to(device)
    canon = tspn.ops.pair_index(N, device)
    rs = np.random.RandomState(5)
    rows = rs.permutation(N * (N - 1))[:50]
    rows = rs.permutation(np.concatenate([rows, rows[:10]]))
    table = canon[torch.from_numpy(rows).to(device)].contiguous()
    assert table.shape == (60, 2)
    hw = torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]).contiguous()
    hb = torch.cat([w["rel_b"], w["dur_b"]]).contiguous()
    args = (tspn.ops.pack_conv3_bf16(w["conv_w"], split=D), w["conv_b"], tspn.ops.pack_heads_bf16(hw), hb, w["cls_w"], w["cls_b"])
    h_can, _ = tspn.ops.forward_fused_bf16(feats.to(torch.bfloat16), canon, 1, N, *args)
    h, l = tspn.ops.forward_fused_bf16(feats.to(torch.bfloat16), table, 1, N, *args, canonical_pairs=False)
    assert h.shape == (60, 12, T) and l.shape == (60, 132)
    assert torch.equal(h, h_can[torch.from_numpy(rows).to(device)])
    _, l32 = tspn.ops.forward_fused(feats, canon, 1, N, tspn.ops.pack_conv3(w["conv_w"], split=D), w["conv_b"],
                                    hw, hb, w["cls_w"], w["cls_b"], canonical_pairs=True)
    assert float((l - l32[torch.from_numpy(rows).to(device)]).abs().max()) <= 2.0 ** -8
    with pytest.raises(ValueError, match="canonical pair table"):
        tspn.ops.forward_fused_bf16(feats.to(torch.bfloat16), table, 1, N, *args)          # the default is unchanged
    with pytest.raises(IndexError):
        tspn.ops.forward_fused_bf16(feats.to(torch.bfloat16), table + 1, 1, N, *args, canonical_pairs=False)


# ------------------------------------------------------------------------------------------------ the model
def test_model_forward_bf16_with_tracklet_pairs_vs_oracle(tspn, device):
    """BaseModel.forward on bf16 PairLists (6,30), (9,17), (6,30): the first and the third carry different
    'tracklet_pairs' (duplicates in one, a scattered subset in the other), the second none."""
    D = 32
    sd = tspn.synth.make_weights(0, c=2 * D, bias_std=0.05)
    model = tspn.BaseModel(temporal_cfg(D))
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    model.eval()
    shapes = [(6, 30), (9, 17), (6, 30)]
    tables = [torch.tensor([[0, 1], [4, 2], [0, 1], [5, 0], [4, 2], [4, 2], [1, 0]], dtype=torch.int64), None,
              torch.tensor([[5, 3], [0, 3], [3, 5], [2, 0]], dtype=torch.int64)]
    vids = [tspn.synth.make_video(90 + i, n, tt, D) for i, (n, tt) in enumerate(shapes)]
    plists = [tspn.PairList.from_tracklets(t(v["tracklet_feats"]).to(torch.bfloat16), t(v["tracklet_boxes"]),
                                           t(v["track_cls_logits"]), tracklet_pairs=tab) for v, tab in zip(vids, tables)]
    pp, dp, logits = model(plists, None)
    w = oracle_weights(sd)
    for i, v in enumerate(vids):
        n, tt = shapes[i]
        pairs = oracle.pair_index(n) if tables[i] is None else tables[i]
        want = oracle.forward_bf16(t(v["tracklet_feats"]), pairs, w)
        P = pairs.shape[0]
        assert dp[i].relness.dtype == torch.float32 and dp[i].relness.shape == want["relness"].shape
        assert dp[i].relness.shape[0] == P and dp[i].duration.shape[0] == P and logits[i].shape == (P, 132)
        check_against_oracle(dp[i].relness, want["relness"], f"relness {i}")
        check_against_oracle(dp[i].duration, want["duration"], f"duration {i}")
        check_against_oracle(logits[i], want["rel_logits"], f"rel_logits {i}")
    dec = model.decode(plists, logits, topk_per_pair=5, topk_per_seg=40)
    assert len(dec) == 3
    for score, trip, tid in dec:
        assert score.shape[0] == trip.shape[0] == tid.shape[0] > 0 and trip.shape[1] == 3 and tid.shape[1] == 2
