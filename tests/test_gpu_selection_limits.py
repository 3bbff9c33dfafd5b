"""The kernels that turn scores into the answer, at their capacity limits, each against its CPU oracle:

* `tspn::select_topk_sorted` with more than 65 536 candidates (the upper index bytes of its tie-break passes), through
  `ops.decode_topk` (oracle.decode_topk) and `ops.decode_span_relations` (the composition of
  tests/span_relations_reference.py);
* `pair_topk_kernel` at every register slot and lane edge (K = 1 ... 256, topk_per_pair = 1 ... K);
* `decode_spans_kernel` at A = 8, A*T = 4096, top_k = 1024, pre_nms on the 64-bit word edges of the suppression matrix,
  thresholds 0 and 1, degenerate spans (oracle.decode_spans);
* `ppn_kernel` at the largest N its LDS holds (oracle.ppn_pair_matrix / ppn_topk);
* `traj_iou_kernel` in its batched cross form and on the box cases where the reference does not clip (oracle.cubic_iou).

Indices, counts, integer spans, span_f and the decoded scores are compared for exact equality (scores by their bits);
the two numeric bounds are the suite's own (PPN matrix atol 2e-6, sigmoid span score atol 1e-7, non-integer IoU
rtol 2e-6 / atol 1e-7: tests/test_gpu_ops.py)."""
import functools

import numpy as np
import pytest
import torch

import cases
import oracle
import test_gpu_span_relations as sr

pytestmark = pytest.mark.gpu

PPN_PRE = "relpn.pair_proposal_network.ppn_head."


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def assert_bits(got, want, msg=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, msg
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), msg


def unsupported(tspn, fn, *words):
    with pytest.raises(tspn._abi.TspnError) as e:
        fn()
    assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED, str(e.value)
    assert all(w in str(e.value) for w in words), str(e.value)


# ----------------------------------------------------- a. select_topk_sorted past 65 536 candidates, via decode_topk
BIG_N, BIG_K, BIG_KP = 65, 24, 20
BIG_P = BIG_N * (BIG_N - 1)                         # 4160 pairs -> Q = P * topk_per_pair = 83 200 candidates


@functools.lru_cache(maxsize=None)
def big_inputs(kind):
    """One segment [P, K] of logits, the classeme feature [P, 75] and the pair table.
    step<p0>: rows below p0 all -1, the rest all +1: every candidate from flat index 20 p0 on ties, the winners are the
    first topk_per_seg of them.  random: quantised to sixteenths (ties at both levels).  random_high: the same with the
    rows below 3300 lowered by 2, so every winner has a flat index above 65 536."""
    if kind.startswith("step"):
        logit = np.full((BIG_P, BIG_K), -1.0, np.float32)
        logit[int(kind[4:]):] = 1.0
    else:
        logit = (np.round(tspn_hash().uniform(161, "big", (BIG_P, BIG_K)) * 16) / 16).astype(np.float32)
        logit[:, 3] = 1.0
        if kind == "random_high":
            logit[:3300] -= 2.0
    feat = tspn_hash().uniform(161, "bigfeat", (BIG_P, 75))
    feat[:, 2] = feat[:, 9]
    return logit, feat, cases.ref_pairs(BIG_N)


def tspn_hash():
    import tspn_mi355x
    return tspn_mi355x.hashrng


@functools.lru_cache(maxsize=None)
def big_reference(kind):
    """oracle.decode_topk at topk_per_seg = 1024; a stable sort's first m rows are its answer for topk_per_seg = m."""
    logit, feat, pairs = big_inputs(kind)
    return tuple(x.numpy() for x in oracle.decode_topk(t(logit), t(feat[:, :70]), t(pairs), BIG_N, BIG_KP, 1024))


def run_big(tspn, device, kinds, ks):
    ins = [big_inputs(k) for k in kinds]
    logit, feat, pairs = (t(np.stack([i[j] for i in ins])).to(device) for j in range(3))
    got = tspn.ops.decode_topk(logit, pairs, feat, row_mul=BIG_N - 1, topk_per_pair=BIG_KP, topk_per_seg=ks)
    got = [g.cpu().numpy() for g in got]
    assert got[0].shape == (len(kinds), ks)
    for s, kind in enumerate(kinds):
        ref = big_reference(kind)
        assert_bits(got[0][s], ref[0][:ks], f"{kind}: scores")
        np.testing.assert_array_equal(got[1][s], ref[1][:ks], err_msg=f"{kind}: triplets")
        np.testing.assert_array_equal(got[2][s], ref[2][:ks], err_msg=f"{kind}: pair ids")
    return got


@pytest.mark.parametrize("p0,first", [(3400, 68000), (3270, 65400)])
def test_select_ties_in_the_upper_index_bytes(tspn, device, p0, first):
    """83 200 candidates, the 1024 winners all tie: flat indices 68 000 ... 69 023 (byte 2 of the index is 1 for all of
    them) and 65 400 ... 66 423 (the tied run straddles 65 536: two buckets are live in that pass)."""
    got = run_big(tspn, device, [f"step{p0}"], 1024)
    flat = np.arange(first, first + 1024)
    pairs = cases.ref_pairs(BIG_N)
    np.testing.assert_array_equal(got[2][0], pairs[flat // BIG_KP])
    np.testing.assert_array_equal(got[1][0][:, 1], flat % BIG_KP)
    assert (got[0][0] == 1.0).all()


@pytest.mark.parametrize("kind", ["random", "random_high"])
@pytest.mark.parametrize("ks", [1, 1023, 1024])
def test_select_quantised_scores_at_83200_candidates(tspn, device, kind, ks):
    run_big(tspn, device, [kind], ks)


def test_select_keeps_no_state_between_segments(tspn, device):
    """Two workgroups, the two tie constructions in either order: each segment's answer is its own."""
    run_big(tspn, device, ["step3270", "step3400"], 1024)
    run_big(tspn, device, ["step3400", "step3270"], 1024)
    run_big(tspn, device, ["random_high", "step3400"], 1023)


# ------------------------------------------------ b. the same select through decode_span_relations (Q = 95 232)
def span_ties_case(tspn, device):
    """N = 32 copies of one tracklet, J = 16 equal span rows per pair, all counted: q[p, j, k] depends on k only.  Span
    score 0.25 for the pairs below 700, 0.75 for the rest: the candidates from flat index 700 J R = 67 200 on tie in
    runs of (P - 700) J = 4672, and the cut at M = 1024 falls inside the first run."""
    S, N, T, D, K, J = 1, 32, 6, 16, 8, 16
    c = sr.make_case(device, S, N, T, D, K, J, seed=171)
    c["feats"][:] = c["feats"][0].clone()
    sr.direct_spans(c, [(1, 5)] * J, scores=[0.75] * J)
    c["score"][:700] = 0.25
    return c


def test_span_relations_ties_above_65536_candidates(tspn, device):
    c = span_ties_case(tspn, device)
    P, J, R = c["P"], c["J"], 6
    assert P * J * R == 95232
    want, q = sr.composition(tspn, c, R, 1024)
    assert bool((q == q[0]).all())                                   # every row the same: ties by construction
    for M in (1024, 1000):
        got = sr.fused(tspn, c, R, M)
        sr.assert_equal(got, sr.composition(tspn, c, R, M)[0])
        flat = (got[2][0, :, 0] * (c["N"] - 1) + got[2][0, :, 1] - (got[2][0, :, 1] > got[2][0, :, 0])) * J + got[4][0]
        assert np.array_equal(flat, 700 * J + np.arange(M))          # rows 11 200 ... : flat index 67 200 + 6 i
    assert want[0]["valid"] == 1024


@pytest.mark.parametrize("first_counted", [700, 990])
def test_span_relations_uncounted_pairs_fill_the_low_indices(tspn, device, first_counted):
    """count = 0 below pair 700 (990): key-0 rows hold every flat index below 67 200 (95 040) and none is selected.
    `valid` is min(topk_per_seg, real candidates): 1024 of (P - 700) J R = 28 032, and all (P - 990) J R = 192."""
    c = span_ties_case(tspn, device)
    P, J, R, M = c["P"], c["J"], 6, 1024
    c["count"][:first_counted] = 0
    real = (P - first_counted) * J * R
    assert int(c["count"].sum()) * R == real
    got = sr.fused(tspn, c, R, M)
    want = sr.composition(tspn, c, R, M)[0]
    sr.assert_equal(got, want)
    v = int(got[5][0])
    assert v == min(M, real) == want[0]["valid"]
    first = cases.ref_pairs(c["N"])[first_counted]
    assert (got[2][0, :v, 0] * c["N"] + got[2][0, :v, 1] >= first[0] * c["N"] + first[1]).all()


# --------------------------------------------------------- c. pair_topk_kernel: register slots and lane edges
def edge_logits(tspn, S, P, K):
    logit = (np.round(tspn.hashrng.uniform(162, f"edge{K}", (S, P, K)) * 16) / 16).astype(np.float32)
    for s in range(S):
        for p in range(P):
            if K == 1:
                if (s * P + p) % 3 < 2:
                    logit[s, p, 0] = (np.nan, -np.inf)[(s * P + p) % 3]
                continue
            a = (5 * (s * P + p) + 1) % K
            logit[s, p, a] = np.nan
            logit[s, p, (a + 1 + p % (K - 1)) % K] = -np.inf
    logit[S - 1, 5] = 0.5                                            # one all-equal row: pure index order
    return logit


@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 129, 192, 193, 255, 256])
def test_decode_topk_register_and_lane_edges(tspn, device, K):
    """One to four values per lane with the last lane of a slot and the first of the next one; topk_per_pair = 1, K
    (every arg-max round) and K + 7 (clamped to K); a NaN and a -Inf in every row; topk_per_seg = 1024 keeps every
    candidate up to K = 85 and cuts the list above."""
    S, N = 2, 4
    P = N * (N - 1)
    logit = edge_logits(tspn, S, P, K)
    feat = tspn.hashrng.uniform(162, "feat", (S, P, 75))
    feat[:, :, 2] = feat[:, :, 9]
    pairs = np.stack([cases.ref_pairs(N)] * S)
    for kp in (1, K, K + 7):
        sc, trip, tids = tspn.ops.decode_topk(t(logit).to(device), t(pairs).to(device), t(feat).to(device),
                                              row_mul=N - 1, topk_per_pair=kp, topk_per_seg=1024)
        assert sc.shape == (S, min(1024, P * min(kp, K)))
        for s in range(S):
            rs, rt, ri = oracle.decode_topk(t(logit[s]), t(feat[s, :, :70]), t(pairs[s]), N, kp, 1024)
            assert_bits(sc[s].cpu().numpy(), rs.numpy(), f"kp={kp} segment {s}: scores")
            np.testing.assert_array_equal(trip[s].cpu().numpy(), rt.numpy(), err_msg=f"kp={kp} segment {s}")
            np.testing.assert_array_equal(tids[s].cpu().numpy(), ri.numpy(), err_msg=f"kp={kp} segment {s}")


def test_decode_topk_refusals(tspn, device):
    N, P = 4, 12
    pairs = t(cases.ref_pairs(N)[None]).to(device)
    feat = torch.zeros(1, P, 75, device=device)
    unsupported(tspn, lambda: tspn.ops.decode_topk(torch.zeros(1, P, 257, device=device), pairs, feat, row_mul=N - 1), "K=257")
    unsupported(tspn, lambda: tspn.ops.decode_topk(torch.zeros(1, P, 128, device=device), pairs, feat, row_mul=N - 1,
                                                   topk_per_pair=128, topk_per_seg=1025), "topk_seg=1025")


# ------------------------------------------------------------------------------ d. decode_spans at its limits
SIZES = [4.0, 8.0, 16.0, 32.0, 64.0, 96.0, 128.0, 192.0]


def span_heads(tspn, P, A, T, seed=163):
    heads = tspn.hashrng.normal(seed, f"spans{A}x{T}", (P, 3 * A, T), std=1.0)
    heads[:, :A] = np.round(heads[:, :A] * 8) / 8                    # quantised logits -> exact ties
    heads[:, A:] *= 0.4
    return heads


def check_spans(tspn, device, heads, sizes, **kw):
    A = len(sizes)
    got = {k: v.cpu().numpy() for k, v in tspn.ops.decode_spans(t(heads).to(device), sizes, **kw).items()}
    ref = {k: v.numpy() for k, v in oracle.decode_spans(t(heads[:, :A]), t(heads[:, A:]), sizes, **kw).items()}
    for k in ("count", "anchor", "span"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k} {kw}")
    assert_bits(got["span_f"], ref["span_f"], f"span_f {kw}")
    np.testing.assert_allclose(got["score"], ref["score"], rtol=0, atol=1e-7, err_msg=f"score {kw}")
    for p, n in enumerate(got["count"]):                             # the filler behind the survivors
        assert (got["anchor"][p, n:] == -1).all() and (got["span"][p, n:] == -1).all()
        assert (got["span_f"][p, n:] == 0).all() and (got["score"][p, n:] == 0).all()
    return got


@pytest.mark.parametrize("A,T", [(8, 512), (4, 1024), (8, 8), (5, 30), (7, 33)])
def test_decode_spans_shapes_and_thresholds(tspn, device, A, T):
    """A*T = 4096 twice (the sort has no padding; A = 8 fills SpanSizes), n = 64, two ragged shapes.  Threshold 0.5,
    0 (every overlapping later span goes) and 1 with top_k = 1024 (nothing is suppressed: min(A*T, 1024) survivors, the
    last slot of the kept list included)."""
    heads = span_heads(tspn, 3, A, T)
    if T > 4:
        heads[0, A + 1, 3] = 9.0                                     # d_w above the clamp
    check_spans(tspn, device, heads, SIZES[:A], top_k=64, nms_threshold=0.5)
    check_spans(tspn, device, heads, SIZES[:A], top_k=64, nms_threshold=0.0)
    got = check_spans(tspn, device, heads, SIZES[:A], top_k=1024, nms_threshold=1.0)
    assert (got["count"] == min(A * T, 1024)).all()


@pytest.mark.parametrize("pre_nms", [1, 63, 64, 65, 128, 129, 149, 150])
def test_decode_spans_pre_nms_at_the_mask_word_edges(tspn, device, pre_nms):
    """n = 150 candidates; pre_nms on either side of the 64-bit words of the suppression matrix, 1, n - 1 and n; top_k
    below and above pre_nms; at threshold 1 the count is min(top_k, pre_nms) exactly."""
    A, T = 5, 30
    heads = span_heads(tspn, 4, A, T)
    for top_k in (max(1, pre_nms // 2), pre_nms + 3):
        check_spans(tspn, device, heads, SIZES[:A], top_k=top_k, nms_threshold=0.5, pre_nms=pre_nms)
        check_spans(tspn, device, heads, SIZES[:A], top_k=top_k, nms_threshold=0.0, pre_nms=pre_nms)
        got = check_spans(tspn, device, heads, SIZES[:A], top_k=top_k, nms_threshold=1.0, pre_nms=pre_nms)
        assert (got["count"] == min(top_k, pre_nms)).all()


def test_decode_spans_degenerate_pairs_among_ordinary_ones(tspn, device):
    """Pair 1: d_c = 0 and d_w = +Inf (clamped): every candidate is clipped to [0, T], one span, count 1 at 0.5.
    Pair 2: d_w = -Inf: zero-width spans, every union with another zero-width span is 0.  Pair 4: all logits equal.
    Pairs 0, 3, 5 are ordinary."""
    A, T = 5, 30
    heads = span_heads(tspn, 6, A, T)
    heads[1, A:] = 0.0
    heads[1, A + 1::2] = np.inf
    heads[2, A + 1::2] = -np.inf
    heads[4, :A] = 0.375
    for thr in (0.5, 0.0, 1.0):
        got = check_spans(tspn, device, heads, SIZES[:A], top_k=200, nms_threshold=thr)
        assert got["count"][1] == (150 if thr == 1.0 else 1)
        assert (got["span"][1, :got["count"][1]] == (0, T)).all()
        assert (got["span_f"][2, :, 0] == got["span_f"][2, :, 1]).all()
    # the same with one size only: zero regressions and a width of 4 T clip every candidate to [0, T]
    heads1 = span_heads(tspn, 3, 1, T, seed=164)
    heads1[1, 1:] = 0.0
    got = check_spans(tspn, device, heads1, [4.0 * T], top_k=64, nms_threshold=0.5)
    assert got["count"][1] == 1 and tuple(got["span"][1, 0]) == (0, T)


def test_decode_spans_more_workgroups_than_compute_units(tspn, device):
    heads = span_heads(tspn, 300, 3, 17)
    check_spans(tspn, device, heads, SIZES[:3], top_k=8, nms_threshold=0.5)


def test_decode_spans_refusals(tspn, device):
    z = lambda *s: torch.zeros(*s, device=device)   # noqa: E731
    unsupported(tspn, lambda: tspn.ops.decode_spans(z(1, 27, 4), [1.0] * 9), "A=9")
    unsupported(tspn, lambda: tspn.ops.decode_spans(z(1, 3, 4097), [4.0]), "A*T=4097")
    unsupported(tspn, lambda: tspn.ops.decode_spans(z(1, 3, 40), [4.0], top_k=1025), "top_k=1025")


# ----------------------------------------------------------------------- e. ppn_pair_matrix_topk at its capacity
def ppn_case(tspn, device, ppn, B, N):
    sd = tspn.synth.make_weights(3, c=8, ppn=ppn, bias_std=0.1)
    w_np = {k[len(PPN_PRE):]: v for k, v in sd.items() if k.startswith(PPN_PRE)}
    cls = 6.0 * tspn.hashrng.uniform(165, f"cls{N}", (B, N, 35))
    cls[:, N // 2] = cls[:, 0]                                       # duplicate tracklet -> exact ties in the matrix
    if N > 8:
        cls[:, N - 1] = cls[:, 3]
    return cls, w_np, {k: t(v).to(device) for k, v in w_np.items()}


@pytest.mark.parametrize("ppn,B,N", [((35, 64, 35), 1, 1), ((35, 64, 35), 2, 2), ((35, 64, 35), 3, 90),
                                     ((35, 8, 8), 1, 91), ((35, 8, 8), 2, 128)],
                         ids=["model-N1", "model-N2", "model-N90xB3", "narrow-N91", "narrow-N128"])
def test_ppn_at_its_lds_capacity(tspn, device, ppn, B, N):
    """The model's widths (35, 64, 35) up to N = 90 (126 376 B of LDS, three such workgroups side by side) and N = 1,
    where the sort loops do not run; embeddings of 8 at N = 91 (n2p = 16 384, nearly half of it padding) and N = 128
    (161 280 B; N*N = 16 384 is a power of two: no padding).  topk 0, 1, 256 and N*N."""
    cls, w_np, w = ppn_case(tspn, device, ppn, B, N)
    refs = [oracle.ppn_pair_matrix(t(cls[b]), {k: t(v) for k, v in w_np.items()}).numpy() for b in range(B)]
    for topk in (0, 1, 256, N * N):
        mat, idx = tspn.ops.ppn_pair_matrix_topk(t(cls).to(device), w, topk)
        k = min(topk, N * N)
        assert mat.shape == (B, N, N) and idx.shape == (B, k) and idx.dtype == torch.int64
        for b in range(B):
            np.testing.assert_allclose(mat[b].cpu().numpy(), refs[b], rtol=0, atol=2e-6)
            # the stable descending order of the device's own matrix (the suite's tie rule)
            np.testing.assert_array_equal(idx[b].cpu().numpy(), oracle.ppn_topk(mat[b].cpu(), k).numpy())
            assert mat[b, N // 2, 0] == mat[b, 0, 0]                 # the ties are there


def test_ppn_refuses_what_lds_cannot_hold(tspn, device):
    """At the model's widths N = 91 needs 4*91*169 + 8*16 384 = 192 588 B: refused, and the message names LDS."""
    cls, _, w = ppn_case(tspn, device, (35, 64, 35), 1, 91)
    unsupported(tspn, lambda: tspn.ops.ppn_pair_matrix_topk(t(cls).to(device), w, 256), "LDS", "192588")


# --------------------------------------------------------------------------------- f. traj_iou shapes and boxes
def random_boxes(tspn, tag, shape):
    xy = tspn.hashrng.uniform(166, tag + "xy", shape + (2,), 0, 500)
    wh = tspn.hashrng.uniform(166, tag + "wh", shape + (2,), 1, 200)
    return np.concatenate([xy, xy + wh], -1).astype(np.float32)


def iou_ref(b1, b2=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        return oracle.cubic_iou(b1, b2)


@pytest.mark.parametrize("B,N1,N2,T", [(3, 17, 31, 5), (2, 6, 9, 1), (1, 1, 300, 7), (2, 300, 1, 3)])
def test_traj_iou_cross_shapes(tspn, device, B, N1, N2, T):
    """Cross form with other boxes in every batch entry (a wrong batch stride of either operand fails), N1 != N2,
    527 = 2 * 256 + 15 outputs, one frame, one row, one column."""
    b1, b2 = random_boxes(tspn, "a", (B, N1, T)), random_boxes(tspn, "b", (B, N2, T))
    got = tspn.ops.traj_iou(t(b1).to(device), t(b2).to(device)).cpu().numpy()
    assert got.shape == (B, N1, N2)
    for b in range(B):
        np.testing.assert_allclose(got[b], iou_ref(b1[b], b2[b]), rtol=2e-6, atol=1e-7)
    one = tspn.ops.traj_iou(t(b1[B - 1]).to(device), t(b2[B - 1]).to(device)).cpu().numpy()   # 3-D operands
    assert_bits(one, got[B - 1])


def test_traj_iou_self_form(tspn, device):
    b = random_boxes(tspn, "s", (2, 23, 11))
    got = tspn.ops.traj_iou(t(b).to(device)).cpu().numpy()
    for i in range(2):
        np.testing.assert_allclose(got[i], iou_ref(b[i]), rtol=2e-6, atol=1e-7)
    assert_bits(got, tspn.ops.traj_iou(t(b).to(device), t(b).to(device)).cpu().numpy())


@pytest.mark.parametrize("N1,N2", [(0, 5), (5, 0), (0, 0)])
def test_traj_iou_empty_operands(tspn, device, N1, N2):
    b1, b2 = torch.zeros(2, N1, 4, 4, device=device), torch.zeros(2, N2, 4, 4, device=device)
    got = tspn.ops.traj_iou(b1, b2)
    assert got.shape == (2, N1, N2) and got.dtype == torch.float32 and got.device == b1.device
    if N1 == 0:
        assert tspn.ops.traj_iou(b1).shape == (2, 0, 0)


def assert_iou_bits(got, ref):
    """The oracle's float32 bits; NaN (0 / 0, whose sign is the divider's business) where it has NaN."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), ref))


def test_traj_iou_integer_boxes_bit_exact(tspn, device):
    """Integer coordinates <= 64 and T = 30: every fp32 sum stays below 2^24, so the result is the oracle's to the
    bit in any summation order.  Rows 0/1 identical (IoU exactly 1), row 2 disjoint from everything (exactly 0), row 3
    with x2 < x1 - 1 in every frame (negative area, which the reference does not clip), rows 4/5 of zero width
    (area 0: their unions are 0 and the IoU is NaN), row 6 whose area cancels row 7's (union 0 with a non-zero
    intersection with others), row 8 with x2 < x1 - 1 in its first ten frames only (their negative areas shrink the
    union: its IoU with itself is above 1)."""
    B, N, T = 2, 12, 30
    lo = tspn.hashrng.integers(167, "lo", (B, N, T, 2), 0, 24)
    wh = tspn.hashrng.integers(167, "wh", (B, N, T, 2), 0, 16)
    b = np.concatenate([lo, lo + wh], -1).astype(np.float32)
    b[:, 1] = b[:, 0]
    b[:, 2, :, 0::2] += 40                                           # x in [40, 79] - 15: beyond every other box
    b[:, 2] = np.minimum(b[:, 2], 64)
    b[:, 3, :, 2] = b[:, 3, :, 0] - 3
    b[:, 4, :, 2] = b[:, 4, :, 0] - 1
    b[:, 5, :, 2] = b[:, 5, :, 0] - 1
    b[:, 6] = (2, 2, 5, 5)                                           # area 16 per frame
    b[:, 7] = (9, 2, 4, 5)                                           # width 4 - 9 + 1 = -4: area -16 per frame
    b[:, 8, :10, 2] = b[:, 8, :10, 0] - 3
    assert b.max() <= 64 and b.min() >= -3
    got = tspn.ops.traj_iou(t(b).to(device)).cpu().numpy()
    cross = tspn.ops.traj_iou(t(b[:, :5]).to(device), t(b[:, 3:]).to(device)).cpu().numpy()
    for i in range(B):
        ref = iou_ref(b[i])
        assert_iou_bits(got[i], ref)
        assert_iou_bits(cross[i], iou_ref(b[i, :5], b[i, 3:]))
        assert ref[0, 1] == 1.0 and ref[0, 0] == 1.0 and got[i, 1, 0] == 1.0
        assert (ref[2, [0, 1, 3, 4, 5, 6, 7]] == 0).all() and (got[i, 2, [0, 1, 6]] == 0).all()
        assert ref[3, 3] == 0 and np.signbit(ref[3, 3])              # 0 over a negative union, kept as it is
        assert ref[8, 8] > 1
        assert np.isnan(ref[4, 5]) and np.isnan(ref[4, 4]) and np.isnan(ref[6, 7])
