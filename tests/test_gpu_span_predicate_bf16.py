"""Span-restricted RelOIPool + predicate head on bf16 segments (`tspn_span_predicate_bf16`: span_prefix_bf16_kernel,
span_pool_bf16_kernel, span_gemm_bf16_kernel; DESIGN.md §2 "bf16 semantics", §4c) against the float64 restatement of
tests/span_bf16_reference.py.

Tolerance of the GEMM tests (derived in span_bf16_reference): |got - ref| <= 0.25 c eps S + 4 eps with eps = 2^-24,
S = the span mean of sum_c |f||w16| over both halves and c = min(2D/32 + 33, 2D + 2): a product is rounded at most 32
times inside its v_mfma_f32_16x16x32_bf16 (31 adds among the 32 products of the k-step, one onto the accumulator), once by
each of the 2D/32 - 1 later k-steps and once by the bias add; one more unit covers |pooled| <= (1 + 2^-8) mean|f|.  The
pooled operand itself is pinned to the bit through an identity classifier."""
import numpy as np
import pytest
import torch

import oracle
import span_bf16_reference as ref
from test_gpu_span_predicate import all_pairs_with_self, bits

pytestmark = pytest.mark.gpu

EPS = ref.EPS


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def dev16(f, device):
    return t(f).to(torch.bfloat16).to(device)


def launch(tspn, device, f, pairs, spans, w, b):
    ops = tspn.ops
    K = w.shape[0]
    packed = ops.pack_span_cls_bf16(t(w).to(device))
    return ops.span_predicate_bf16(dev16(f, device), t(pairs).to(device), t(spans).to(device), packed,
                                   None if b is None else t(b).to(device), K).cpu().numpy()


def run_case(tspn, device, what, f, pairs, spans, w, b):
    got = launch(tspn, device, f, pairs, spans, w, b)
    r, z, S, frames = ref.span_predicate_ref(f, pairs, spans, w, b)
    ref.check_against_ref(got, r, z, S, f.shape[2], what)
    return got, (r, z, S, frames)


# ------------------------------------------------------------------------------------------------ the pooled operand
@pytest.mark.parametrize("NT,T,D", [(5, 37, 16), (3, 1, 48), (4, 150, 32)])
def test_pooling_pinned_through_an_identity_classifier(tspn, device, NT, T, D):
    """K = 2D, W = I (exact in bf16), no bias: z[p, c] is the pooled element itself, the only fp32 work is the sigmoid.
    A wrong frame range, a sum rounded to fp32 or a bf16 operand one ulp off is 10^3 times the bound."""
    rs, f, _, _ = ref.make_operands(800 + T, NT, T, D, 1)
    pairs = all_pairs_with_self(NT, 40)
    spans = ref.draw_spans(rs, len(pairs), T)
    w = np.eye(2 * D, dtype=np.float32)
    got = launch(tspn, device, f, pairs, spans, w, None).astype(np.float64)
    pooled = ref.pooled_rows(f, pairs, spans).astype(np.float64)
    want = 1.0 / (1.0 + np.exp(-pooled))
    err = np.abs(got - want).max()
    print(f"identity classifier NT={NT} T={T} D={D}: max |got - sigmoid(pooled)| = {err:.3g} (bound {4 * EPS:.3g})")
    assert got.shape == (len(pairs), 2 * D) and err <= 4 * EPS


# ------------------------------------------------------------------------------------------------ the GEMM
# (P, K, D, T): the granularities of span_gemm_bf16_kernel (tests/spanbf16_kernel_variants.py) are 16 rows per wave, 64
# rows per workgroup, 16 columns per tile, 64 columns per workgroup (1 to 4 tiles: four code paths), 32 of the 2D
# channels per k-step (D % 16 == 0: D = 16 is one k-step, D = 48 three), groups of 4 k-steps loaded together (D = 48, 64, 80:
# 3, 4, 5 k-steps; D = 128, 144: 8, 9)
GEMM_CASES = ([(P, 132, 48, 7) for P in (1, 15, 16, 17, 33, 63, 64, 65, 130)] +
              [(33, K, 16, 5) for K in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 132, 145, 260)] +
              [(33, 17, D, 6) for D in (16, 32, 48, 64, 80, 128, 144)] + [(33, 17, 1040, 3)])


@pytest.mark.parametrize("P,K,D,T", GEMM_CASES, ids=["x".join(map(str, c)) for c in GEMM_CASES])
def test_gemm_against_float64(tspn, device, P, K, D, T):
    NT = 5
    rs, f, w, b = ref.make_operands(810 + P + K + D, NT, T, D, K)
    pairs = all_pairs_with_self(NT, P)[:P]
    pairs = pairs[rs.permutation(P)]
    run_case(tspn, device, f"P={P} K={K} D={D} T={T}", f, pairs, ref.spans_for(rs, P, T), w, b)


def test_one_tracklet_pairs_with_itself(tspn, device):
    rs, f, w, b = ref.make_operands(820, 1, 9, 16, 5)
    pairs = all_pairs_with_self(1, 40)
    assert (pairs == 0).all()
    run_case(tspn, device, "NT=1", f, pairs, ref.draw_spans(rs, len(pairs), 9), w, b)


def test_no_rows_and_no_tracklets_launch_nothing(tspn, device):
    ops = tspn.ops
    packed = ops.pack_span_cls_bf16(torch.zeros(5, 32, device=device))
    i64 = dict(dtype=torch.int64, device=device)
    out = ops.span_predicate_bf16(torch.zeros((3, 4, 16), dtype=torch.bfloat16, device=device), torch.zeros((0, 2), **i64),
                                  torch.zeros((0, 2), **i64), packed, None, 5)
    assert tuple(out.shape) == (0, 5)
    out = ops.span_predicate_bf16(torch.zeros((0, 4, 16), dtype=torch.bfloat16, device=device), torch.zeros((0, 2), **i64),
                                  torch.zeros((0, 2), **i64), packed, None, 5)
    assert tuple(out.shape) == (0, 5)
    with pytest.raises(IndexError):
        ops.span_predicate_bf16(torch.zeros((3, 4, 16), dtype=torch.bfloat16, device=device),
                                torch.tensor([[0, 3]], **i64), torch.zeros((1, 2), **i64), packed, None, 5)
    with pytest.raises(ValueError, match="D % 16"):
        ops.pack_span_cls_bf16(torch.zeros(5, 48, device=device))


def fused_bf16_logits(tspn, device, f, pairs, B, N, w, b):
    """rel_logits of ops.forward_fused_bf16 on the same features, table and predicate head (the encoder's weights are
    zero: the logits do not depend on them)."""
    ops = tspn.ops
    D = f.shape[2]
    C = 2 * D
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)   # noqa: E731
    packed = ops.pack_conv3_bf16(z(C, C, 3), split=D)
    hpk = ops.pack_heads_bf16(z(3, C))
    return ops.forward_fused_bf16(dev16(f, device), t(pairs).to(device), B, N, packed, z(C), hpk, z(3),
                                  t(ref.bf16(w)).to(device), t(ref.bf16(b)).to(device), canonical_pairs=False)[1].cpu().numpy()


def link_to_fused(tspn, device, what, f, pairs, B, N, w, b, got, r, z, S, frames):
    """Whole-segment rows against the fused bf16 pass: it takes the segment mean in fp32 (temporal_mean_bf16_kernel), so
    a pooled element may land one bf16 ulp (2^-8 relative, 2^-7 as a bound on both sides of a tie) away; if every one
    did, the value before the sigmoid would move by 2^-7 S.  A consistency link, not the accuracy test."""
    T, D = f.shape[1], f.shape[2]
    rows = np.flatnonzero((frames[:, 0] == 0) & (frames[:, 1] == T))
    assert rows.size >= 8
    lg = fused_bf16_logits(tspn, device, f, pairs, B, N, w, b).astype(np.float64)
    tol = 0.25 * 2.0 ** -7 * S + ref.tolerance(S, D)
    err = (np.abs(lg - got) / tol)[rows].max()
    print(f"{what}: whole-segment rows against the fused bf16 pass: {err:.3f} of the tolerance")
    assert err <= 1.0


def test_four_videos_global_ids_shuffled_table(tspn, device):
    """Four videos in one call, as forward() batches them: global tracklet ids, the in-video pairs in shuffled order."""
    B, N, T, D, K = 4, 8, 30, 64, 132
    rs, f, w, b = ref.make_operands(830, B * N, T, D, K)
    pairs = np.concatenate([oracle.pair_index(N).numpy() + v * N for v in range(B)])
    pairs = pairs[rs.permutation(len(pairs))]
    spans = ref.draw_spans(rs, len(pairs), T)
    got, (r, z, S, frames) = run_case(tspn, device, "4 videos", f, pairs, spans, w, b)
    link_to_fused(tspn, device, "4 videos", f, pairs, B, N, w, b, got, r, z, S, frames)


def test_whole_segment_rows_against_the_fused_pass(tspn, device):
    """One small video, every ordered pair with (i, i), odd T."""
    NT, T, D, K = 6, 37, 32, 9
    rs, f, w, b = ref.make_operands(831, NT, T, D, K)
    pairs = all_pairs_with_self(NT, 72)
    spans = ref.draw_spans(rs, len(pairs), T)
    got, (r, z, S, frames) = run_case(tspn, device, "small video", f, pairs, spans, w, b)
    link_to_fused(tspn, device, "small video", f, pairs, 1, NT, w, b, got, r, z, S, frames)


def test_cfg3_shape_sampled_pairs(tspn, device):
    """The cfg3 shape (N = 64, T = 900, D = 1024, K = 132): 65536 prefix threads = 256 workgroups, 64 k-steps, prefix
    sums over 900 frames; 96 sampled pairs (two row workgroups, the second half empty above row 96)."""
    N, T, D, K = 64, 900, 1024, 132
    rs, f, w, b = ref.make_operands(832, N, T, D, K)
    allp = oracle.pair_index(N).numpy()
    pairs = allp[rs.permutation(len(allp))[:96]]
    run_case(tspn, device, "cfg3 shape", f, pairs, ref.draw_spans(rs, len(pairs), T), w, b)


def test_a_row_does_not_depend_on_its_place_in_the_table(tspn, device):
    """The same (pair, span) rows in another order and among other rows: the bits of each row stay."""
    NT, T, D, K = 5, 20, 48, 70
    rs, f, w, b = ref.make_operands(833, NT, T, D, K)
    pairs = all_pairs_with_self(NT, 150)
    spans = ref.draw_spans(rs, len(pairs), T)
    base = launch(tspn, device, f, pairs, spans, w, b)
    perm = rs.permutation(len(pairs))[:77]
    moved = launch(tspn, device, f, pairs[perm], spans[perm], w, b)
    assert np.array_equal(bits(moved), bits(base[perm]))


# ------------------------------------------------------------------------------------------------ non-finite features
PLANTED = [("+inf", 0x7F80, False), ("-inf", 0xFF80, False), ("nan", 0x7FC0, False), ("-nan", 0xFFC0, False),
           ("nan payload", 0x7FA5, False), ("inf * 0", 0x7F80, True)]
_clean = {}


def nonfinite_case(tspn, device, NT, T, D, K, zero_weight):
    key = (NT, T, D, K, zero_weight)
    if key not in _clean:
        trk, ch = 2, 3
        rs, f, w, b = ref.make_operands(840, NT, T, D, K)
        if zero_weight:
            w[1, ch] = 0.0           # subject half of predicate 1, object half of predicate K - 1: Inf * 0 = NaN there
            w[K - 1, D + ch] = 0.0
        pairs = all_pairs_with_self(NT, 6 * NT * NT)
        spans = ref.draw_spans(rs, len(pairs), T)
        clean = launch(tspn, device, f, pairs, spans, w, b)
        assert np.isfinite(clean).all()
        _clean[key] = (f, w, b, pairs, spans, clean)
    return _clean[key]


@pytest.mark.parametrize("NT,T,D,K", [(6, 12, 32, 9), (8, 150, 64, 132)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("name,pattern,zero_weight", PLANTED, ids=[p[0].replace(" ", "") for p in PLANTED])
def test_nonfinite_stays_in_the_spans_that_hold_it(tspn, device, NT, T, D, K, where, name, pattern, zero_weight):
    """One non-finite bf16 value in one channel of one frame of one tracklet (the plan of
    test_span_predicate_nonfinite_stays_in_the_spans_that_hold_it).  (a) NaN exactly where the restatement has NaN, 0 / 1
    where it has -Inf / +Inf, the tolerance elsewhere; (b) every output of a row that does not hold the planted frame is
    bit for bit the clean launch's: the prefix sums are non-finite from the planted frame on and must not reach the spans
    behind it."""
    trk, ch = 2, 3
    frame = {"first": 0, "middle": T // 2, "last": T - 1}[where]
    f, w, b, pairs, spans, clean = nonfinite_case(tspn, device, NT, T, D, K, zero_weight)
    bad16 = t(f).to(torch.bfloat16)
    bad16.view(torch.int16)[trk, frame, ch] = int(np.array(pattern, dtype=np.uint16).view(np.int16))
    bad = bad16.float().numpy()
    assert not np.isfinite(bad[trk, frame, ch]) and np.isfinite(bad).sum() == bad.size - 1
    ops = tspn.ops
    got = ops.span_predicate_bf16(bad16.to(device), t(pairs).to(device), t(spans).to(device),
                                  ops.pack_span_cls_bf16(t(w).to(device)), t(b).to(device), K).cpu().numpy()
    r, z, S, frames = ref.span_predicate_ref(bad, pairs, spans, w, b)
    uses = (pairs == trk).any(axis=1)
    holds = uses & (frames[:, 0] <= frame) & (frame < frames[:, 1])
    assert holds.any() and (uses & ~holds).any() and (~uses).any()
    if frame < T - 1:
        assert (uses & (frames[:, 0] > frame)).any()          # spans that start behind the planted frame
    assert np.isfinite(z[~holds]).all() and not np.isfinite(z[holds]).any()
    if zero_weight:
        assert np.isnan(z[holds][:, [1, K - 1]]).any() and np.isinf(z[holds]).any()
    ref.check_against_ref(got, r, z, S, D, f"{name} at frame {frame}")
    leaked = np.argwhere(bits(got)[~holds] != bits(clean)[~holds])
    assert leaked.size == 0, (f"{name} at frame {frame}: {len(leaked)} outputs of rows that do not hold the planted value "
                              f"differ from the clean launch, first {got[~holds][tuple(leaked[0])]}")
