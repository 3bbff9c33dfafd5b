"""Relations decoded with their temporal spans on bf16 segments (`tspn_decode_span_relations_bf16`: the bf16 pooling and
GEMM stage, `span_row_topk_q_kernel`, the shared `segment_span_topk_kernel`) against the unfused
composition (tests/span_relations_reference.py fed with `ops.span_predicate_bf16` on the flattened (pair, span) rows).
Only compares and integer work follow the shared per-row values, so equality is asked TO THE BIT: scores as int32 views,
every index as it is, the sentinel behind `valid`."""
import numpy as np
import pytest
import torch

import span_relations_reference as ref
from test_gpu_span_relations import SENT_F_BITS, SENT_I, assert_equal, make_case, sentinel_out, with_spans

pytestmark = pytest.mark.gpu


def bf16_case(tspn, device, S, N, T, D, K, J, seed, **kw):
    c = make_case(device, S, N, T, D, K, J, seed=seed, **kw)
    c["feats"] = c["feats"].to(torch.bfloat16)
    c["packed"] = tspn.ops.pack_span_cls_bf16(c["w"])
    return c


def fused(tspn, c, R, M):
    out = sentinel_out(c, R, M, c["feats"].device)
    res = tspn.ops.decode_span_relations_bf16(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["packed"], c["b"],
                                              c["K"], c["cls"], topk_per_span=R, topk_per_seg=M, out=out)
    assert all(a is b for a, b in zip(res, out))
    return [r.cpu().numpy() for r in res]


def composition(tspn, c, R, M):
    rp, rs = ref.span_rows(c["pairs"], c["N"], c["spans"])
    q = tspn.ops.span_predicate_bf16(c["feats"], rp, rs, c["packed"], c["b"], c["K"])
    return ref.compose(q, c["pairs"], c["spans"], c["score"], c["count"], c["cls"], R, M)


SHAPES = [(1, 2, 1, 16, 1, 1, 1, 1), (1, 5, 7, 16, 64, 3, 20, 200), (3, 5, 12, 32, 132, 4, 20, 200),
          (2, 6, 9, 16, 256, 2, 256, 1024), (1, 32, 6, 16, 132, 4, 20, 200), (1, 4, 5, 32, 65, 16, 70, 50)]


@pytest.mark.parametrize("S,N,T,D,K,J,R,M", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_equals_the_composition(tspn, device, S, N, T, D, K, J, R, M):
    """One lane to four values per lane (K = 1 ... 256), R clamped to K (70 -> 65), one to three segments (segment-local
    ids on global rows), P = 992 pairs in one segment, M = 1024, J = 16 with the NMS leaving ragged counts."""
    c = with_spans(tspn, bf16_case(tspn, device, S, N, T, D, K, J, seed=100 + K + J))
    got = fused(tspn, c, R, M)
    want = composition(tspn, c, R, M)
    assert_equal(got, want)
    assert sum(w["valid"] for w in want) > 0


def test_ragged_counts_and_fewer_candidates_than_topk(tspn, device):
    """All-NaN heads -> count 0 for those pairs; segment 1 keeps one pair only, so its candidates (<= J R = 8) are fewer
    than M = 40: `valid` says so and the tail keeps the sentinel.  Then no proposal anywhere: only valid = 0 is written."""
    S, N, T, D, K, J, R, M = 2, 3, 8, 16, 8, 2, 4, 40
    c = bf16_case(tspn, device, S, N, T, D, K, J, seed=7)
    P = c["P"]
    heads = c["heads"].clone()
    heads[1] = float("nan")
    heads[P + 1:] = float("nan")
    with_spans(tspn, c, heads)
    count = c["count"].cpu().numpy()
    assert count[1] == 0 and (count[P + 1:] == 0).all() and count[P] > 0 and (count[:P] > 0).sum() == P - 1
    got = fused(tspn, c, R, M)
    assert_equal(got, composition(tspn, c, R, M))
    assert int(got[5][1]) == int(count[P]) * R < M and int(got[5][0]) == min(M, int(count[:P].sum()) * R)
    assert not (got[2][0, :int(got[5][0])] == np.array([0, 2])).all(axis=1).any()        # pair 1 = (0, 2) has no span
    with_spans(tspn, c, torch.full_like(heads, float("nan")))
    got = fused(tspn, c, R, M)
    assert (got[5] == 0).all() and (got[0].view(np.int32) == SENT_F_BITS).all() and (got[4] == SENT_I).all()


def test_custom_pair_table_with_repeated_and_reversed_pairs(tspn, device):
    pairs = torch.tensor([[0, 1], [1, 0], [0, 1], [2, 0], [0, 1], [2, 2]], dtype=torch.int64)
    c = with_spans(tspn, bf16_case(tspn, device, 2, 3, 9, 16, 20, 3, seed=33, pairs=pairs))
    c["pairs"][1] = c["pairs"][1].flip(0)                            # another table in the second segment
    assert_equal(fused(tspn, c, 5, 60), composition(tspn, c, 5, 60))
    with pytest.raises(IndexError):
        bad = dict(c, pairs=c["pairs"].clone())
        bad["pairs"][0, 0, 0] = 3
        fused(tspn, bad, 5, 60)
    with pytest.raises(tspn._abi.TspnError):
        tspn.ops.decode_span_relations_bf16(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["packed"], c["b"],
                                            c["K"], c["cls"], topk_per_seg=1025)
