"""Span-bounded association matched on the device (`tspn_span_match_f64`, `ops.span_match`,
`greedy_relational_association(device_spans=True)`): both outputs against the numpy restatement to the bit, every gate at
its edge, the greedy pass under contention, sentinels around caller-held outputs, and the association end to end against
the host path."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import sentinel_buffers as sb
import span_association_cases as sac
import span_match_reference as ref
from test_association import unpack

pytestmark = pytest.mark.gpu

NAMES = ("rel_boxes", "rel_range", "rel_fend", "rel_triplet", "trk_boxes", "pred_triplet", "pred_pair", "pred_span")
WINDOWS = (1, 7, 8, 9, 127, 128, 129)


def problem(seed, U, P, N, L):
    """A random segment whose relations and predictions meet: two triplets, non-integer boxes, relations that end at a
    frame of the segment (or past it, or before it), predictions that start inside them.  For every window length of
    WINDOWS that fits L one pair is planted with that window, starting off the multiples of 8."""
    rs = np.random.RandomState(seed)

    def boxes(*lead):
        xy = rs.uniform(0, 300, size=lead + (L, 2))
        wh = rs.uniform(5, 250, size=lead + (L, 2))
        return np.concatenate([xy, xy + wh], axis=-1)

    trk = boxes(N)
    rel_boxes = boxes(U, 2)
    pair = rs.randint(0, N, size=(P, 2)).astype(np.int32)
    span = np.zeros((P, 2), dtype=np.int32)
    span[:, 0] = rs.randint(0, L, size=P)
    span[:, 1] = np.where(rs.uniform(size=P) < 0.7, L, np.minimum(span[:, 0] + 1 + rs.randint(0, L, size=P), L))
    ptrip = np.stack([rs.randint(0, 2, size=P), np.full(P, 7), np.full(P, 3)], axis=1).astype(np.int64)
    rtrip = np.stack([rs.randint(0, 2, size=U), np.full(U, 7), np.full(U, 3)], axis=1).astype(np.int64)
    rng = np.zeros((U, 2, 2), dtype=np.int32)
    rng[:, :, 1] = rs.randint(max(L // 2, 1), L + 3, size=(U, 1))          # both roles end together, a few past L
    rng[:, 1, 1] -= (rs.uniform(size=U) < 0.2) & (rng[:, 1, 1] > 1)          # some objects end a frame earlier
    rng[:, :, 0] = rs.randint(0, 2, size=(U, 2)) * rs.randint(0, max(L // 3, 1), size=(U, 2))
    fend = rng[:, 1, 1].copy()
    fend[rs.uniform(size=U) < 0.1] = 0                                       # relations that ended before the segment
    if U and P:
        # near-identical boxes where a prediction can meet a relation, so that IoUs pass 0.5 and the greedy pass has work
        for p in range(P):
            u = rs.randint(0, U)
            for c in range(2):
                rel_boxes[u, c] = trk[pair[p, c]] + rs.uniform(-2, 2, size=(L, 4))
        k = 0
        for n in WINDOWS:                                                    # planted windows [a, a + n), a % 8 != 0
            a = 3 if n + 3 <= L else (1 if n + 1 <= L else 0)
            if a + n > L or k >= min(U, P):
                continue
            u = p = k
            k += 1
            span[p] = a, L
            rng[u, :, 0], rng[u, :, 1], fend[u] = 0, a + n, a + n
            rtrip[u] = ptrip[p]
            for c in range(2):
                rel_boxes[u, c] = trk[pair[p, c]] + rs.uniform(-1, 1, size=(L, 4))
    return dict(zip(NAMES, (rel_boxes, rng, fend.astype(np.int32), rtrip, trk, ptrip, pair, span)))


def on_device(prob, device):
    return [torch.from_numpy(np.ascontiguousarray(prob[n])).to(device) for n in NAMES]


def run(tspn, device, prob, thr=0.5):
    match, iou = tspn.ops.span_match(*on_device(prob, device), iou_thr=thr)
    return match.cpu().numpy(), iou.cpu().numpy()


def windows_of(prob, iou):
    """Window lengths (end - a of the subject role) of the candidate pairs."""
    u, p = np.nonzero(iou[:, :, 0] != -1)
    return set((prob["rel_range"][u, 0, 1] - prob["pred_span"][p, 0]).tolist())


def assert_equal(got, want):
    (match, iou), (rmatch, riou) = got, want
    assert match.dtype == np.int32 and iou.dtype == np.float32 and iou.shape == riou.shape
    np.testing.assert_array_equal(iou.view(np.uint32), riou.view(np.uint32))
    np.testing.assert_array_equal(match, rmatch)


@pytest.mark.parametrize("U,P,N,L", [(1, 1, 2, 1), (1, 1, 3, 30), (19, 14, 13, 1), (19, 14, 13, 9), (19, 14, 13, 30),
                                     (19, 14, 13, 137), (19, 14, 13, 300), (300, 260, 17, 9)])
def test_outputs_equal_the_restatement_to_the_bit(tspn, device, U, P, N, L):
    """`iou` as uint32 and `match` against the plain-loop restatement: float32 intersections in frame order, float64 areas
    in numpy's pairwise order over the window that starts at a, the quotient in float64 stored as float32."""
    prob = problem(1000 + 7 * L + U, U, P, N, L)
    want = ref.span_match(*[prob[n] for n in NAMES])
    got = run(tspn, device, prob)
    assert_equal(got, want)
    iou, match = got[1], got[0]
    cand = iou[:, :, 0] != -1
    assert cand.any() and (iou[cand] >= 0).all() and (iou[~cand] == -1).all()
    if (U, P) != (1, 1):
        assert (match >= 0).any() and (match == -1).any() and not cand.all()
        assert windows_of(prob, iou) >= {n for n in WINDOWS if n + 3 <= L}      # every planted window was computed
        starts = prob["pred_span"][np.nonzero(cand)[1], 0]
        assert L == 1 or (starts % 8 != 0).any()
    if U == 300:
        assert match.max() >= 256                                             # a match past the first chunk of relations


def test_no_relations_and_no_predictions(tspn, device):
    prob = problem(5, 0, 5, 4, 9)
    match, iou = run(tspn, device, prob)
    assert match.tolist() == [-1] * 5 and iou.shape == (0, 5, 2)
    prob = problem(6, 3, 0, 4, 9)
    match, iou = run(tspn, device, prob)
    assert match.shape == (0,) and iou.shape == (3, 0, 2)


def edge_problem(L=12, N=3):
    """One relation [2, 8) x [2, 8), fend 8, and one prediction (tracklets 0, 1; span [4, 10)) that passes every gate."""
    rs = np.random.RandomState(77)
    xy = rs.uniform(0, 100, size=(N, L, 2))
    trk = np.concatenate([xy, xy + rs.uniform(20, 90, size=(N, L, 2))], axis=-1)
    rel_boxes = np.stack([trk[0] + 0.25, trk[1] - 0.5])[None]
    return {"rel_boxes": rel_boxes, "rel_range": np.array([[[2, 8], [2, 8]]], dtype=np.int32),
            "rel_fend": np.array([8], dtype=np.int32), "rel_triplet": np.array([[4, 5, 6]], dtype=np.int64), "trk_boxes": trk,
            "pred_triplet": np.array([[4, 5, 6]], dtype=np.int64), "pred_pair": np.array([[0, 1]], dtype=np.int32),
            "pred_span": np.array([[4, 10]], dtype=np.int32)}


def test_gate_edges_one_per_condition(tspn, device):
    base = edge_problem()
    match, iou = run(tspn, device, base)
    assert match.tolist() == [0] and (iou > 0.9).all()
    assert_equal((match, iou), ref.span_match(*[base[n] for n in NAMES]))

    def changed(**kw):
        prob = {k: v.copy() for k, v in base.items()}
        for name, (index, value) in kw.items():
            prob[name][index] = value
        got = run(tspn, device, prob)
        assert_equal(got, ref.span_match(*[prob[n] for n in NAMES]))
        return got

    refused = ([-1], [[[-1.0, -1.0]]])
    for kw in ({"pred_triplet": ((0, 1), 9)},                        # a wrong triplet
               {"rel_fend": (0, 4)},                                 # a == rel_fend
               {"rel_range": ((0, 0, 1), 4)},                        # a == end (subject)
               {"rel_range": ((0, 1, 1), 4)},                        # a == end (object)
               {"rel_range": ((0, 0, 0), 5)},                        # a == start - 1
               {"rel_range": ((0, 1, 0), 5)},
               {"rel_range": ((0, 0, 1), 11)},                       # end == e + 1
               {"rel_range": ((0, 1, 1), 11)},
               {"rel_range": ((0, slice(None), 1), 13), "pred_span": ((0, 1), 12), "rel_fend": (0, 13)}):   # end > L
        m, v = changed(**kw)
        assert (m.tolist(), v.tolist()) == refused, kw
    # each gate at the value that still passes
    for kw in ({"rel_fend": (0, 5)}, {"rel_range": ((0, slice(None), 1), 5)}, {"rel_range": ((0, slice(None), 0), 4)},
               {"rel_range": ((0, slice(None), 1), 10)}, {"pred_span": ((0, 1), 12), "rel_range": ((0, slice(None), 1), 12)}):
        m, v = changed(**kw)
        assert m.tolist() == [0] and (v >= 0).all(), kw


def test_bad_prediction_rows_are_refused_and_their_neighbours_intact(tspn, device):
    """A pair index of N, a negative one, e = L + 1, a < 0 and a == e: the row is -1 whatever the relations hold; the
    rows beside it are what they are without it."""
    L, N = 12, 3
    base = edge_problem(L, N)
    rep = lambda a, n: np.repeat(a, n, axis=0)                      # noqa: E731
    for col, value in (("pred_pair", (0, N)), ("pred_pair", (1, N)), ("pred_pair", (1, -1)), ("pred_span", (1, L + 1)),
                       ("pred_span", (0, -1)), ("pred_span", (0, 10))):
        prob = dict(base, rel_boxes=rep(base["rel_boxes"], 2), rel_range=rep(base["rel_range"], 2),
                    rel_fend=rep(base["rel_fend"], 2), rel_triplet=rep(base["rel_triplet"], 2),
                    pred_triplet=rep(base["pred_triplet"], 3), pred_pair=rep(base["pred_pair"], 3),
                    pred_span=rep(base["pred_span"], 3))
        if col == "pred_span" and value[0] == 1:
            prob["rel_range"][:, :, 1] = L                              # so that only e = L + 1 refuses the row
            prob["rel_fend"][:] = L
            prob["pred_span"][:, 1] = L
        prob[col][1, value[0]] = value[1]
        match, iou = run(tspn, device, prob)
        assert_equal((match, iou), ref.span_match(*[prob[n] for n in NAMES]))
        assert match.tolist() == [0, -1, 1] and (iou[:, 1] == -1).all() and (iou[:, [0, 2]] > 0.9).all(), (col, value)


def test_greedy_contention(tspn, device):
    """Five predictions want one relation: the first gets it.  A prediction whose first choice is taken gets its second.
    A NaN box makes the pair fail."""
    L, N = 12, 3
    base = edge_problem(L, N)
    rep = lambda a, n: np.repeat(a, n, axis=0)                      # noqa: E731
    five = dict(base, pred_triplet=rep(base["pred_triplet"], 5), pred_pair=rep(base["pred_pair"], 5),
                pred_span=rep(base["pred_span"], 5))
    match, iou = run(tspn, device, five)
    assert match.tolist() == [0, -1, -1, -1, -1] and (iou > 0.9).all()
    two = {k: (rep(v, 3) if k.startswith("rel_") else rep(v, 4) if k.startswith("pred_") else v) for k, v in base.items()}
    two["rel_boxes"][1, 0, 5, 2] = np.nan                            # relation 1, subject, a frame inside the window
    match, iou = run(tspn, device, two)
    assert_equal((match, iou), ref.span_match(*[two[n] for n in NAMES]))
    assert match.tolist() == [0, 2, -1, -1]                          # second choice: relation 2, for relation 1 is NaN
    assert np.isnan(iou[1, :, 0]).all() and (iou[1, :, 1] > 0.9).all() and (iou[[0, 2]] > 0.9).all()
    # the threshold decides: nothing reaches 0.999
    assert run(tspn, device, two, thr=0.999)[0].tolist() == [-1] * 4


I32_SENTINEL = -77777          # tests/sentinel_buffers.py's float sentinel has no int32 form; no match is ever this value


def held_i32(n, device):
    buf = torch.full((n + 2 * sb.GUARD,), I32_SENTINEL, dtype=torch.int32, device=device)
    return buf, buf[sb.GUARD:sb.GUARD + n]


def test_sentinels_and_stale_outputs(tspn, device):
    """Through the C entry with caller-held outputs: guard bands intact, every element written, and the result does not
    depend on what iou and match held."""
    A_ = tspn._abi
    U, P, N, L = 19, 14, 13, 30
    prob = problem(4242, U, P, N, L)
    want = ref.span_match(*[prob[n] for n in NAMES])
    ops_in = on_device(prob, device)
    outs = []
    for stale in (False, True):
        ibuf, iou = sb.held((U, P, 2), device)
        mbuf, match = held_i32(P, device)
        if stale:                                                     # stale outputs: passing IoUs, all matched to row 0
            iou.fill_(0.75)
            match.zero_()
        with torch.cuda.device(device):
            tspn.ops.status_words()
            rc = A_.lib().tspn_span_match_f64(*[sb.p(t) for t in ops_in], U, P, N, L, 0.5, sb.p(iou), sb.p(match),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == A_.TSPN_OK, A_.lib().tspn_last_error()
        torch.cuda.synchronize()
        b, m, n = ibuf.cpu(), mbuf.cpu(), iou.numel()
        assert bool((b[:sb.GUARD] == sb.sentinel_of(b)).all()) and bool((b[sb.GUARD + n:] == sb.sentinel_of(b)).all()), "iou"
        assert bool((m[:sb.GUARD] == I32_SENTINEL).all()) and bool((m[sb.GUARD + P:] == I32_SENTINEL).all()), "match"
        if not stale:
            sb.assert_written_inside_only(ibuf, iou, "iou")
            assert not bool((m[sb.GUARD:sb.GUARD + P] == I32_SENTINEL).any()), "match: an element never written"
        outs.append((match.cpu().numpy(), iou.cpu().numpy()))
    assert_equal(outs[0], want)
    assert_equal(outs[1], want)


def test_op_argument_checks(tspn, device):
    ops_in = on_device(problem(9, 3, 4, 5, 9), device)
    sm = tspn.ops.span_match
    for i, other in ((0, torch.float32), (1, torch.int64), (2, torch.int64), (3, torch.int32), (4, torch.float32),
                     (5, torch.int32), (6, torch.int64), (7, torch.int64)):
        bad = list(ops_in)
        bad[i] = bad[i].to(other)
        with pytest.raises(TypeError):
            sm(*bad)
    for i, cut in ((0, lambda t: t[:, :1]), (1, lambda t: t[:2]), (2, lambda t: t[:2]), (3, lambda t: t[:, :2]),
                   (4, lambda t: t[:, :8]), (5, lambda t: t[:, :2]), (6, lambda t: t[:3]), (7, lambda t: t[:3])):
        bad = list(ops_in)
        bad[i] = cut(bad[i]).contiguous()
        with pytest.raises(ValueError):
            sm(*bad)
    bad = list(ops_in)
    bad[4] = bad[4].transpose(0, 1).contiguous().transpose(0, 1)      # right shape, not contiguous
    with pytest.raises(ValueError):
        sm(*bad)
    with pytest.raises(ValueError, match="finite"):
        sm(*ops_in, iou_thr=float("nan"))
    with pytest.raises(RuntimeError):
        sm(*[t.cpu() for t in ops_in])


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("scenario,cap", [((11, 5, 7, 40), 25), ((11, 5, 7, 40), 100), ((23, 12, 32, 120), 100)])
def test_device_spans_association_equals_the_host_path(tspn, device, scenario, cap):
    A = tspn.association
    rels, trajs = sac.spanned(*scenario)
    host = A.greedy_relational_association(None, copy.deepcopy(rels), max_traj_num_in_clip=cap, trajectories=trajs)
    stats = {}
    dev = A.greedy_relational_association(None, copy.deepcopy(rels), max_traj_num_in_clip=cap, trajectories=trajs,
                                          device=device, device_spans=True, stats=stats)
    a, b = unpack(host), unpack(dev)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # the scenario merges across segments and starts off the 15-frame grid (at the cap of 100 the scenarios were chosen for;
    # a cap of 25 keeps a quarter of the predictions and with them fewer merges)
    assert (a["sub_traj_len"] > 30).sum() >= (10 if cap == 100 else 1) and (a["duration"][:, 0] % 15 != 0).any()
    assert 1 <= stats["iou_launches"] <= scenario[1] - 1 and stats["iou_host_rows"] == 0
    assert stats["iou_lookups"] >= stats["iou_launches"] and stats["segments"] == scenario[1]
    # a video of whole-segment predictions takes the batched-table path unchanged, keyword or not
    rels3 = [(index, ([p[:3] for p in preds], iou, tid)) for index, (preds, iou, tid) in rels]
    s3, s3k = {}, {}
    plain = A.greedy_relational_association(None, copy.deepcopy(rels3), max_traj_num_in_clip=cap, trajectories=trajs,
                                            device=device, stats=s3)
    keyed = A.greedy_relational_association(None, copy.deepcopy(rels3), max_traj_num_in_clip=cap, trajectories=trajs,
                                            device=device, device_spans=True, stats=s3k)
    assert plain == keyed and s3 == s3k


def test_association_worker_with_device_spans_gives_the_host_relations(tspn, device):
    A = tspn.association
    rels, trajs = sac.spanned(11, 5, 7, 40)
    want = A.greedy_relational_association(None, copy.deepcopy(rels), max_traj_num_in_clip=60, trajectories=trajs)
    segs = [index for index, _ in rels]
    col = lambda k: [np.stack([np.asarray(p[k]) for p in pr[0]]) for _, pr in rels]   # noqa: E731
    with A.AssociationWorker(device=str(device), max_traj_num_in_clip=60, device_spans=True) as w:
        w.submit_arrays("spans", segs, col(0), col(1), col(2), [trajs[i] for i in segs], spans=col(3))
        key, out, ms, stats = w.result()
    assert key == "spans" and out == want and 1 <= stats["iou_launches"] <= 4 and stats["iou_host_rows"] == 0
