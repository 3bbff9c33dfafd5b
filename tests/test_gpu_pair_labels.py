"""Pair labels from ground-truth relation instances on the GPU (tspn_pair_labels_f32, ops.pair_labels, the `gt_rel_insts`
argument of dataset.proposal_pair_list(s)): every shared case bit-equal to the numpy restatement
(tests/pair_labels_reference.py) in all four outputs, the batched call against the per-segment calls, sentinel-guarded and
unaligned operands through the C ABI, stale outputs, the wrapper's refusals and empty cases, the dataset layer against its
`pred_labels=` path, and a BaseModel training step on the targets it produces."""
import functools

import numpy as np
import pytest
import torch

import cases
import oracle
import pair_labels_reference as ref
import sentinel_buffers as sb
from test_gpu_span_loss import _model, _t

pytestmark = pytest.mark.gpu

NAMES = ("labels", "spans", "span_count", "inst_cols")
INT_SENTINEL = -777                      # no span, count or column takes it


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(case, the four outputs of the restatement): computed once per case, never written to."""
    case = next(c for c in ref.cases() if c["id"] == cid)
    out = ref.case_ref(case)
    for a in out:
        a.setflags(write=False)
    return case, out


def run_op(tspn, device, case, single=None):
    b = {k: _t(v).to(device) for k, v in ref.batch_of(case).items()}
    single = case["single"] if single is None else single
    frames = b["seg_frames"] if case["G"] else None
    if single:
        M = len(b["trackid"])
        return tspn.ops.pair_labels(b["pairs"], b["trackid"], b["iou"].view(M, M), b["insts"], case["K"], case["thr"],
                                    case["merge"], case["G"], frames)
    return tspn.ops.pair_labels(b["pairs"], b["trackid"], b["iou"], b["insts"], case["K"], case["thr"], case["merge"],
                                case["G"], frames, b["pair_off"], b["track_off"], b["iou_off"], b["inst_off"])


def check(got, want, G, what):
    for name, g, w in zip(NAMES, got, want):
        if G == 0 and name in ("spans", "span_count"):
            assert g is None, (what, name)
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if name == "labels":
            g, w = g.view(np.int32), w.view(np.int32)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1)) if len(w) else []
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} rows, first {bad[:5]}"


@pytest.mark.parametrize("cid", ref.case_ids())
def test_outputs_equal_the_restatement(tspn, device, cid):
    case, want = reference(cid)
    check(run_op(tspn, device, case), want, case["G"], cid)


@pytest.mark.parametrize("cid", ["S3-last", "S3-or", "S3-empty-ends-last", "S3-empty-ends-or"])
def test_batched_call_equals_the_per_segment_calls(tspn, device, cid):
    case, _ = reference(cid)
    whole = run_op(tspn, device, case)
    parts = [run_op(tspn, device, dict(case, segments=[s]), single=True) for s in case["segments"]]
    for i, name in enumerate(NAMES):
        if whole[i] is None:
            assert all(p[i] is None for p in parts)
            continue
        assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), (cid, name)


def _held_int(shape, device, dtype, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * sb.GUARD + offset,), INT_SENTINEL, dtype=dtype, device=device)
    return buf, buf[sb.GUARD + offset:sb.GUARD + offset + n].view(shape)


def _int_written_inside_only(buf, v, what):
    b = buf.cpu()
    n, lo = v.numel(), v.storage_offset()
    assert bool((b[:lo] == INT_SENTINEL).all()) and bool((b[lo + n:] == INT_SENTINEL).all()), f"{what}: wrote outside the output"
    assert int((b[lo:lo + n] == INT_SENTINEL).sum()) == 0, f"{what}: outputs never written"


def call_abi(tspn, device, case, labels, spans, span_count, inst_cols, shift=0):
    """The entry through the C ABI on caller-held outputs; `shift` moves every input off its 16-byte alignment (int64
    operands by 8 bytes, iou by 4)."""
    b = ref.batch_of(case)
    keep = {}
    for k, v in b.items():
        t = _t(v).to(device)
        if shift:
            pad = torch.zeros(shift + t.numel(), dtype=t.dtype, device=device)
            pad[shift:] = t.reshape(-1)
            t = pad[shift:].view(t.shape)
            assert t.data_ptr() % 16 == (shift * t.element_size()) % 16
        keep[k] = t
    G = case["G"]
    rc = tspn._abi.lib().tspn_pair_labels_f32(
        sb.p(keep["pairs"]), sb.p(keep["pair_off"]), sb.p(keep["trackid"]), sb.p(keep["track_off"]), sb.p(keep["iou"]),
        sb.p(keep["iou_off"]), sb.p(keep["insts"]), sb.p(keep["inst_off"]), sb.p(keep["seg_frames"] if G else None),
        len(case["segments"]), len(b["pairs"]), len(b["trackid"]), len(b["insts"]), case["K"], G, case["thr"],
        tspn.ops.PAIR_LABEL_MERGES[case["merge"]], sb.p(labels), sb.p(spans if G else None), sb.p(span_count if G else None),
        sb.p(inst_cols), tspn.ops._stream())
    torch.cuda.synchronize(device)
    return rc, keep


@pytest.mark.parametrize("cid,offset", [("P257-last", 0), ("P257-or", 1), ("K65-or", 3), ("K1-last", 2), ("G16-dense-or", 1),
                                        ("S3-last", 1), ("K512-last", 0)])
def test_sentinels_and_unaligned_operands(tspn, device, cid, offset):
    """Outputs held between guard bands, `offset` elements off their alignment (labels off 16 bytes takes the scalar stores),
    inputs off their 16-byte alignment too: every output element written, nothing else, results unchanged."""
    case, want = reference(cid)
    P, R, K, G = len(want[0]), len(want[3]), case["K"], max(case["G"], 1)
    bl, labels = sb.held((P, K), device, offset=offset)
    bs, spans = _held_int((P, G, 2), device, torch.int64, offset)
    bc, count = _held_int((P,), device, torch.int32, offset)
    bi, cols = _held_int((R, 2), device, torch.int32, 2 * (offset % 2))
    with torch.cuda.device(device):
        rc, _ = call_abi(tspn, device, case, labels, spans, count, cols, shift=1 if offset else 0)
    assert rc == 0, tspn._abi.lib().tspn_last_error()
    sb.assert_written_inside_only(bl, labels, cid + " labels")
    _int_written_inside_only(bi, cols, cid + " inst_cols")
    if case["G"]:
        _int_written_inside_only(bs, spans, cid + " spans")
        _int_written_inside_only(bc, count, cid + " span_count")
    else:
        assert bool((bs == INT_SENTINEL).all()) and bool((bc == INT_SENTINEL).all())
    check((labels, spans if case["G"] else None, count if case["G"] else None, cols), want, case["G"], cid)


@pytest.mark.parametrize("cid", ["P515-last", "G4-dense-or", "S3-or"])
def test_stale_outputs_do_not_change_the_result(tspn, device, cid):
    case, want = reference(cid)
    P, R, K, G = len(want[0]), len(want[3]), case["K"], case["G"]
    for fill in (1.0, float("nan")):
        labels = torch.full((P, K), fill, device=device)
        spans = torch.full((P, G, 2), 12345, dtype=torch.int64, device=device)
        count = torch.full((P,), 99, dtype=torch.int32, device=device)
        cols = torch.full((R, 2), 3, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            rc, _ = call_abi(tspn, device, case, labels, spans, count, cols)
        assert rc == 0
        check((labels, spans, count, cols), want, G, f"{cid} stale {fill}")


def test_refusals_and_the_empty_cases(tspn, device):
    ops = tspn.ops
    case, _ = reference("P257-last")
    b = {k: _t(v).to(device) for k, v in ref.batch_of(case).items()}
    M = len(b["trackid"])
    iou = b["iou"].view(M, M)
    good = (b["pairs"], b["trackid"], iou, b["insts"], 132)
    with pytest.raises(TypeError, match="pairs"):
        ops.pair_labels(b["pairs"].to(torch.int32), *good[1:])
    with pytest.raises(TypeError, match="iou"):
        ops.pair_labels(b["pairs"], b["trackid"], iou.double(), b["insts"], 132)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_labels(b["pairs"], b["trackid"].cpu(), iou, b["insts"], 132)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pair_labels(b["pairs"], b["trackid"], iou.t(), b["insts"], 132)
    with pytest.raises(ValueError, match=r"insts \[R,5\]"):
        ops.pair_labels(b["pairs"], b["trackid"], iou, b["insts"][:, :3].contiguous(), 132)
    with pytest.raises(ValueError, match=r"iou must be \[M,M\]"):
        ops.pair_labels(b["pairs"], b["trackid"][:-1].contiguous(), iou, b["insts"], 132)
    with pytest.raises(ValueError, match="merge"):
        ops.pair_labels(*good, merge="first")
    for K in (0, 513):
        with pytest.raises(ValueError, match="num_predicates"):
            ops.pair_labels(*good[:4], K)
    with pytest.raises(ValueError, match="max_spans"):
        ops.pair_labels(*good, max_spans=17)
    with pytest.raises(ValueError, match="seg_frames"):
        ops.pair_labels(*good, max_spans=4)
    with pytest.raises(ValueError, match=r"seg_frames must be \[S,2\]"):
        ops.pair_labels(*good, max_spans=4, seg_frames=torch.zeros((2, 2), dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match="finite"):
        ops.pair_labels(*good, iou_thres=float("nan"))
    with pytest.raises(ValueError, match="go together"):
        ops.pair_labels(*good, pair_off=b["pair_off"])
    with pytest.raises(ValueError, match="flat"):
        ops.pair_labels(*good, pair_off=b["pair_off"], track_off=b["track_off"], iou_off=b["iou_off"], inst_off=b["inst_off"])
    # nothing to label: empty tensors, nothing launched
    e = lambda *shape, dt=torch.int64: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
    labels, spans, count, cols = ops.pair_labels(e(0, 2), e(0), e(0, 0, dt=torch.float32), e(0, 5), 132, max_spans=4,
                                                 seg_frames=e(1, 2))
    assert labels.shape == (0, 132) and spans.shape == (0, 4, 2) and count.shape == (0,) and cols.shape == (0, 2)
    off = e(1)
    labels, spans, count, cols = ops.pair_labels(e(0, 2), e(0), e(0, dt=torch.float32), e(0, 5), 7, pair_off=off,
                                                 track_off=off, iou_off=off, inst_off=off)                 # S = 0
    assert labels.shape == (0, 7) and spans is None and count is None and cols.shape == (0, 2)
    # pairs without instances: zero rows; instances without pairs: their columns
    labels, spans, count, cols = ops.pair_labels(b["pairs"], b["trackid"], iou, e(0, 5), 132)
    assert labels.shape == (257, 132) and not bool(labels.any()) and cols.shape == (0, 2)
    labels, _, _, cols = ops.pair_labels(e(0, 2), b["trackid"], iou, b["insts"], 132)
    assert labels.shape == (0, 132) and np.array_equal(cols.cpu().numpy(), reference("P257-last")[1][3])


# ------------------------------------------------------------------------------------------------ the dataset layer
def _loader_segment(seed, n_prop, gt_ids, R, K, thr, fstart, layout="tail", F=6):
    seg = ref.make_segment(seed, n_prop, gt_ids, 1, R, K, thr, layout=layout, fstart=fstart)
    M = len(seg["trackid"])
    seg["pairs"] = cases.full_pairs(M).astype(np.int64)
    rs = np.random.RandomState(seed)
    seg["feats"] = rs.uniform(0, 1, (len(seg["pairs"]), F)).astype(np.float32)
    seg["cls"] = rs.uniform(-1, 1, (n_prop, 35)).astype(np.float32)
    return seg


def _kept(seg):
    keep = oracle.proposal_pair_idx(seg["pairs"], seg["trackid"])
    return dict(seg, pairs=seg["pairs"][keep])


@pytest.mark.parametrize("merge", ["last", "or"])
def test_proposal_pair_lists_with_gt_rel_insts_equal_the_pred_labels_path(tspn, device, merge):
    """One segment and a batch of three (one without instances, one without ground truth): the TargetList of `gt_rel_insts`
    equals the one of `pred_labels=` fed the restatement's labels of the whole pair table; 'spans' / 'span_count' equal the
    restatement on the kept pairs; the PairLists are the same tensors; [R,3] instances give the same labels and no spans."""
    ds, K, G, thr = tspn.dataset, 132, 4, 0.5
    segs = [_loader_segment(40, 9, ref.GT4, 30, K, thr, 0), _loader_segment(41, 5, (2,), 0, K, thr, 15, layout="mixed"),
            _loader_segment(42, 6, (), 6, K, thr, 30)]
    want = [ref.segment_ref(s, K, G, thr, merge) for s in segs]
    want_kept = [ref.segment_ref(_kept(s), K, G, thr, merge) for s in segs]
    assert want[0][0].sum() > 0 and (want_kept[0][2] > 0).any()
    base = [dict(pairs=s["pairs"], feats=s["feats"], iou=s["iou"], trackid=s["trackid"], cls_logits=s["cls"]) for s in segs]
    by_labels = ds.proposal_pair_lists([dict(d, pred_labels=w[0]) for d, w in zip(base, want)], preprocess=False, device=device)
    by_insts = ds.proposal_pair_lists([dict(d, gt_rel_insts=s["insts"], segment=s["frames"]) for d, s in zip(base, segs)],
                                      preprocess=False, device=device, max_spans=G, iou_thres=thr, merge=merge, num_predicates=K)
    three = ds.proposal_pair_lists([dict(d, gt_rel_insts=s["insts"][:, :3]) for d, s in zip(base, segs)], preprocess=False,
                                   device=device, iou_thres=thr, merge=merge, num_predicates=K)
    for k, s in enumerate(segs):
        (pl_a, tl_a), (pl_b, tl_b), (_, tl_c) = by_labels[k], by_insts[k], three[k]
        assert torch.equal(pl_a.features, pl_b.features) and torch.equal(tl_a.target, tl_b.target), k
        assert torch.equal(pl_a.get_field("tracklet_pairs"), pl_b.get_field("tracklet_pairs"))
        assert np.array_equal(tl_b.target.cpu().numpy(), want_kept[k][0]) and torch.equal(tl_c.target, tl_b.target)
        assert tl_a.fields() == [] and tl_c.fields() == [] and tl_b.fields() == ["spans", "span_count"]
        assert np.array_equal(tl_b.get_field("spans").cpu().numpy(), want_kept[k][1])
        assert np.array_equal(tl_b.get_field("span_count").cpu().numpy(), want_kept[k][2])
        one_pl, one_tl = ds.proposal_pair_list(s["pairs"], s["feats"], s["iou"], s["trackid"], s["cls"], preprocess=False,
                                               device=device, gt_rel_insts=s["insts"], segment=s["frames"], max_spans=G,
                                               iou_thres=thr, merge=merge, num_predicates=K)
        assert torch.equal(one_tl.target, tl_b.target) and torch.equal(one_pl.features, pl_b.features)
        assert torch.equal(one_tl.get_field("spans"), tl_b.get_field("spans"))
        assert torch.equal(one_tl.get_field("span_count"), tl_b.get_field("span_count"))
    # a batch where only some segments carry instances; the others keep their path
    mixed = ds.proposal_pair_lists([dict(base[0], gt_rel_insts=segs[0]["insts"][:, :3]), base[1], dict(base[2], pred_labels=want[2][0])],
                                   preprocess=False, device=device, iou_thres=thr, merge=merge, num_predicates=K)
    assert torch.equal(mixed[0][1].target, by_insts[0][1].target) and mixed[1][1] is None
    assert torch.equal(mixed[2][1].target, by_labels[2][1].target)
    with pytest.raises(ValueError, match="not both"):
        ds.proposal_pair_lists([dict(base[0], pred_labels=want[0][0], gt_rel_insts=segs[0]["insts"])], preprocess=False, device=device)


def test_model_training_step_on_labelled_targets_equals_hand_given_targets(tspn, device):
    """BaseModel in training mode on two segments (7 and 8 proposals, four ground-truth tracks, eight instances; some pairs
    with several spans, some with none) whose TargetLists come from `proposal_pair_list(gt_rel_insts=...)`:
    `loss_rel`, `loss_relationness` and `loss_duration_proposal` equal, bit for bit, those of TargetLists built by hand from
    the restatement's labels and spans."""
    D, T, G, K, thr = 16, ref.SEG_LEN, 3, 132, 0.5
    model, _ = _model(tspn, device, D)
    plists, made, by_hand = [], [], []
    for i, N in enumerate((7, 8)):
        seg = _loader_segment(60 + i, N, ref.GT4, 8, K, thr, 15 * i)
        seg["iou"][N - 2:N, N:] = 0.1                                             # two proposals overlap no ground truth
        assert np.array_equal(_kept(seg)["pairs"], oracle.pair_index(N))         # the model's own pair order
        v = tspn.synth.make_video(95 + i, N, T, D)
        plists.append(tspn.PairList.from_tracklets(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]),
                                                   _t(v["track_cls_logits"])).to(device))
        _, tl = tspn.dataset.proposal_pair_list(seg["pairs"], seg["feats"], seg["iou"], seg["trackid"], seg["cls"],
                                                preprocess=False, device=device, gt_rel_insts=seg["insts"],
                                                segment=seg["frames"], max_spans=G, iou_thres=thr, num_predicates=K)
        labels, spans, count, _ = ref.segment_ref(_kept(seg), K, G, thr, "last")
        assert labels.sum() > 0 and (count > 0).any() and (count == 0).any()
        hand = tspn.TargetList(_t(labels))
        hand.add_field("spans", _t(spans))
        made.append(tl)
        by_hand.append(hand.to(device))
    got, want = model(plists, made), model(plists, by_hand)
    assert set(got) == set(want) == {"loss_relationness", "loss_duration_proposal", "loss_rel"}
    for k in got:
        a, b = got[k].detach().cpu().numpy(), want[k].detach().cpu().numpy()
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and a > 0, (k, a, b)
