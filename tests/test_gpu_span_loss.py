"""Span anchor targets and losses on the GPU (csrc/spanloss/tspn_span_loss.hip; ops.span_anchor_labels, ops.span_loss; the
'spans' target of DPN training) against the float64 restatement of tests/span_loss_reference.py.

Inputs: integer ground-truth frames and anchor widths that are multiples of 0.25, so every IoU is one correctly rounded
division of exact operands and the labels are compared exactly (tests/test_span_loss_host.py checks the generators).
Tolerances: the two losses to rtol 1e-9 (float64 sums of at most ~10^5 non-negative terms in
another order: n 2^-53, plus libm differences); the counts exactly; dheads to rtol 2^-22 with atol 0 (an fp32 rounding of
a float64 value that may differ in its last bits -- in fact two roundings, of the un-normalised gradient and of its
quotient by the normaliser: at most 2^-23 relative) and exactly 0 where the restatement's gradient is 0."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cases
import oracle
import sentinel_buffers as sb
import span_loss_reference as ref
from test_span_loss_host import FULL_SHAPES, SHAPES, case, round_trip_heads
from train_reference import train_reference

pytestmark = pytest.mark.gpu

RTOL_LOSS, RTOL_GRAD = 1e-9, 2.0 ** -22


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(gt, sizes, heads, out, dheads, label, matched) of one shape, computed once and shared; never written to."""
    gt, sizes, heads = case(shape)
    out, dh, label, matched = ref.span_loss_ref(heads, gt, sizes)
    for a in (gt, heads, out, dh, label, matched):
        a.setflags(write=False)
    return gt, tuple(sizes), heads, out, dh, label, matched


def launch(tspn, device, gt, sizes, heads, T, mask=None):
    """(label, matched, out, dheads) of the three entries as numpy arrays."""
    g, h = torch.from_numpy(np.array(gt)).to(device), torch.from_numpy(np.array(heads)).to(device)
    label, matched = tspn.ops.span_anchor_labels(g, list(sizes), T, ref.POS_IOU, ref.NEG_IOU)
    m = None if mask is None else torch.from_numpy(mask).to(device)
    out, dh = tspn.ops.span_loss(h, g, list(sizes), label, matched, mask=m, beta=ref.BETA)
    return label.cpu().numpy(), matched.cpu().numpy(), out.cpu().numpy(), dh.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def check_losses(got_out, got_dh, want_out, want_dh, what):
    print(f"{what}: out {got_out.tolist()} want {want_out.tolist()}; max |dheads - ref| / |ref| = "
          f"{np.max(np.abs(got_dh - want_dh)[want_dh != 0] / np.abs(want_dh[want_dh != 0]), initial=0.0):.3g}")
    np.testing.assert_allclose(got_out[:2], want_out[:2], rtol=RTOL_LOSS, atol=0, err_msg=what)
    assert got_out[2:].tolist() == want_out[2:].tolist(), what
    assert not got_dh[want_dh == 0].any(), f"{what}: a gradient where the restatement has none"
    np.testing.assert_allclose(got_dh.astype(np.float64), want_dh, rtol=RTOL_GRAD, atol=0, err_msg=what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_and_matches_equal_the_restatement(tspn, device, shape):
    gt, sizes, heads, _, _, label, matched = reference(shape)
    if shape in FULL_SHAPES:
        cond = ref.input_conditions(gt, sizes, shape[3])
        assert all(cond.values()), cond
    got_label, got_matched, _, _ = launch(tspn, device, gt, sizes, heads, shape[3])
    assert got_label.dtype == np.int8 and got_label.shape == (shape[0], shape[2], shape[3])
    assert np.array_equal(got_matched, matched), np.argwhere(got_matched != matched)[:5]
    assert np.array_equal(got_label, label), np.argwhere(got_label != label)[:5]


def test_threshold_edges(tspn, device):
    """The hand-made cases of span_loss_reference.edge_cases (checked on the restatement by the host test): IoU exactly 7/10
    is positive, exactly 3/10 is ignored, a span equal to an anchor has IoU 1, and [0, 1) under wide anchors gives a plateau
    of tied low-quality positives."""
    for name, gt, sizes, T, expect in ref.edge_cases():
        g = torch.tensor(gt, dtype=torch.int64, device=device)
        label, matched = tspn.ops.span_anchor_labels(g, sizes, T, ref.POS_IOU, ref.NEG_IOU)
        want_label, want_matched, _ = ref.labels_ref(np.array(gt), sizes, T)
        label, matched = label.cpu().numpy(), matched.cpu().numpy()
        for (a, t), want in expect.items():
            assert label[0, a, t] == want, (name, a, t, label[0, a, t])
        assert np.array_equal(label, want_label) and np.array_equal(matched, want_matched), name
    # the thresholds are parameters: IoU 7/10 under pos_iou = 0.75 is ignored unless the low-quality rule holds it
    name, gt, sizes, T, _ = ref.edge_cases()[0]
    label, _ = tspn.ops.span_anchor_labels(torch.tensor(gt, device=device), sizes, T, 0.75, 0.3)
    assert label.cpu().numpy()[0, 0, 10] == -1 == ref.labels_ref(np.array(gt), sizes, T, 0.75, 0.3)[0][0, 0, 10]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_losses_and_gradient_against_the_restatement(tspn, device, shape):
    gt, sizes, heads, out, dh, label, matched = reference(shape)
    if shape in FULL_SHAPES:
        cond = ref.input_conditions(gt, sizes, shape[3], heads)
        assert all(cond.values()), cond                   # |d| < beta and |d| > beta on both channels among them
    if shape[1] == 0:                                     # the segment without a positive anchor
        assert out[3] == 0 and out[1] == 0 and out[2] == shape[0] * shape[2] * shape[3]
    _, _, got_out, got_dh = launch(tspn, device, gt, sizes, heads, shape[3])
    check_losses(got_out, got_dh, out, dh, str(shape))
    if shape[1] == 0:
        assert got_out[1] == 0 and got_out[3] == 0 and not got_dh[:, shape[2]:].any()


def _masks(shape):
    """A mask that removes every positive of one pair and some negatives of another."""
    gt, sizes, heads, _, _, label, _ = reference(shape)
    mask = np.ones(label.shape, np.uint8)
    p_pos = next(p for p in range(3, shape[0]) if (label[p] == 1).any())
    p_neg = next(p for p in range(shape[0]) if p != p_pos and (label[p] == 0).sum() >= 4)
    mask[p_pos][label[p_pos] == 1] = 0
    neg = np.argwhere(label[p_neg] == 0)[::2]
    mask[p_neg][neg[:, 0], neg[:, 1]] = 0
    assert (mask[p_pos] == 0).any() and (mask[p_neg] == 0).any() and p_pos != p_neg
    return mask


@pytest.mark.parametrize("shape", [(5, 3, 4, 17), (257, 2, 4, 30)], ids=lambda s: "x".join(map(str, s)))
def test_mask(tspn, device, shape):
    gt, sizes, heads, out, dh, label, matched = reference(shape)
    mask = _masks(shape)
    want_out, want_dh, _, _ = ref.span_loss_ref(heads, gt, sizes, mask=mask)
    assert want_out[2] < out[2] and want_out[3] < out[3]
    got_label, got_matched, got_out, got_dh = launch(tspn, device, gt, sizes, heads, shape[3], mask=mask)
    assert np.array_equal(got_label, label) and np.array_equal(got_matched, matched)     # the matching ignores the mask
    check_losses(got_out, got_dh, want_out, want_dh, f"{shape} masked")
    assert not got_dh[:, :shape[2]][mask == 0].any()
    # all ones = no mask, to the bit
    _, _, none_out, none_dh = launch(tspn, device, gt, sizes, heads, shape[3])
    _, _, ones_out, ones_dh = launch(tspn, device, gt, sizes, heads, shape[3], mask=np.ones(label.shape, np.uint8))
    assert np.array_equal(bits(none_out), bits(ones_out)) and np.array_equal(bits(none_dh), bits(ones_dh))


def test_two_launches_are_bit_equal(tspn, device):
    shape = (257, 2, 4, 30)
    gt, sizes, heads = reference(shape)[:3]
    a, b = launch(tspn, device, gt, sizes, heads, shape[3]), launch(tspn, device, gt, sizes, heads, shape[3])
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_nan_heads(tspn, device):
    shape = (5, 3, 4, 17)
    gt, sizes, heads, _, _, label, _ = reference(shape)
    A, T = shape[2], shape[3]
    mask = _masks(shape)
    _, _, clean_out, clean_dh = launch(tspn, device, gt, sizes, heads, T, mask=mask)
    # NaN in every head element that enters no loss: all three channels of the ignored and of the masked anchors, and
    # the regression channels of the negatives
    off = (label == -1) | (mask == 0)
    noreg = off | (label == 0)
    assert (label == -1).any() and (mask == 0).any() and off.sum() > 20
    dirty = np.array(heads)
    dirty[:, :A][off] = np.nan
    dirty[:, A::2][noreg] = np.nan
    dirty[:, A + 1::2][noreg] = np.nan
    assert np.isnan(dirty).sum() == off.sum() + 2 * noreg.sum()
    _, _, out, dh = launch(tspn, device, gt, sizes, dirty, T, mask=mask)
    assert np.array_equal(bits(out), bits(clean_out)) and np.array_equal(bits(dh), bits(clean_dh))
    # a NaN logit at a labelled anchor: that loss and that gradient element, nothing else
    p, a, t = np.argwhere((label == 0) & (mask == 1))[3]
    dirty = np.array(heads)
    dirty[p, a, t] = np.nan
    _, _, out, dh = launch(tspn, device, gt, sizes, dirty, T, mask=mask)
    assert np.isnan(out[0]) and np.array_equal(bits(out[1:]), bits(clean_out[1:]))
    assert np.isnan(dh[p, a, t])
    dh[p, a, t] = clean_dh[p, a, t]
    assert np.array_equal(bits(dh), bits(clean_dh))


def _held_i8(shape, device):
    """sentinel_buffers.held for int8 (its float sentinel does not fit): 77 is no label and no row."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * sb.GUARD,), 77, dtype=torch.int8, device=device)
    return buf, buf[sb.GUARD:sb.GUARD + n].view(shape)


def _i8_written_inside_only(buf, v, what):
    b, n = buf.cpu(), v.numel()
    assert bool((b[:sb.GUARD] == 77).all()) and bool((b[sb.GUARD + n:] == 77).all()), f"{what}: wrote outside the output"
    assert not bool((b[sb.GUARD:sb.GUARD + n] == 77).any()), f"{what}: outputs never written"


@pytest.mark.parametrize("shape", [(5, 3, 4, 17), (257, 2, 4, 30)], ids=lambda s: "x".join(map(str, s)))
def test_sentinels_nothing_written_outside_the_outputs(tspn, device, shape):
    P, G, A, T = shape
    gt, sizes, heads, out, dh, label, matched = reference(shape)
    lib, p = tspn._abi.lib(), sb.p
    g, h = torch.from_numpy(np.array(gt)).to(device), torch.from_numpy(np.array(heads)).to(device)
    sz = (ctypes.c_float * A)(*sizes)
    lab_buf, lab = _held_i8((P, A, T), device)
    mat_buf, mat = _held_i8((P, A, T), device)
    par_buf, par = sb.held((P, 4), device, torch.float64)
    out_buf, o = sb.held((4,), device, torch.float64)
    dh_buf, d = sb.held((P, 3 * A, T), device)
    stream = tspn.ops._stream()
    assert lib.tspn_span_anchor_labels(p(g), sz, P, G, A, T, ref.POS_IOU, ref.NEG_IOU, p(lab), p(mat), stream) == 0
    assert lib.tspn_span_loss_f32(p(h), p(g), sz, p(lab), p(mat), None, P, G, A, T, ref.BETA, p(par), p(d), stream) == 0
    assert lib.tspn_span_loss_finish(p(par), P, A, T, p(o), p(d), stream) == 0
    _i8_written_inside_only(lab_buf, lab, "label")
    _i8_written_inside_only(mat_buf, mat, "matched")
    for buf, v, what in ((par_buf, par, "partials"), (out_buf, o, "out"), (dh_buf, d, "dheads")):
        sb.assert_written_inside_only(buf, v, what)
    assert np.array_equal(lab.cpu().numpy(), label) and np.array_equal(mat.cpu().numpy(), matched)
    check_losses(o.cpu().numpy(), d.cpu().numpy(), out, dh, f"{shape} held")
    # the partials are the per-pair sums and counts: their totals are the segment's
    par = par.cpu().numpy()
    assert par[:, 1].sum() == out[2] and par[:, 3].sum() == out[3]
    assert par[0].tolist()[1::2] == [A * T, 0.0]           # pair 0 has no ground truth: every anchor negative


def test_refusals_and_the_empty_case(tspn, device):
    P, G, A, T = 5, 3, 4, 17
    gt, sizes, heads, _, _, label, matched = reference((P, G, A, T))
    A_, lib, p = tspn._abi, tspn._abi.lib(), sb.p
    g, h = torch.from_numpy(np.array(gt)).to(device), torch.from_numpy(np.array(heads)).to(device)
    lab_d, mat_d = torch.from_numpy(np.array(label)).to(device), torch.from_numpy(np.array(matched)).to(device)
    sz = (ctypes.c_float * 16)(*(list(sizes) + [1.0] * 12))
    lab_buf, lab = _held_i8((P, A, T), device)
    mat_buf, mat = _held_i8((P, A, T), device)
    par_buf, par = sb.held((P, 4), device, torch.float64)
    out_buf, o = sb.held((4,), device, torch.float64)
    dh_buf, d = sb.held((P, 3 * A, T), device)
    stream = tspn.ops._stream()

    def labels(gt_=g, sz_=sz, P_=P, G_=G, A_n=A, T_=T, pos=0.7, neg=0.3, label_=lab, matched_=mat):
        return lib.tspn_span_anchor_labels(p(gt_), sz_, P_, G_, A_n, T_, pos, neg, p(label_), p(matched_), stream)

    def loss(heads_=h, gt_=g, label_=lab_d, matched_=mat_d, G_=G, A_n=A, T_=T, beta=ref.BETA, partials=par, dheads=d):
        return lib.tspn_span_loss_f32(p(heads_), p(gt_), sz, p(label_), p(matched_), None, P, G_, A_n, T_, beta, p(partials),
                                      p(dheads), stream)

    def finish(partials=par, A_n=A, T_=T, out=o, dheads=d):
        return lib.tspn_span_loss_finish(p(partials), P, A_n, T_, p(out), p(dheads), stream)

    for call in (labels, loss):
        assert call(G_=9) == A_.TSPN_EUNSUPPORTED and call(G_=-1) == A_.TSPN_EINVAL and call(gt_=None) == A_.TSPN_EINVAL
    for call in (labels, loss, finish):
        assert call(A_n=17) == A_.TSPN_EUNSUPPORTED and call(A_n=0) == A_.TSPN_EINVAL and call(T_=0) == A_.TSPN_EINVAL
        assert call(A_n=16, T_=2 ** 27) == A_.TSPN_EUNSUPPORTED
    for pos, neg in ((0.3, 0.7), (1.5, 0.3), (0.7, -0.1), (float("nan"), 0.3)):
        assert labels(pos=pos, neg=neg) == A_.TSPN_EINVAL
    assert labels(label_=None) == A_.TSPN_EINVAL and labels(matched_=None) == A_.TSPN_EINVAL
    assert loss(heads_=None) == A_.TSPN_EINVAL and loss(partials=None) == A_.TSPN_EINVAL and loss(dheads=None) == A_.TSPN_EINVAL
    assert loss(label_=None) == A_.TSPN_EINVAL and loss(matched_=None) == A_.TSPN_EINVAL and loss(beta=0.0) == A_.TSPN_EINVAL
    assert finish(out=None) == A_.TSPN_EINVAL and finish(partials=None) == A_.TSPN_EINVAL and finish(dheads=None) == A_.TSPN_EINVAL
    torch.cuda.synchronize(device)
    for buf in (par_buf, out_buf, dh_buf):
        sb.assert_untouched(buf, "a refused call")
    assert bool((lab_buf == 77).all()) and bool((mat_buf == 77).all())
    # the ops' own checks
    ops = tspn.ops
    with pytest.raises(TypeError):
        ops.span_anchor_labels(g.int(), list(sizes), T)
    with pytest.raises(ValueError):
        ops.span_anchor_labels(g[:, :, :1].contiguous(), list(sizes), T)
    with pytest.raises(ValueError):
        ops.span_loss(h, g, list(sizes)[:3], lab_d, mat_d)
    with pytest.raises(ValueError):
        ops.span_loss(h, g[:4].contiguous(), list(sizes), lab_d, mat_d)
    with pytest.raises(TypeError):
        ops.span_loss(h, g, list(sizes), lab_d.int(), mat_d)
    with pytest.raises(ValueError):
        ops.span_loss(h, g, list(sizes), lab_d, mat_d, mask=torch.ones((P, A, T + 1), dtype=torch.uint8, device=device))
    with pytest.raises(ValueError):
        ops.span_loss(h.transpose(0, 1), g, list(sizes), lab_d, mat_d)
    with pytest.raises(tspn._abi.TspnError):
        ops.span_anchor_labels(g, list(sizes), T, pos_iou=0.2, neg_iou=0.3)
    # P = 0: nothing to label, and the losses are written as zeros
    g0 = torch.zeros((0, G, 2), dtype=torch.int64, device=device)
    lab0, mat0 = ops.span_anchor_labels(g0, list(sizes), T)
    assert lab0.shape == (0, A, T) and mat0.shape == (0, A, T)
    out0, dh0 = ops.span_loss(torch.zeros((0, 3 * A, T), device=device), g0, list(sizes), lab0, mat0)
    assert out0.cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and dh0.shape == (0, 3 * A, T)


# ------------------------------------------------------------------------------------------------------- the model
def _temporal_cfg(D):
    return cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                 "PREDICT.FEATURE_DIM": 2 * D})


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _model(tspn, device, D):
    sd = tspn.synth.make_weights(3, c=2 * D, bias_std=0.05)
    model = tspn.BaseModel(_temporal_cfg(D))
    own = model.state_dict()
    model.load_state_dict({k: _t(v) for k, v in sd.items() if k in own})
    return model.to(device).train(), sd


def _dpn_grads(model):
    h = model.relpn.duration_proposal_network.dpn_head
    return {"conv_w": h.conv.weight.grad, "conv_b": h.conv.bias.grad, "dur_w": h.duration_pred.weight.grad,
            "dur_b": h.duration_pred.bias.grad, "rel_w": h.relness_pred.weight.grad, "rel_b": h.relness_pred.bias.grad,
            "cls_w": model.classifier.rel_predictor.weight.grad, "cls_b": model.classifier.rel_predictor.bias.grad}


@pytest.mark.parametrize("form", ["tracklets", "dense"])
def test_model_trains_the_span_heads_from_a_spans_target(tspn, device, form):
    """BaseModel in training mode with a 'spans' target on two segments of different N (T = 30, D = 16, A = 4, G = 3; pair 0
    of each has no ground truth): `loss_relationness`, `loss_duration_proposal` and every DPN-head parameter gradient
    against the float64 autograd restatement (span_loss_reference.train_reference_spans), with the tolerances of
    tests/test_gpu_model.py: losses rtol 2e-5, parameter gradients atol 2e-4 max|ref| + 1e-9."""
    D, T, G, K = 16, 30, 3, 132
    model, sd = _model(tspn, device, D)
    segments, plists, tlists = [], [], []
    for i, N in enumerate((5, 6)):
        v = tspn.synth.make_video(95 + i, N, T, D)
        pairs = oracle.pair_index(N)
        P = pairs.shape[0]
        gt = ref.make_gt(70 + i, P, G, T)
        assert (gt[0, :, 1] <= gt[0, :, 0]).all() and (gt[1:, :, 1] > gt[1:, :, 0]).any(axis=1).all()
        targets = _t((tspn.hashrng.uniform(96 + i, "tg", (P, K)) < 0.05).astype(np.float32))
        if form == "tracklets":
            plist = tspn.PairList.from_tracklets(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), _t(v["track_cls_logits"]))
        else:
            plist = tspn.PairList(oracle.pair_gather(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), pairs)[0])
        tlist = tspn.TargetList(targets)
        tlist.add_field("spans", _t(gt))
        segments.append((v, pairs, gt, targets))
        plists.append(plist.to(device))
        tlists.append(tlist.to(device))
    loss = model(plists, tlists)
    assert set(loss) == {"loss_relationness", "loss_duration_proposal", "loss_rel"} and all(x.dim() == 0 for x in loss.values())
    sum(loss.values()).backward()
    ref_loss, ref_grad = ref.train_reference_spans(segments, sd, model.anchor_sizes)
    assert model.anchor_sizes(T) == [7.5, 15.0, 22.5, 30.0]
    print({k: (loss[k].item(), ref_loss[k]) for k in loss})
    for k in loss:
        np.testing.assert_allclose(loss[k].item(), ref_loss[k], rtol=2e-5, err_msg=k)
    for k, gq in _dpn_grads(model).items():
        r = ref_grad[k].numpy()
        assert np.abs(r).max() > 0, k
        np.testing.assert_allclose(gq.cpu().numpy(), r, rtol=0, atol=2e-4 * np.abs(r).max() + 1e-9, err_msg=k)
    # an upstream gradient other than 1 scales each loss's own rows
    model.zero_grad(set_to_none=True)
    loss = model(plists, tlists)
    (2.0 * loss["loss_relationness"] + 0.0 * loss["loss_duration_proposal"]).backward()
    g = _dpn_grads(model)
    assert float(g["dur_w"].abs().max()) == 0.0 and float(g["rel_w"].abs().max()) > 0.0


def test_model_duration_target_is_unchanged_and_both_targets_raise(tspn, device):
    """A target with 'duration' alone takes the code it took before: losses and gradients against tests/train_reference.py,
    as tests/test_gpu_model.py::test_temporal_branch_training_losses_and_grads compares them.  'spans' together with
    'duration' raises, and so does a batch that mixes the two kinds."""
    D, N, T, A, K, G = 16, 5, 30, 4, 132, 3
    model, sd = _model(tspn, device, D)
    v = tspn.synth.make_video(97, N, T, D)
    pairs = oracle.pair_index(N)
    P = pairs.shape[0]
    gt_dur = _t((tspn.hashrng.uniform(98, "gt_dur", (P, 2 * A, T)) < 0.3).astype(np.float32))
    targets = _t((tspn.hashrng.uniform(98, "tg", (P, K)) < 0.05).astype(np.float32))
    plist = tspn.PairList.from_tracklets(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), _t(v["track_cls_logits"])).to(device)
    tlist = tspn.TargetList(targets)
    tlist.add_field("duration", gt_dur)
    loss = model([plist], [tlist.to(device)])
    assert set(loss) == {"loss_duration", "loss_rel"}
    sum(loss.values()).backward()
    ref_loss, ref_grad = train_reference(v, pairs, sd, gt_dur, None, targets)
    for k in loss:
        np.testing.assert_allclose(loss[k].item(), ref_loss[k], rtol=2e-5)
    got = _dpn_grads(model)
    for k in ("conv_w", "conv_b", "dur_w", "dur_b", "cls_w", "cls_b"):
        r = ref_grad[k].numpy()
        np.testing.assert_allclose(got[k].cpu().numpy(), r, rtol=0, atol=2e-4 * np.abs(r).max() + 1e-9, err_msg=k)
    both = tspn.TargetList(targets)
    both.add_field("duration", gt_dur)
    both.add_field("spans", _t(ref.make_gt(71, P, G, T)))
    with pytest.raises(ValueError, match="not both"):
        model([plist], [both.to(device)])
    only_spans = tspn.TargetList(targets)
    only_spans.add_field("spans", _t(ref.make_gt(71, P, G, T)))
    with pytest.raises(ValueError, match="not both"):
        model([plist, plist], [only_spans.to(device), tlist.to(device)])
    wrong = tspn.TargetList(targets)
    wrong.add_field("spans", torch.zeros((P + 1, G, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="spans"):
        model([plist], [wrong.to(device)])


def test_decode_round_trip(tspn, device):
    """Heads that hold the regression targets of the restatement (float64, rounded to fp32) and logits of +10 at positives,
    -10 elsewhere decode, with top_k = 1, to the ground-truth row itself -- for every pair with ground truth whose
    positives all match one row, the statement's own condition; no such pair is left out (156 pairs over these shapes;
    tests/test_span_loss_host.py::test_decode_round_trip_on_the_oracle shows the same on oracle.decode_spans)."""
    total = 0
    for shape in FULL_SHAPES:
        P, G, A, T = shape
        gt, sizes = reference(shape)[:2]
        heads, pairs = round_trip_heads(gt, sizes, T)
        got = tspn.ops.decode_spans(torch.from_numpy(heads).to(device), list(sizes), top_k=1)
        span, count = got["span"][:, 0].cpu().numpy(), got["count"].cpu().numpy()
        assert len(pairs) >= 2
        for p, g in pairs:
            assert count[p] == 1 and span[p].tolist() == gt[p, g].tolist(), (shape, p, span[p], gt[p, g])
        total += len(pairs)
    assert total >= 150
