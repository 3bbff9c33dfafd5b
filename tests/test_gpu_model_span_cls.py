"""RELPN.DPN.POOL_GT_SPAN through BaseModel: a training step at N = 5, T = 12, D = 16 on two segments whose targets
carry 'spans', 'span_count' and 'span_labels', against float64 autograd (binary_cross_entropy_with_logits over explicitly
pooled rows): loss_rel at rtol 2e-5, the classifier gradients at atol 2e-4 max|ref| + 1e-9 (the tolerances of
tests/test_gpu_training_shapes.py), every other loss and gradient bit-equal to the same step with the switch off, a
missing target field refused by name, and the loader's 'span_labels' field."""
import numpy as np
import pytest
import torch

import cases
import oracle
import pair_labels_reference as plr
import span_cls_reference as ref
from test_gpu_span_loss import _dpn_grads, _t

pytestmark = pytest.mark.gpu

N, T, D, K, G = 5, 12, 16, 132, 3


def build(tspn, device, pool_gt_span):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D})
    cfg.RELPN.DPN.POOL_GT_SPAN = pool_gt_span
    sd = tspn.synth.make_weights(3, c=2 * D, bias_std=0.05)
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: _t(v) for k, v in sd.items() if k in own})
    return model.to(device).train(), sd


def segments(tspn):
    out = []
    for i in range(2):
        v = tspn.synth.make_video(140 + i, N, T, D)
        c = ref.loss_case(150 + i, N, 1, T, D, K, G)
        # the span heads refuse nothing here: rows beyond a pair's count are padding (0, 0)
        out.append({"v": v, "pairs": c["pairs"], "spans": c["spans"], "span_count": c["span_count"], "span_labels": c["span_labels"],
                    "targets": (tspn.hashrng.uniform(160 + i, "tg", (len(c["pairs"]), K)) < 0.05).astype(np.float32)})
    return out


def lists_of(tspn, device, segs, drop=None):
    plists, tlists = [], []
    for s in segs:
        v = s["v"]
        plists.append(tspn.PairList.from_tracklets(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), _t(v["track_cls_logits"])).to(device))
        tl = tspn.TargetList(_t(s["targets"]))
        for name in ("spans", "span_count", "span_labels"):
            if name != drop:
                tl.add_field(name, _t(s[name]))
        tlists.append(tl.to(device))
    return plists, tlists


def autograd_reference(segs, sd):
    w = _t(sd["classifier.rel_predictor.weight"]).double().requires_grad_(True)
    b = _t(sd["classifier.rel_predictor.bias"]).double().requires_grad_(True)
    total = 0
    for s in segs:
        f = _t(s["v"]["tracklet_feats"]).double()
        valid, a, e = ref.row_table(s["pairs"], s["spans"], s["span_count"], N, T, G)
        xs, ys = [], []
        for p, g in zip(*np.nonzero(valid)):
            i, j = s["pairs"][p]
            xs.append(torch.cat([f[i, a[p, g]:e[p, g]].mean(0), f[j, a[p, g]:e[p, g]].mean(0)]))
            ys.append(_t(s["span_labels"][p, g] if s["span_count"][p] >= 1 else np.zeros(K, np.float32)).double())
        total = total + torch.nn.functional.binary_cross_entropy_with_logits(torch.stack(xs) @ w.t() + b, torch.stack(ys))
    total.backward()
    return float(total.detach()), w.grad.numpy(), b.grad.numpy()


def test_training_step_with_the_switch_on_and_off(tspn, device):
    segs = segments(tspn)
    assert np.array_equal(segs[0]["pairs"], oracle.pair_index(N).numpy())
    steps = {}
    for on in (False, True):
        model, sd = build(tspn, device, on)
        assert model.pool_gt_span is on
        loss = model(*lists_of(tspn, device, segs))
        assert set(loss) == {"loss_relationness", "loss_duration_proposal", "loss_rel"}
        sum(loss.values()).backward()
        steps[on] = ({k: v.detach().clone() for k, v in loss.items()}, {k: g.clone() for k, g in _dpn_grads(model).items()})
    want_loss, want_w, want_b = autograd_reference(segs, sd)
    loss, grads = steps[True]
    print(f"loss_rel {loss['loss_rel'].item():.10g} vs {want_loss:.10g}")
    np.testing.assert_allclose(loss["loss_rel"].item(), want_loss, rtol=2e-5)
    for name, want in (("cls_w", want_w), ("cls_b", want_b)):
        got = grads[name].cpu().numpy()
        print(f"d{name}: max|ref| {np.abs(want).max():.3g}, error {np.abs(got - want).max():.3g}")
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-4 * np.abs(want).max() + 1e-9, err_msg=name)
    off_loss, off_grads = steps[False]
    assert not torch.equal(off_loss["loss_rel"], loss["loss_rel"]) and not torch.equal(off_grads["cls_w"], grads["cls_w"])
    for k in ("loss_relationness", "loss_duration_proposal"):
        assert torch.equal(off_loss[k], loss[k]), k
    for k in ("conv_w", "conv_b", "dur_w", "dur_b", "rel_w", "rel_b"):
        assert torch.equal(off_grads[k], grads[k]), k


@pytest.mark.parametrize("field", ["span_labels", "span_count"])
def test_a_missing_target_field_is_refused_by_name(tspn, device, field):
    model, _ = build(tspn, device, True)
    with pytest.raises(ValueError, match=f"'{field}'"):
        model(*lists_of(tspn, device, segments(tspn), drop=field))


def test_baseline_form_segments_keep_their_path_and_the_loader_adds_span_labels(tspn, device):
    """dataset.proposal_pair_list(s) with span_labels=True: the 'span_labels' field equals the restatement on the kept pair
    table, the batch form equals the per-segment form; a model with the switch on trains such [P,F] samples as before."""
    case = next(c for c in plr.cases() if c["id"] == "S3-or")
    segs = [s for s in case["segments"] if len(s["pairs"])]
    rs = np.random.RandomState(3)
    loader_segs = []
    for s in segs:
        M = len(s["trackid"])
        allp = np.array([(a, b) for a in range(M) for b in range(M) if a != b], np.int64)
        loader_segs.append({"pairs": allp, "feats": rs.uniform(0, 1, (len(allp), 40)).astype(np.float32), "iou": s["iou"],
                            "trackid": s["trackid"], "cls_logits": np.zeros((M, 4), np.float32), "gt_rel_insts": s["insts"],
                            "segment": s["frames"]})
    kw = dict(preprocess=False, device=device, max_spans=4, iou_thres=case["thr"], merge="or", num_predicates=case["K"])
    batch = tspn.dataset.proposal_pair_lists(loader_segs, span_labels=True, **kw)
    with_rows = 0
    for s, ls, (plist, tlist) in zip(segs, loader_segs, batch):
        one_p, one_t = tspn.dataset.proposal_pair_list(ls["pairs"], ls["feats"], ls["iou"], ls["trackid"], ls["cls_logits"],
                                                       gt_rel_insts=ls["gt_rel_insts"], segment=ls["segment"], span_labels=True, **kw)
        kept = plist.get_field("tracklet_pairs").cpu().numpy()
        seg = dict(s, pairs=kept)
        _, spans, count, _ = plr.segment_ref(seg, case["K"], 4, case["thr"], "or")
        want = ref.span_labels_segment(seg, case["K"], 4, case["thr"], "or", spans, count)
        got = tlist.get_field("span_labels")
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
        with_rows += bool(want.any())
        assert torch.equal(got, one_t.get_field("span_labels")) and torch.equal(tlist.get_field("spans"), one_t.get_field("spans"))
    assert with_rows == 1 and len(batch) == 2                     # the second segment has no instances: all rows zero
    plain = tspn.dataset.proposal_pair_lists(loader_segs, **kw)
    assert not plain[0][1].has_field("span_labels") and torch.equal(plain[0][1].target, batch[0][1].target)
    with pytest.raises(ValueError, match="span_labels=True needs"):
        tspn.dataset.proposal_pair_lists(loader_segs, span_labels=True, **dict(kw, max_spans=0))
    # [P,F] samples through a model with the switch on: the loss of the same model with the switch off, bit for bit
    losses = []
    for on in (False, True):
        cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": False, "PREDICT.FEATURE_DIM": 40,
                                    "PREDICT.PREDICATE_NUM": case["K"]})
        cfg.RELPN.DPN.POOL_GT_SPAN = on
        torch.manual_seed(0)
        model = tspn.BaseModel(cfg).to(device).train()
        loss = model([b[0] for b in batch], [b[1] for b in batch])
        losses.append(loss["loss_rel"].detach())
    assert torch.equal(losses[0], losses[1])
