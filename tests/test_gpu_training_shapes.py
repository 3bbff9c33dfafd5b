"""The training step (model.py: _LinearFn, _MatmulNTFn, _PredicateHeadFn, _TemporalHeadsDenseFn,
_TemporalHeadsTrackletFn, _conv3_weight_grad, _heads_backward) beyond one tile: more pairs than one PAIR_BLOCK, odd and
single-frame segments, contractions with several splits, D % 16 != 0, explicit pair tables, several segments per step,
accumulated gradients, every direct-conv variant in both roles of the dense backward, an empty batch.

Reference: the float64 torch-autograd restatement (tests/train_reference.py; F.conv1d + 1x1 conv for the dense
function).  Tolerances are those of tests/test_gpu_model.py: parameter gradients atol = 2e-4 max|ref| + 1e-9 (tracklet
step), 2e-5 max(1, max|ref|) (dense function and the three small functions), losses rtol = 2e-5."""
import importlib

import numpy as np
import pytest
import torch

import cases
import oracle
from train_reference import t, train_reference_segments

pytestmark = pytest.mark.gpu

A, K = 4, 132


def model_module(tspn):
    return importlib.import_module(tspn.BaseModel.__module__)


def lib_splits(tspn, P, F, K_):
    """choose_splits of the library's split-K GEMM for a [P,F] x [K_,F]^T product, read off its workspace size."""
    return tspn._abi.lib().tspn_predicate_head_workspace_bytes(P, F, K_) // (P * K_ * 4)


def temporal_model(tspn, device, D, sd):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D})
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    return model.to(device).train()


def make_segment(tspn, seed, N, T, D, pairs=None):
    """(video, pairs, gt_dur, gt_rel, targets) of one tracklet segment; `pairs` None = the canonical table."""
    v = tspn.synth.make_video(seed, N, T, D)
    explicit = pairs is not None
    pairs = oracle.pair_index(N) if pairs is None else t(pairs)
    P = pairs.shape[0]
    gt_dur = t((tspn.hashrng.uniform(seed, "gt_dur", (P, 2 * A, T)) < 0.3).astype(np.float32))
    gt_rel = t((tspn.hashrng.uniform(seed, "gt_rel", (P, A, T)) < 0.3).astype(np.float32))
    targets = t((tspn.hashrng.uniform(seed, "tg", (P, K)) < 0.05).astype(np.float32))
    return {"v": v, "pairs": pairs, "explicit": explicit, "gt_dur": gt_dur, "gt_rel": gt_rel, "targets": targets}


def lists_of(tspn, device, segs):
    plists, tlists = [], []
    for s in segs:
        v = s["v"]
        pl = tspn.PairList.from_tracklets(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), t(v["track_cls_logits"]))
        if s["explicit"]:
            pl.add_field("tracklet_pairs", s["pairs"])
        tl = tspn.TargetList(s["targets"])
        tl.add_field("duration", s["gt_dur"])
        tl.add_field("relness", s["gt_rel"])
        plists.append(pl.to(device))
        tlists.append(tl.to(device))
    return plists, tlists


def grads_of(model):
    h = model.relpn.duration_proposal_network.dpn_head
    return {"conv_w": h.conv.weight.grad, "conv_b": h.conv.bias.grad,
            "dur_w": h.duration_pred.weight.grad, "dur_b": h.duration_pred.bias.grad,
            "rel_w": h.relness_pred.weight.grad, "rel_b": h.relness_pred.bias.grad,
            "cls_w": model.classifier.rel_predictor.weight.grad, "cls_b": model.classifier.rel_predictor.bias.grad}


def reference(segs, sd):
    return train_reference_segments([(s["v"], s["pairs"], s["gt_dur"], s["gt_rel"], s["targets"]) for s in segs], sd)


def check_step(what, loss, got, ref_loss, ref_grad, times=1):
    assert set(loss) == {"loss_duration", "loss_relationness", "loss_rel"} == set(ref_loss)
    for k in ref_loss:
        print(f"{what}: {k} {loss[k].item():.8g} vs {ref_loss[k]:.8g}")
        np.testing.assert_allclose(loss[k].item(), ref_loss[k], rtol=2e-5, err_msg=f"{what}: {k}")
    for k, gq in got.items():
        r = times * ref_grad[k].numpy()
        err = float(np.abs(gq.cpu().numpy() - r).max())
        print(f"{what}: d{k} max|ref| {np.abs(r).max():.3g}, error {err / np.abs(r).max():.2e} of it")
        np.testing.assert_allclose(gq.cpu().numpy(), r, rtol=0, atol=2e-4 * np.abs(r).max() + 1e-9, err_msg=f"{what}: {k}")


# ------------------------------------------------------------------------------------------------ tracklet form
@pytest.mark.parametrize("D,N,T", [
    (16, 17, 14),     # 272 pairs: one full PAIR_BLOCK and a ragged block of 16
    (32, 9, 33),      # odd T, T % 4 != 0
    (64, 6, 150),     # N T = 900: the weight-gradient GEMMs run with several splits (asserted below)
    (16, 3, 1),       # one frame
    (24, 5, 12),      # D % 16 != 0: the channels-last conv refuses it; transpose + direct kernel, as in eval
])
def test_tracklet_training_step_shapes(tspn, device, D, N, T):
    """Losses and every parameter gradient of one step on a tracklet segment against float64 autograd."""
    if (D, N, T) == (16, 17, 14):
        assert model_module(tspn)._TemporalHeadsTrackletFn.PAIR_BLOCK == 256 and N * (N - 1) == 256 + 16
    if (D, N, T) == (64, 6, 150):
        C, H, P = 2 * D, 3 * A, N * (N - 1)
        assert lib_splits(tspn, 2 * D, N * T, D) == 14        # _conv3_weight_grad: dU [C, N T] . X_k [D, N T]^T, 2 tiles
        assert lib_splits(tspn, H, P * T, C) == 64            # d_head_w: g [H, P T] . act [C, P T]^T, one tile
        assert lib_splits(tspn, P * T, H, C) == 1             # dZ: g^T [P T, H] . head_w^T [C, H]^T, 71 row tiles
    sd = tspn.synth.make_weights(3, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, device, D, sd)
    segs = [make_segment(tspn, 800 + D + N + T, N, T, D)]
    loss = model(*lists_of(tspn, device, segs))
    sum(loss.values()).backward()
    ref_loss, ref_grad = reference(segs, sd)
    check_step(f"D={D} N={N} T={T}", loss, grads_of(model), ref_loss, ref_grad)


def test_tracklet_training_explicit_pair_table(tspn, device, monkeypatch):
    """An explicit `tracklet_pairs` table of 300 rows (two PAIR_BLOCKs) with repeated pairs, a tracklet that is never a
    subject and one that is never an object: gradients against float64, and the rows of dU / dV of those two tracklets
    (what _TemporalHeadsTrackletFn.backward hands to the weight-gradient contraction) are exactly zero."""
    D, N, T = 16, 8, 10
    never_subject, never_object = 5, 2
    rs = np.random.RandomState(11)
    subj = rs.choice([i for i in range(N) if i != never_subject], size=300)
    obj = rs.choice([i for i in range(N) if i != never_object], size=300)
    pairs = np.stack([subj, obj], axis=1).astype(np.int64)
    pairs[7] = pairs[3]
    pairs[299] = pairs[3]                                       # a repeated pair across the two blocks
    assert len(pairs) > 256 and len({tuple(p) for p in pairs}) < len(pairs)
    mod = model_module(tspn)
    seen, orig = [], mod._conv3_weight_grad
    monkeypatch.setattr(mod, "_conv3_weight_grad", lambda x, dz: (seen.append(dz.detach().clone()), orig(x, dz))[1])
    sd = tspn.synth.make_weights(4, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, device, D, sd)
    segs = [make_segment(tspn, 820, N, T, D, pairs=pairs)]
    loss = model(*lists_of(tspn, device, segs))
    sum(loss.values()).backward()
    ref_loss, ref_grad = reference(segs, sd)
    check_step("explicit pair table", loss, grads_of(model), ref_loss, ref_grad)
    du, dv = (x.cpu().numpy() for x in seen)
    assert du.shape == dv.shape == (N, 2 * D, T)
    assert not du[never_subject].any() and not dv[never_object].any()
    assert all(du[i].any() for i in range(N) if i != never_subject)
    assert all(dv[i].any() for i in range(N) if i != never_object)


def test_tracklet_training_two_segments_and_accumulated_gradients(tspn, device):
    """Two segments of different (N, T) in one step (each loss is the sum over the segments), then a second backward()
    without zero_grad(): the gradients add to twice the single-call gradient, within the same tolerance."""
    D = 16
    sd = tspn.synth.make_weights(5, c=2 * D, bias_std=0.05)
    model = temporal_model(tspn, device, D, sd)
    segs = [make_segment(tspn, 830, 6, 14, D), make_segment(tspn, 831, 4, 9, D)]
    loss = model(*lists_of(tspn, device, segs))
    total = sum(loss.values())
    total.backward(retain_graph=True)
    ref_loss, ref_grad = reference(segs, sd)
    check_step("two segments", loss, {k: g.clone() for k, g in grads_of(model).items()}, ref_loss, ref_grad)
    total.backward()
    check_step("two segments, second backward", loss, grads_of(model), ref_loss, ref_grad, times=2)


# ------------------------------------------------------------------------------------------------ dense form
@pytest.mark.parametrize("P,C,T,H", [
    (3, 130, 20, 12),     # M % 4 != 0: conv3_mfma_kernel<false>
    (2, 136, 33, 12),     # C % 8 == 0, not % 16: conv3_mfma_dma_kernel<8>; odd T
    (2, 128, 150, 12),    # C % 16 == 0: conv3_mfma_dma_kernel<16>; 300 columns = three 128-column tiles
    (3, 132, 9, 12),      # M % 4 == 0, C % 8 != 0: conv3_mfma_kernel<true>
    (3, 24, 1, 12),       # T = 1
    (4, 40, 16, 3),       # H = 3
    (4, 48, 16, 16),      # H = 16
])
def test_dense_training_function_every_conv_variant(tspn, device, P, C, T, H):
    """_TemporalHeadsDenseFn: output, input gradient and parameter gradients against float64 autograd of
    relpn/dpn.py:69-73.  The conv is square (C -> C), so the forward conv, its recomputation and the flipped,
    role-swapped input-gradient conv all run the variant the row names.  Weights are scaled by 1/sqrt(fan-in) so that
    activations stay O(1) at every depth."""
    rs = np.random.RandomState(100 + C + T + H)
    mk = lambda *shape: torch.from_numpy(rs.randn(*shape).astype(np.float32))   # noqa: E731
    x, cw, cb = mk(P, C, T), mk(C, C, 3) / np.sqrt(3 * C), 0.1 * mk(C)
    hw, hb, gout = mk(H, C) / np.sqrt(C), 0.1 * mk(H), mk(P, H, T)
    dev_in = [v.clone().to(device).requires_grad_(True) for v in (x, cw, cb, hw, hb)]
    out = model_module(tspn)._TemporalHeadsDenseFn.apply(*dev_in)
    out.backward(gout.to(device))
    ref_in = [v.clone().double().requires_grad_(True) for v in (x, cw, cb, hw, hb)]
    act = torch.relu(torch.nn.functional.conv1d(ref_in[0], ref_in[1], ref_in[2], padding=1))
    ref = torch.nn.functional.conv1d(act, ref_in[3].unsqueeze(2), ref_in[4])
    ref.backward(gout.double())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-5)
    for name, a, b in zip(("x", "conv_w", "conv_b", "head_w", "head_b"), dev_in, ref_in):
        scale = max(1.0, float(b.grad.abs().max()))
        err = float((a.grad.cpu().double() - b.grad).abs().max())
        print(f"P={P} C={C} T={T} H={H}: d{name} max|ref| {float(b.grad.abs().max()):.3g}, error {err:.2e}")
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=0, atol=2e-5 * scale, err_msg=name)


# ------------------------------------------------------------------------------------------------ the three small functions
M_ROWS, N_OUT, K_IN = 200, 150, 170


def _small_operands(device, rows):
    rs = np.random.RandomState(7)
    x = torch.from_numpy(rs.uniform(-1, 1, (rows, K_IN)).astype(np.float32))
    w = torch.from_numpy((rs.randn(N_OUT, K_IN) / np.sqrt(K_IN)).astype(np.float32))
    b = torch.from_numpy((0.1 * rs.randn(N_OUT)).astype(np.float32))
    g = torch.from_numpy(rs.randn(rows, N_OUT).astype(np.float32))
    return x, w, b, g


def _compare(name, dev_in, ref_in, out, ref):
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-5, err_msg=name)
    for tag, a, b in zip("abc", dev_in, ref_in):
        assert a.grad is not None and a.grad.shape == b.grad.shape, f"{name}: operand {tag}"
        scale = max(1.0, float(b.grad.abs().max())) if b.grad.numel() else 1.0
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=0, atol=2e-5 * scale,
                                   err_msg=f"{name}: gradient of operand {tag}")


@pytest.mark.parametrize("fn", ["linear", "matmul_nt", "predicate_head"])
@pytest.mark.parametrize("rows", [M_ROWS, 0])
def test_small_training_functions_beyond_one_tile(tspn, device, fn, rows):
    """_LinearFn / _MatmulNTFn / _PredicateHeadFn with [200,170] x [150,170]^T: the forward product, dx = g W and
    dW = g^T x each have more than one row tile, more than one column tile (width > 144) and more than one split.
    rows = 0 is the empty batch: empty output, zero parameter gradients, no launch error."""
    assert lib_splits(tspn, M_ROWS, K_IN, N_OUT) == 2       # forward: 4 x 2 tiles, F = 170
    assert lib_splits(tspn, M_ROWS, N_OUT, K_IN) == 2       # dx:      4 x 2 tiles, F = 150
    assert lib_splits(tspn, N_OUT, M_ROWS, K_IN) == 3       # dW:      3 x 2 tiles, F = 200
    mod = model_module(tspn)
    x, w, b, g = _small_operands(device, rows)
    if fn == "matmul_nt":
        ops_in = (x, w)
        apply, plain = mod._MatmulNTFn.apply, lambda a, b_: a @ b_.t()
    elif fn == "linear":
        ops_in = (x, w, b)
        apply, plain = mod._LinearFn.apply, lambda a, w_, b_: a @ w_.t() + b_
    else:
        ops_in = (x, w, b)
        apply, plain = mod._PredicateHeadFn.apply, lambda a, w_, b_: torch.sigmoid(a @ w_.t() + b_)
    dev_in = [v.clone().to(device).requires_grad_(True) for v in ops_in]
    ref_in = [v.clone().double().requires_grad_(True) for v in ops_in]
    out, ref = apply(*dev_in), plain(*ref_in)
    assert out.shape == (rows, N_OUT)
    out.backward(g.to(device))
    ref.backward(g.double())
    _compare(f"{fn} rows={rows}", dev_in, ref_in, out, ref)
    if rows == 0:
        assert all(float(a.grad.abs().sum()) == 0.0 for a in dev_in)


def test_ppn_training_two_segments(tspn, device):
    """USE_PPN training with two segments in the batch (loss_pair and loss_rel are sums over the segments): losses and
    the gradients of both MLPs against float64 autograd of ppn.py:92-112, 57-71."""
    g = cases.load("g2_ppn_n32.npz")
    c = cases.g2_inputs(int(g["input_seed"]))
    model = tspn.BaseModel(cases.baseline_cfg(**{"RELPN.USE_PPN": True, "PREDICT.FEATURE_DIM": 64}))
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in c["state_dict"].items() if k in own})
    model.to(device).train()
    cls_of = [c["cls"], (0.5 * c["cls"][::-1] + 0.25).astype(np.float32)]

    def sample(cls):
        plist = tspn.PairList(t(c["feats"]))
        plist.add_field("track_cls_logits", t(cls))
        plist.add_field("tracklet_pairs", c["pairs"])
        plist.add_field("num_tracklets", np.int64(c["n"]))
        return plist

    tl = tspn.TargetList(t(c["targets"]))
    loss = model([sample(x).to(device) for x in cls_of], [tl.to(device), tl.to(device)])
    assert set(loss) == {"loss_pair", "loss_rel"}
    sum(loss.values()).backward()
    pre = "relpn.pair_proposal_network.ppn_head."
    sd = {k: t(v).double().requires_grad_(True) for k, v in c["state_dict"].items()
          if k.startswith(pre) or k.startswith("classifier.")}
    gt = tspn.PPN._gt_matrices([sample(cls_of[0])], [tl])[0].double()
    ref_pair = 0
    for cls in cls_of:
        x = t(cls).double()
        mlp = lambda name: torch.relu(x @ sd[pre + name + ".0.weight"].t() + sd[pre + name + ".0.bias"]) \
            @ sd[pre + name + ".2.weight"].t() + sd[pre + name + ".2.bias"]   # noqa: E731
        ref_pair = ref_pair + torch.nn.functional.binary_cross_entropy(torch.sigmoid(mlp("sub_emb") @ mlp("obj_emb").t()), gt)
    logit = torch.sigmoid(t(c["feats"]).double() @ sd["classifier.rel_predictor.weight"].t() + sd["classifier.rel_predictor.bias"])
    ref_rel = 2 * torch.nn.functional.binary_cross_entropy(logit, t(c["targets"]).double())
    (ref_pair + ref_rel).backward()
    np.testing.assert_allclose(loss["loss_pair"].item(), float(ref_pair), rtol=2e-5)
    np.testing.assert_allclose(loss["loss_rel"].item(), float(ref_rel), rtol=2e-5)
    head = dict(model.relpn.pair_proposal_network.ppn_head.named_parameters())
    for name in ("sub_emb.0.weight", "sub_emb.0.bias", "sub_emb.2.weight", "sub_emb.2.bias",
                 "obj_emb.0.weight", "obj_emb.0.bias", "obj_emb.2.weight", "obj_emb.2.bias"):
        want = sd[pre + name].grad
        assert float((head[name].grad.cpu().double() - want).abs().max()) <= 2e-7 + 1e-5 * float(want.abs().max()), name
    for name, p in (("weight", model.classifier.rel_predictor.weight), ("bias", model.classifier.rel_predictor.bias)):
        want = sd["classifier.rel_predictor." + name].grad
        assert float((p.grad.cpu().double() - want).abs().max()) <= 2e-7 + 1e-5 * float(want.abs().max()), name
