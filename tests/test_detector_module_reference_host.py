"""The detector-module reference and its bounds are sound before anything runs on a device.

tests/detector_module_reference.py returns hand-worked values exactly on integer cases, and a plain fp32 evaluation on
the CPU (torch.nn.functional.conv2d and `@` in float32: a correct implementation, in some summation order) stays inside
the envelope the reference computes, at every shape the device tests use.  The largest error / bound ratio is printed."""
import pytest
import torch
import torch.nn.functional as F

import detector_module_reference as dm


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1)


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape)
    assert bool((bound > 0).all())                       # every bias is non-zero: no element has a free pass
    return float((err / bound).max()), bool((err <= bound).all())


def test_rpn_head_hand_worked():
    # one pixel, two channels, one anchor: t = relu(x + cb) = (relu(3 - 5), relu(4 + 1)) = (0, 5)
    eye = torch.zeros((2, 2, 3, 3))
    eye[0, 0, 1, 1] = eye[1, 1, 1, 1] = 1
    sd = {"conv.weight": eye, "conv.bias": torch.tensor([-5.0, 1.0]),
          "objectness_logits.weight": torch.tensor([[2.0, 3.0]]).view(1, 2, 1, 1), "objectness_logits.bias": torch.tensor([7.0]),
          "anchor_deltas.weight": torch.tensor([[1.0, 0], [0, 1], [1, 1], [0, -2]]).view(4, 2, 1, 1),
          "anchor_deltas.bias": torch.tensor([10.0, 20.0, 30.0, 40.0])}
    x = torch.tensor([3.0, 4.0]).view(1, 1, 1, 2)
    for dtype in (torch.float32, torch.bfloat16):
        lg, dl = dm.rpn_head(x, sd, dtype)
        assert lg.dtype == dl.dtype == torch.float64
        assert lg.reshape(-1).tolist() == [22.0] and dl.reshape(-1).tolist() == [10.0, 25.0, 35.0, 30.0]
    # a 3x3 tap reaches the neighbour: weight on tap (0, 2) of channel 0 reads the pixel above and to the right
    w = torch.zeros((1, 1, 3, 3))
    w[0, 0, 0, 2] = 1
    sd = {"conv.weight": w, "conv.bias": torch.tensor([0.5]),
          "objectness_logits.weight": torch.ones((1, 1, 1, 1)), "objectness_logits.bias": torch.tensor([1.0]),
          "anchor_deltas.weight": torch.tensor([1.0, 2, 3, 4]).view(4, 1, 1, 1), "anchor_deltas.bias": torch.zeros(4)}
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).view(1, 2, 2, 1)
    lg, dl = dm.rpn_head(x, sd, torch.float32)
    assert lg.reshape(-1).tolist() == [1.5, 1.5, 3.5, 1.5]             # only pixel (1, 0) has a neighbour at (0, 1) = 2
    assert dl[0, 1, 0].tolist() == [2.5, 5.0, 7.5, 10.0]


@pytest.mark.parametrize("channels,anchors,shape", [(96, 7, (2, 5, 7)), (96, 15, (1, 3, 2)), (32, 3, (1, 1, 1))])
def test_rpn_head_exact_case(channels, anchors, shape):
    x, sd, want_lg, want_dl = dm.rpn_exact_case(channels, anchors, shape)
    assert len(set(sd["objectness_logits.bias"].tolist() + sd["anchor_deltas.bias"].tolist())) == 5 * anchors
    assert float(x.min()) >= 0 and bool((x + sd["conv.bias"] < 0).any())      # the ReLU cuts somewhere
    lg, dl = dm.rpn_head(x, sd, torch.float32)
    assert torch.equal(lg, want_lg) and torch.equal(dl, want_dl)
    lg, dl = dm.rpn_head(x, sd, torch.bfloat16)                               # small integers are bf16 values
    assert torch.equal(lg, want_lg) and torch.equal(dl, want_dl)


def test_box_predictor_hand_worked_and_exact_case():
    sd = {"cls_score.weight": torch.tensor([[1.0, 0, 0], [0, 2, 0]]), "cls_score.bias": torch.tensor([1.0, -1.0]),
          "bbox_pred.weight": torch.tensor([[0.0, 0, 1], [1, 1, 1], [0, -1, 0], [3, 0, 0]]),
          "bbox_pred.bias": torch.tensor([0.5, 0.0, 2.0, -3.0])}
    cls, dl = dm.box_predictor(torch.tensor([[1.0, 2, 3], [4, 5, 6]]), sd)
    assert cls.tolist() == [[2.0, 3.0], [5.0, 9.0]] and dl.tolist() == [[3.5, 6.0, 0.0, 0.0], [6.5, 15.0, -3.0, 9.0]]
    for r, c, k in ((65, 2048, 35), (300, 64, 1)):
        x, sd, want_cls, want_dl = dm.predictor_exact_case(r, c, k)
        cls, dl = dm.box_predictor(x, sd)
        assert tuple(cls.shape) == (r, k + 1) and tuple(dl.shape) == (r, 4 * k)
        assert torch.equal(cls, want_cls) and torch.equal(dl, want_dl)


def test_pixel_normalise_by_channel():
    img = torch.tensor([[[[10.0, 20.0, 30.0]]]])
    assert dm.pixel_normalise(img, (2.0, 4.0, 6.0), (2.0, 4.0, 8.0)).reshape(-1).tolist() == [4.0, 4.0, 3.0]


def _rpn_shapes(channels):
    return [(channels, a, m) for a in dm.RPN_ANCHORS for m in dm.RPN_MAPS] + [dm.RPN_WIDE]


def _fp32_rpn(x, sd, bf16):
    """A plain fp32 evaluation; bf16: on bf16-rounded operands, with the two roundings."""
    r = (lambda v: v.to(torch.bfloat16).float()) if bf16 else (lambda v: v)
    t = r(F.relu(F.conv2d(_nchw(r(x)), r(sd["conv.weight"]), sd["conv.bias"], padding=1)))
    lg = r(F.conv2d(t, r(sd["objectness_logits.weight"]), sd["objectness_logits.bias"]))
    dl = r(F.conv2d(t, r(sd["anchor_deltas.weight"]), sd["anchor_deltas.bias"]))
    return _nhwc(lg), _nhwc(dl)


@pytest.mark.parametrize("bf16", [False, True])
def test_plain_fp32_rpn_head_is_inside_the_bound(tspn, bf16, capsys):
    worst = 0.0
    for channels, anchors, shape in _rpn_shapes(64 if bf16 else 32):
        sd = dm.rpn_weights(tspn.hashrng, 93, channels, anchors)
        x = torch.from_numpy(tspn.hashrng.uniform(94, "x", (*shape, channels), -1, 1))
        ref = dm.rpn_head_with_bounds(x, sd, torch.bfloat16 if bf16 else torch.float32)
        lg, dl = _fp32_rpn(x, sd, bf16)
        for got, name in ((lg, "logits"), (dl, "deltas")):
            ratio, ok = _ratio(got, ref["raw_" + name], ref[name + "_bound"])
            assert ok, (channels, anchors, shape, name, ratio)
            worst = max(worst, ratio)
        if bf16:                                          # the reference's own rounded form is that close as well
            assert bool(((ref["logits"] - ref["raw_logits"]).abs() <= dm.H16 * ref["raw_logits"].abs()).all())
    with capsys.disabled():
        print(f"\nrpn_head {'bf16' if bf16 else 'fp32'}: largest |plain fp32 - reference| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_plain_fp32_box_predictor_is_inside_the_bound(tspn, capsys):
    worst = 0.0
    for r, c, k in dm.PREDICTOR_SHAPES:
        sd = dm.predictor_weights(tspn.hashrng, 95, c, k)
        x = torch.from_numpy(tspn.hashrng.normal(96, "x", (r, c), std=1.0))
        cls, dl, bc, bd = dm.box_predictor_with_bounds(x, sd)
        got = (x @ sd["cls_score.weight"].T + sd["cls_score.bias"], x @ sd["bbox_pred.weight"].T + sd["bbox_pred.bias"])
        for g, w, b in zip(got, (cls, dl), (bc, bd)):
            ratio, ok = _ratio(g, w, b)
            assert ok, (r, c, k, ratio)
            worst = max(worst, ratio)
    with capsys.disabled():
        print(f"\nbox_predictor: largest |plain fp32 - reference| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_the_bounds_would_catch_a_wrong_channel(tspn):
    """The envelope is narrow enough to tell a permuted channel, a missing ReLU or a lost bias from rounding."""
    sd = dm.rpn_weights(tspn.hashrng, 93, 32, 7)
    x = torch.from_numpy(tspn.hashrng.uniform(94, "x", (2, 5, 7, 32), -1, 1))
    ref = dm.rpn_head_with_bounds(x, sd, torch.float32)
    y = torch.cat([ref["logits"], ref["deltas"]], dim=3)
    shifted = y[..., 6:34]                                                   # the delta split one channel early
    assert bool(((shifted - ref["deltas"]).abs() > ref["deltas_bound"]).any())
    no_bias = dict(sd, **{"objectness_logits.bias": torch.zeros(7)})
    assert bool(((dm.rpn_head(x, no_bias)[0] - ref["logits"]).abs() > ref["logits_bound"]).all())
    no_relu = dm._nhwc(F.conv2d(F.conv2d(dm._nchw(x), sd["conv.weight"].double(), sd["conv.bias"].double(), padding=1),
                                sd["objectness_logits.weight"].double(), sd["objectness_logits.bias"].double()))
    assert bool(((no_relu - ref["logits"]).abs() > ref["logits_bound"]).any())
