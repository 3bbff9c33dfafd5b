"""detector.py against references, module by module and hand-over by hand-over.

`RPNHead` and `BoxPredictor` must lie inside the envelopes of tests/detector_module_reference.py (float64 from the
separate weights; DESIGN.md 3 "Detector module bounds") and EQUAL it on integer cases.  One forward pass of
`FasterRCNNC4` is recorded by forward hooks on its four stages and every tensor that flowed is held to something
independent: bounded stages to their float64 references, exact stages to the restatement of
tests/detector_reference.py fed the device's own upstream tensors.  No tolerance here comes from a device result."""
import numpy as np
import pytest
import torch

import detector_module_reference as dm
import detector_reference as ref
from oracle import roi_head_oracle as ro

pytestmark = pytest.mark.gpu

K, D, R, PRE, THR = 35, 20, 40, 6000, 0.01
MEAN, STD = (100.0, 110.0, 120.0), (60.0, 61.0, 62.0)
BLOCKS, RES5 = (1, 1, 1), (64, 128, 1)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _inside(got, want, bound, what):
    """Every element of `got` within `bound` of `want`; prints the largest error / bound."""
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape), (what, got.shape, want.shape)
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all()) and bool((bound > 0).all())
    ratio = float((err / bound).max())
    print(f"{what}: max error / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


def _rpn_head(tspn, device, sd, channels, anchors):
    head = tspn.RPNHead(channels, anchors)
    head.load_state_dict(sd, strict=True)
    return head.to(device)


def _predictor(tspn, device, sd, channels, classes):
    pred = tspn.BoxPredictor(channels, classes)
    pred.load_state_dict(sd, strict=True)
    return pred.to(device)


def _check_rpn_head(got, x, sd, bf16, what):
    want = dm.rpn_head_with_bounds(x.float(), sd, torch.bfloat16 if bf16 else torch.float32)
    lg, dl = got
    assert lg.dtype == dl.dtype == torch.float32 and lg.is_contiguous() and dl.is_contiguous()
    _inside(lg, want["raw_logits"], want["logits_bound"], what + " logits")
    _inside(dl, want["raw_deltas"], want["deltas_bound"], what + " deltas")
    if bf16:                                     # the head's output is rounded to bf16 once
        assert torch.equal(lg, lg.bfloat16().float()) and torch.equal(dl, dl.bfloat16().float())


# ------------------------------------------------------------------------------------------------------ a. RPNHead
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", dm.RPN_MAPS)
@pytest.mark.parametrize("anchors", dm.RPN_ANCHORS)
def test_rpn_head_inside_the_reference_bound(tspn, device, anchors, shape, bf16):
    channels = 64 if bf16 else 32
    sd = dm.rpn_weights(tspn.hashrng, 93, channels, anchors)
    x = torch.from_numpy(tspn.hashrng.uniform(94, "x", (*shape, channels), -1, 1))
    x = x.bfloat16() if bf16 else x
    got = _rpn_head(tspn, device, sd, channels, anchors)(x.to(device))
    assert tuple(got[0].shape) == (*shape, anchors) and tuple(got[1].shape) == (*shape, 4 * anchors)
    _check_rpn_head(got, x, sd, bf16, f"RPNHead A={anchors} {shape} {'bf16' if bf16 else 'fp32'}")


@pytest.mark.parametrize("bf16", [False, True])
def test_rpn_head_at_the_detector_width(tspn, device, bf16):
    channels, anchors, shape = dm.RPN_WIDE
    sd = dm.rpn_weights(tspn.hashrng, 93, channels, anchors)
    x = torch.from_numpy(tspn.hashrng.uniform(94, "x", (*shape, channels), -1, 1))
    x = x.bfloat16() if bf16 else x
    got = _rpn_head(tspn, device, sd, channels, anchors)(x.to(device))
    _check_rpn_head(got, x, sd, bf16, f"RPNHead C={channels} {'bf16' if bf16 else 'fp32'}")


@pytest.mark.parametrize("anchors,shape", [(7, (2, 5, 7)), (15, (3, 9, 13)), (3, (1, 1, 1))])
def test_rpn_head_exact_on_integers(tspn, device, anchors, shape):
    """Centre-tap identity conv, one-hot head rows on distinct channels, distinct integer biases: a wrong channel, a shifted
    split or a lost ReLU is a wrong integer."""
    x, sd, want_lg, want_dl = dm.rpn_exact_case(96, anchors, shape)
    lg, dl = _rpn_head(tspn, device, sd, 96, anchors)(x.to(device))
    rl, rd = dm.rpn_head(x, sd, torch.float32)
    assert torch.equal(rl, want_lg) and torch.equal(rd, want_dl)
    assert torch.equal(lg.cpu().double(), rl) and torch.equal(dl.cpu().double(), rd)


# ------------------------------------------------------------------------------------------------- b. BoxPredictor
@pytest.mark.parametrize("rows,channels,classes", dm.PREDICTOR_SHAPES)
def test_box_predictor_inside_the_reference_bound(tspn, device, rows, channels, classes):
    sd = dm.predictor_weights(tspn.hashrng, 95, channels, classes)
    x = torch.from_numpy(tspn.hashrng.normal(96, "x", (rows, channels), std=1.0))
    cls, dl = _predictor(tspn, device, sd, channels, classes)(x.to(device))
    want_cls, want_dl, bc, bd = dm.box_predictor_with_bounds(x, sd)
    assert cls.dtype == dl.dtype == torch.float32 and cls.is_contiguous() and dl.is_contiguous()
    _inside(cls, want_cls, bc, f"BoxPredictor cls R={rows} C={channels} K={classes}")
    _inside(dl, want_dl, bd, f"BoxPredictor deltas R={rows} C={channels} K={classes}")


@pytest.mark.parametrize("rows,channels,classes", [(65, 2048, 35), (300, 64, 1), (1000, 2048, 1)])
def test_box_predictor_exact_on_integers(tspn, device, rows, channels, classes):
    x, sd, want_cls, want_dl = dm.predictor_exact_case(rows, channels, classes)
    cls, dl = _predictor(tspn, device, sd, channels, classes)(x.to(device))
    rc, rd = dm.box_predictor(x, sd)
    assert torch.equal(rc, want_cls) and torch.equal(rd, want_dl)
    assert torch.equal(cls.cpu().double(), rc) and torch.equal(dl.cpu().double(), rd)


def test_box_predictor_without_rows(tspn, device):
    pred = _predictor(tspn, device, dm.predictor_weights(tspn.hashrng, 95, 64, 35), 64, 35)
    cls, dl = pred(torch.zeros((0, 64), device=device))
    assert tuple(cls.shape) == (0, 36) and tuple(dl.shape) == (0, 140) and cls.is_cuda and dl.is_cuda


# ------------------------------------------------------------------------------------------- c. the forward, walked
def _widths(bf16):
    return (64, 256) if bf16 else (16, 64)


def _weights(tspn, stem_out, res2_out, seed=91):
    u = lambda name, shape, lo, hi: tspn.hashrng.uniform(seed, name, shape, lo, hi)       # noqa: E731
    nrm = lambda name, shape, std: tspn.hashrng.normal(seed, name, shape, std=std)         # noqa: E731
    c4 = res2_out * 4
    sd = {"backbone." + k: v for k, v in ro.make_backbone_weights(u, nrm, stem_out, res2_out, BLOCKS).items()}
    sd.update({"roi_heads." + k: v for k, v in ro.make_res5_weights(u, nrm, c4, *RES5).items()})
    # deltas of a few tenths and boxes e^1.5 times their anchors: the clip and the NMS leave a handful of proposals per
    # frame, so that fewer than D detections come out and the rows past both counts are exercised
    rpn = dm.rpn_weights(tspn.hashrng, seed, c4, 15, delta_gain=0.03, size_bias=1.5)
    sd.update({"proposal_generator.rpn_head." + k: v for k, v in rpn.items()})
    sd.update({"roi_heads.box_predictor." + k: v for k, v in dm.predictor_weights(tspn.hashrng, seed, RES5[1], K).items()})
    return sd


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _model(tspn, device, bf16, sd=None, seed=91, post=R):
    stem_out, res2_out = _widths(bf16)
    model = tspn.FasterRCNNC4(num_classes=K, blocks=BLOCKS, stem_out=stem_out, res2_out=res2_out, res5_bottleneck=RES5[0],
                              res5_out=RES5[1], res5_blocks=RES5[2], post_nms_topk=post, score_thresh=THR,
                              detections_per_image=D, pixel_mean=MEAN, pixel_std=STD, frame_chunk=2)
    sd = _weights(tspn, stem_out, res2_out, seed) if sd is None else sd
    model.load_state_dict(sd, strict=True)
    return model.to(device).eval(), sd


class _Tape:
    """Forward hooks on the four stages: what each was called with and what it returned, in call order."""

    def __init__(self, model):
        self.calls = {"backbone": [], "rpn_head": [], "roi_heads": [], "box_predictor": []}
        mods = {"backbone": model.backbone, "rpn_head": model.proposal_generator.rpn_head, "roi_heads": model.roi_heads,
                "box_predictor": model.roi_heads.box_predictor}
        self.handles = [m.register_forward_hook(self._hook(name), with_kwargs=True) for name, m in mods.items()]

    def _hook(self, name):
        def record(module, args, kwargs, output):
            keep = lambda v: v.detach().clone() if isinstance(v, torch.Tensor) else v          # noqa: E731
            out = tuple(keep(o) for o in output) if isinstance(output, tuple) else keep(output)
            self.calls[name].append((tuple(keep(a) for a in args), dict(kwargs), out))
        return record

    def close(self):
        for h in self.handles:
            h.remove()


_RUNS = {}


def _recorded_forward(tspn, device, bf16):
    """ONE model(images) under the hooks, shared by the tests that read it (nothing in it is modified afterwards)."""
    if bf16 not in _RUNS:
        model, sd = _model(tspn, device, bf16)
        img = torch.from_numpy(tspn.hashrng.uniform(92, "img", (3, 70, 100, 3), 0, 255))
        tape = _Tape(model)
        try:
            result = model(img.to(device), bf16=bf16)
        finally:
            tape.close()
        _RUNS[bf16] = (model, sd, img, tape.calls, result)
    return _RUNS[bf16]


def _proposals_restated(tspn, device, logits, deltas, sizes, post=R):
    """DESIGN.md 2 "proposals" on captured head outputs: the restatement's selection, the device's decode, the
    restatement's NMS -> (boxes [Tc,post,4], count [Tc]) as numpy."""
    lg_np, = host(logits)
    cand = ref.rpn_proposals_select(lg_np, PRE)
    cell = torch.from_numpy(ref.cell_anchors()).to(device)
    boxes, lg, valid = host(*tspn.ops.rpn_decode(torch.from_numpy(cand).to(device), logits, deltas, cell, 16.0,
                                                 torch.from_numpy(sizes).to(device)))
    ob, _, cnt = ref.rpn_proposals_finish(boxes, lg, valid, post, 0.7, 0.0)
    return ob, cnt


def _detections_restated(tspn, device, cls, dl, props, count, sizes):
    """DESIGN.md 2 "detections" on captured predictor outputs: the device's decode, the restatement's NMS and top-k."""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                        # noqa: E731
    sc, bx, vl = host(*tspn.ops.box_head_decode(cls, dl, to(props), to(count), to(sizes), THR, BOX_WEIGHTS))
    return ref.detections_finish(sc, bx, vl, 0.5, D)


def _walk_heads(tspn, device, calls, sd, maps, sizes, bf16, post=R):
    """Steps 3 - 8 on the recorded calls of one detect_from_maps over `maps` with per-frame `sizes` (numpy [T,2]); returns
    the restated result concatenated over the chunks and the restated proposals."""
    T = maps.shape[0]
    chunks = [(lo, min(lo + 2, T)) for lo in range(0, T, 2)]
    assert len(calls["rpn_head"]) == len(calls["roi_heads"]) == len(chunks) and len(calls["box_predictor"]) == T
    rpn_sd = _sub(sd, "proposal_generator.rpn_head.")
    pred_sd = _sub(sd, "roi_heads.box_predictor.")
    res5_sd = {k: v for k, v in _sub(sd, "roi_heads.").items() if k.startswith("res5.")}
    want, all_props, frame = [], [], 0
    for (lo, hi), rpn, roi in zip(chunks, calls["rpn_head"], calls["roi_heads"]):
        tc = hi - lo
        # 3. the RPN head read the backbone's maps of this chunk, bit for bit
        (x,), _, (logits, deltas) = rpn
        assert x.dtype == maps.dtype and torch.equal(x, maps[lo:hi])
        # 4. and returned logits and deltas inside the reference's envelope
        assert tuple(logits.shape) == (tc, 5, 7, 15) and tuple(deltas.shape) == (tc, 5, 7, 60)
        _check_rpn_head((logits, deltas), x.cpu(), rpn_sd, bf16, f"walk chunk {lo}: RPNHead")
        # 5. the RoI head received these maps and the restated proposals, transposed to [R, Tc, 4]
        props, count = _proposals_restated(tspn, device, logits, deltas, sizes[lo:hi], post)
        (fm, boxes), _, feats = roi
        assert fm.dtype == maps.dtype and torch.equal(fm, maps[lo:hi])
        assert tuple(boxes.shape) == (post, tc, 4) and boxes.dtype == torch.float32
        assert np.array_equal(boxes.cpu().numpy(), props.transpose(1, 0, 2))
        assert 0 < count.min() and count.max() <= post
        # 6. and returned the res5 features of every (proposal, frame), rows past the count included
        assert tuple(feats.shape) == (post, tc, RES5[1]) and feats.dtype == maps.dtype
        if bf16:
            fref = ro.res5_roi_head_bf16(fm.cpu(), boxes.cpu(), res5_sd, num_blocks=RES5[2])
            scale = float(fref.abs().max())
            err = (feats.cpu().float() - fref).abs()
            assert float(err.max()) <= 4 * 2.0 ** -8 * scale, (float(err.max()), scale)
            assert float((err <= 2.0 ** -8 * fref.abs() + 1e-6).double().mean()) > 0.97
        else:
            fref = ro.res5_roi_head(fm.cpu(), boxes.cpu(), res5_sd, num_blocks=RES5[2], dtype=torch.float64)
            scale = float(fref.abs().max())
            np.testing.assert_allclose(feats.cpu().numpy(), fref.numpy(), rtol=0, atol=2e-5 * max(scale, 1.0))
        # 7. one predictor call per frame, on that frame's features as fp32, inside the linear layers' envelope
        cls, dl = [], []
        for i in range(tc):
            (px,), _, (pc, pd) = calls["box_predictor"][frame]
            assert px.dtype == torch.float32 and torch.equal(px, feats[:, i].float())
            want_c, want_d, bc, bd = dm.box_predictor_with_bounds(px, pred_sd)
            _inside(pc, want_c, bc, f"walk frame {frame}: cls_score")
            _inside(pd, want_d, bd, f"walk frame {frame}: bbox_pred")
            cls.append(pc)
            dl.append(pd)
            frame += 1
        # 8. the chunk's result, from the predictor outputs frame-major, the proposals and count of step 5
        want.append(_detections_restated(tspn, device, torch.cat(cls), torch.cat(dl), props, count, sizes[lo:hi]))
        all_props.append(props)
    return tuple(np.concatenate([w[k] for w in want]) for k in range(4)), np.concatenate(all_props)


def _equal_result(got, want):
    assert got[0].dtype == got[1].dtype == torch.float32 and got[2].dtype == got[3].dtype == torch.int64
    for g, w in zip(host(*got), want):
        assert g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("bf16", [False, True])
def test_forward_walked_hand_over_by_hand_over(tspn, device, bf16):
    model, sd, img, calls, result = _recorded_forward(tspn, device, bf16)
    T = img.shape[0]
    # 1. the backbone read (image - mean[c]) / std[c]: one correctly rounded subtraction and one division
    assert len(calls["backbone"]) == 1
    (x,), kwargs, maps = calls["backbone"][0]
    assert kwargs == {"bf16": bf16} and x.dtype == torch.float32
    norm = dm.pixel_normalise(img, MEAN, STD)
    assert tuple(x.shape) == tuple(norm.shape)
    assert bool(((x.cpu().double() - norm).abs() <= 3 * dm.U * norm.abs()).all())
    # 2. and returned the res4 maps of the reference's normalised frames
    bsd = _sub(sd, "backbone.")
    if bf16:
        mref = ro.resnet_c4_bf16(norm, bsd, BLOCKS)
        assert maps.dtype == torch.bfloat16 and tuple(maps.shape) == tuple(mref.shape) == (T, 5, 7, 1024)
        scale = float(mref.abs().max())
        err = (maps.cpu().float() - mref).abs()
        assert float(err.max()) <= 6 * 2.0 ** -8 * scale, (float(err.max()), scale)
        assert float((err <= 2.0 ** -7 * mref.abs() + 1e-3 * scale).double().mean()) > 0.97
    else:
        mref = ro.resnet_c4(norm, bsd, BLOCKS)
        assert maps.dtype == torch.float32 and tuple(maps.shape) == tuple(mref.shape) == (T, 5, 7, 256)
        scale = max(1.0, float(mref.abs().max()))
        np.testing.assert_allclose(maps.cpu().numpy(), mref.numpy(), rtol=0, atol=5e-5 * scale)
    # 3 - 8
    sizes = np.array([[70.0, 100.0]] * T, np.float32)
    want, _ = _walk_heads(tspn, device, calls, sd, maps, sizes, bf16)
    _equal_result(result, want)
    count = want[3]
    assert tuple(result[0].shape) == (T, D, 4) and count.sum() > 0 and count.min() < D     # zero rows are exercised
    for t in range(T):
        assert not want[0][t, count[t]:].any() and not want[1][t, count[t]:].any() and not want[2][t, count[t]:].any()


def test_walk_with_as_many_proposals_as_frames(tspn, device):
    """post_nms_topk = 2 on a chunk of two frames: [R, Tc, 4] and [Tc, R, 4] have one shape, so a hand-over that forgets
    a transpose still runs -- and must be seen.  The maps are the reference's, so nothing here rides on another forward."""
    small, sd = _model(tspn, device, False, post=2)
    img = torch.from_numpy(tspn.hashrng.uniform(92, "img", (2, 70, 100, 3), 0, 255))
    maps = ro.resnet_c4(dm.pixel_normalise(img, MEAN, STD), _sub(sd, "backbone."), BLOCKS).to(device)
    sizes = np.array([[70.0, 100.0], [64.0, 90.0]], np.float32)
    tape = _Tape(small)
    try:
        result = small.detect_from_maps(maps, torch.from_numpy(sizes).to(device))
    finally:
        tape.close()
    want, props = _walk_heads(tspn, device, tape.calls, sd, maps, sizes, False, post=2)
    _equal_result(result, want)
    assert not np.array_equal(props, props.transpose(1, 0, 2)) and want[3].sum() > 0


# --------------------------------------------------------------------------------------- d. per-frame image sizes
@pytest.mark.parametrize("bf16", [False, True])
def test_detect_from_maps_takes_each_frames_own_size(tspn, device, bf16):
    model, sd, _, calls, _ = _recorded_forward(tspn, device, bf16)
    maps = calls["backbone"][0][2]
    sizes = np.array([[70.0, 100.0], [64.0, 90.0], [50.0, 100.0]], np.float32)
    dsizes = torch.from_numpy(sizes).to(device)
    tape = _Tape(model)
    try:
        result = model.detect_from_maps(maps, dsizes)
    finally:
        tape.close()
    want, props = _walk_heads(tspn, device, tape.calls, sd, maps, sizes, bf16)
    _equal_result(result, want)
    # the case discriminates: under frame 0's size the restatement gives frames 1 and 2 other proposals and detections
    same = np.repeat(sizes[:1], 3, axis=0)
    wrong_props, wrong = [], []
    frame = 0
    for lo, rpn in zip((0, 2), tape.calls["rpn_head"]):
        p, c = _proposals_restated(tspn, device, rpn[2][0], rpn[2][1], same[lo:lo + 2])
        outs = tape.calls["box_predictor"][frame:frame + len(p)]
        frame += len(p)
        wrong_props.append(p)
        wrong.append(_detections_restated(tspn, device, torch.cat([o[2][0] for o in outs]), torch.cat([o[2][1] for o in outs]),
                                          p, c, same[lo:lo + 2]))
    wrong_props = np.concatenate(wrong_props)
    wrong_boxes = np.concatenate([w[0] for w in wrong])
    assert np.array_equal(wrong_props[0], props[0])
    for t in (1, 2):
        assert not np.array_equal(wrong_props[t], props[t]) and not np.array_equal(wrong_boxes[t], want[0][t])
        assert props[t][:, 2].max() <= sizes[t, 1] and props[t][:, 3].max() <= sizes[t, 0]
    # and a frame run alone with its own size gives its rows
    for t in range(3):
        alone = model.detect_from_maps(maps[t:t + 1], dsizes[t:t + 1])
        for g, w in zip(alone, result):
            assert torch.equal(g[0], w[t])


# ------------------------------------------------------------------------------------------------ e. weight caches
def _state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _cache_protocol(tspn, module, fresh, run, other_sd, loaders, touched):
    """`run(module)` -> tuple of tensors.  After every kind of parameter change the next run equals that of a freshly
    built module holding the new weights, bit for bit, and differs from the run before.  `touched`: names of the
    parameters to change in place; `loaders`: callables that load `other_sd` (one per route)."""
    before = run(module)
    params = dict(module.named_parameters())
    for name in touched:                                   # what an optimiser step does
        with torch.no_grad():
            params[name].mul_(2)
        after = run(module)
        assert _same(after, run(fresh(_state(module)))), name
        assert not _same(after, before), name
        before = after
    for load in loaders:                                   # load_state_dict, on the submodule or on the whole model
        load(other_sd)
        after = run(module)
        assert _same(after, run(fresh(_state(module))))
        assert not _same(after, before)
        before, other_sd = after, {k: v * 0.5 for k, v in other_sd.items()}
    # the documented exception: an edit through .data is not seen until invalidate_caches()
    for name in touched:
        params[name].data.copy_(params[name].data * 3)
    tspn.model.invalidate_caches(module)
    after = run(module)
    assert _same(after, run(fresh(_state(module))))
    assert not _same(after, before)


@pytest.mark.parametrize("bf16", [False, True])
def test_rpn_head_sees_changed_parameters(tspn, device, bf16):
    channels, anchors = (64 if bf16 else 32), 7
    x = torch.from_numpy(tspn.hashrng.uniform(94, "x", (2, 5, 7, channels), -1, 1)).to(device)
    x = x.bfloat16() if bf16 else x
    head = _rpn_head(tspn, device, dm.rpn_weights(tspn.hashrng, 93, channels, anchors), channels, anchors)
    other = dm.rpn_weights(tspn.hashrng, 97, channels, anchors)
    _cache_protocol(tspn, head, lambda sd: _rpn_head(tspn, device, sd, channels, anchors), lambda m: m(x), other,
                    [head.load_state_dict], [n for n, _ in head.named_parameters()])


def test_box_predictor_sees_changed_parameters(tspn, device):
    x = torch.from_numpy(tspn.hashrng.normal(96, "x", (65, 64), std=1.0)).to(device)
    pred = _predictor(tspn, device, dm.predictor_weights(tspn.hashrng, 95, 64, K), 64, K)
    other = dm.predictor_weights(tspn.hashrng, 97, 64, K)
    _cache_protocol(tspn, pred, lambda sd: _predictor(tspn, device, sd, 64, K), lambda m: m(x), other,
                    [pred.load_state_dict], [n for n, _ in pred.named_parameters()])


def test_model_sees_changed_head_parameters(tspn, device):
    """The whole model, fp32 and bf16 packs of the RPN head at once: in-place steps, load_state_dict on each of the two
    submodules and on FasterRCNNC4, invalidate_caches() after an edit through .data."""
    model, sd = _model(tspn, device, True)
    img = torch.from_numpy(tspn.hashrng.uniform(92, "img", (2, 64, 96, 3), 0, 255)).to(device)
    run = lambda m: m(img) + m(img, bf16=True)                                               # noqa: E731
    other = _weights(tspn, *_widths(True), seed=98)
    rpn, pred = "proposal_generator.rpn_head.", "roi_heads.box_predictor."
    loaders = [lambda o: model.proposal_generator.rpn_head.load_state_dict(_sub(o, rpn)),
               lambda o: model.roi_heads.box_predictor.load_state_dict(_sub(o, pred)),
               lambda o: model.load_state_dict(o)]
    _cache_protocol(tspn, model, lambda s: _model(tspn, device, True, sd=s)[0], run, other, loaders,
                    [rpn + "anchor_deltas.weight", pred + "bbox_pred.weight"])


# ------------------------------------------------------------------------------------------- f. edges and refusals
def test_edges_and_refusals(tspn, device):
    model, _ = _model(tspn, device, False)
    c4 = 256
    got = model.detect_from_maps(torch.zeros((0, 5, 7, c4), device=device), torch.zeros((0, 2), device=device))
    assert [tuple(g.shape) for g in got] == [(0, D, 4), (0, D), (0, D), (0,)] and all(g.is_cuda for g in got)
    assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.int64, torch.int64]
    with pytest.raises(ValueError):
        model(torch.zeros((2, 64, 96, 4), device=device))                                     # not [T,H,W,3]
    with pytest.raises(ValueError):
        model(torch.zeros((2, 3, 64, 96), device=device))
    with pytest.raises(ValueError):
        model(torch.zeros((64, 96, 3), device=device))
    maps = torch.zeros((2, 5, 7, c4), device=device)
    with pytest.raises(ValueError):
        model.detect_from_maps(maps, torch.tensor([[70.0, 100.0, 1.0]] * 2, device=device))   # not [T,2]
    with pytest.raises(ValueError):
        model.detect_from_maps(maps, torch.tensor([[70.0, 100.0]] * 3, device=device))
    with pytest.raises(ValueError):
        model.detect_from_maps(torch.zeros((2, 5, 7, c4 // 2), device=device), torch.tensor([[70.0, 100.0]] * 2, device=device))
    with pytest.raises(ValueError):
        tspn.RPNHead(48, 3).to(device)(torch.zeros((1, 2, 2, 48), device=device))             # fp32: channels in 32s
    with pytest.raises(ValueError):
        tspn.RPNHead(96, 3).to(device)(torch.zeros((1, 2, 2, 96), device=device, dtype=torch.bfloat16))   # bf16: in 64s
