"""The detector's compositions and the module on the device.

ops.rpn_proposals and ops.box_detections must reproduce, EXACTLY, the restatement of their selection stages
(tests/detector_reference.py) fed the boxes and scores the device decoded -- the decode stages have their own bounded
test (tests/test_gpu_detect_decode.py).  FasterRCNNC4 runs at reduced depth on two 64 x 96 frames with seeded weights."""
import io

import numpy as np
import pytest
import torch

import detector_reference as ref
from oracle import roi_head_oracle as ro

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("pre,post", [(300, 50), (6000, 1000), (64, 64)])
def test_compositions_equal_the_restatement(tspn, device, pre, post):
    rng = np.random.default_rng(pre + post)
    ops = tspn.ops
    # ---- proposals: a 9 x 7 map, 15 anchors; logits on a coarse grid (ties), a few non-finite deltas and logits
    B, H, W, A = 2, 9, 7, 15
    HWA = H * W * A
    cell = ref.cell_anchors()
    logits = (rng.integers(-20, 20, (B, H, W, A)) / np.float32(4)).astype(np.float32)
    deltas = (rng.standard_normal((B, H, W, 4 * A)) * 0.5).astype(np.float32)
    deltas.reshape(-1)[rng.integers(0, deltas.size, 12)] = np.nan
    deltas.reshape(-1)[rng.integers(0, deltas.size, 6)] = np.inf
    logits.reshape(-1)[rng.integers(0, logits.size, 5)] = np.inf        # first in the selection, dropped after it
    sizes = np.array([[100.0, 90.0], [144.0, 112.0]], np.float32)
    d = [dev(x, device) for x in (logits, deltas, cell, sizes)]
    # HWA = 945, so M is 945 in the (6000, 1000) row too: the selection that does cut at 6000, and the NMS of 6000
    # candidates, are tests/test_gpu_box_nms_limits.py::test_rpn_proposals_where_6000_cuts
    M = min(pre, HWA)
    cand, _, _ = ops.box_nms(None, d[0].reshape(-1), range(0, (B + 1) * HWA, HWA), M, 0.0, M)
    assert np.array_equal(cand.cpu().numpy(), ref.rpn_proposals_select(logits, pre))
    boxes, lg, valid = host(*ops.rpn_decode(cand, *d[:3], 16.0, d[3]))
    for min_size in (0.0, 12.0):
        want = ref.rpn_proposals_finish(boxes, lg, valid, post, 0.7, min_size)
        got = host(*ops.rpn_proposals(*d[:3], 16.0, d[3], pre, post, 0.7, min_size))
        assert got[0].shape == (B, post, 4) and got[1].shape == (B, post)
        assert np.array_equal(got[2], want[2]) and 0 < got[2].min() and got[2].max() <= min(post, M)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ---- detections: the proposals above through a random box head; 35 classes
    K, R = 35, min(post, 130)                  # past one 64-block twice over; the restatement's loops stay short
    props, _, count = ops.rpn_proposals(*d[:3], 16.0, d[3], pre, R, 0.7, 0.0)
    z = (rng.integers(-12, 12, (B * R, K + 1)) / np.float32(2)).astype(np.float32)      # coarse logits: tied scores
    bd = (rng.standard_normal((B * R, 4 * K)) * 0.8).astype(np.float32)
    z[rng.integers(0, B * R, 3), rng.integers(0, K + 1, 3)] = np.nan
    bd[rng.integers(0, B * R, 3), rng.integers(0, 4 * K, 3)] = np.inf
    dz, dbd = dev(z, device), dev(bd, device)
    for thr, nms, D in ((0.05, 0.5, 100), (0.0, 0.3, 7), (0.2, 0.5, 1000)):
        sc, bx, vl = host(*ops.box_head_decode(dz, dbd, props, count, d[3], thr))
        want = ref.detections_finish(sc, bx, vl, nms, D)
        got = host(*ops.box_detections(dz, dbd, props, count, d[3], thr, nms, D))
        assert np.array_equal(got[3], want[3]) and got[3].max() > 0
        for g, w in zip(got[:3], want[:3]):
            assert g.shape == w.shape and np.array_equal(g, w)


def test_detections_topk_ties_and_counts(tspn, device):
    rng = np.random.default_rng(5)
    B, K, R = 3, 4, 70
    scores = (rng.integers(0, 4, (B, K, R)) / np.float32(4)).astype(np.float32)         # four score levels: ties everywhere
    boxes = rng.uniform(0, 50, (B, K, R, 4)).astype(np.float32)
    keep = (rng.random((B, K, R)) < 0.4).astype(np.uint8)
    keep[1] = 0                                                                          # an image without survivors
    keep[2, :, 5:] = 0
    for D in (1, 10, 300):
        ob, os_, oc, cnt = host(*tspn.ops.detections_topk(dev(scores, device), dev(boxes, device), dev(keep, device), D))
        for b in range(B):
            r, c = np.nonzero(keep[b].T)                                                 # ascending r K + c
            order = np.lexsort((r * K + c, -scores[b][c, r].astype(np.float64)))[:D]
            n = len(order)
            assert cnt[b] == n == min(D, int(keep[b].sum()))
            assert np.array_equal(oc[b, :n], c[order]) and np.array_equal(os_[b, :n], scores[b][c[order], r[order]])
            assert np.array_equal(ob[b, :n], boxes[b][c[order], r[order]])
            assert not ob[b, n:].any() and not os_[b, n:].any() and not oc[b, n:].any()


def _weights(tspn, blocks, res5, num_classes):
    u = lambda name, shape, lo, hi: tspn.hashrng.uniform(91, name, shape, lo, hi)       # noqa: E731
    nrm = lambda name, shape, std: tspn.hashrng.normal(91, name, shape, std=std)         # noqa: E731
    sd = {"backbone." + k: v for k, v in ro.make_backbone_weights(u, nrm, 64, 256, blocks).items()}
    sd.update({"roi_heads." + k: v for k, v in ro.make_res5_weights(u, nrm, 1024, res5[0], res5[1], res5[2]).items()})
    t = lambda a: torch.from_numpy(a)                                                    # noqa: E731
    pre = "proposal_generator.rpn_head."
    sd[pre + "conv.weight"] = t(nrm("rpn.conv.w", (1024, 1024, 3, 3), 0.01))
    sd[pre + "conv.bias"] = t(u("rpn.conv.b", (1024,), -0.1, 0.1))
    sd[pre + "objectness_logits.weight"] = t(nrm("rpn.obj.w", (15, 1024, 1, 1), 0.02))
    sd[pre + "objectness_logits.bias"] = t(u("rpn.obj.b", (15,), -0.5, 0.5))
    sd[pre + "anchor_deltas.weight"] = t(nrm("rpn.dl.w", (60, 1024, 1, 1), 0.01))
    sd[pre + "anchor_deltas.bias"] = t(u("rpn.dl.b", (60,), -0.2, 0.2))
    pre = "roi_heads.box_predictor."
    sd[pre + "cls_score.weight"] = t(nrm("cls.w", (num_classes + 1, res5[1]), 0.3))
    sd[pre + "cls_score.bias"] = t(u("cls.b", (num_classes + 1,), -0.5, 0.5))
    sd[pre + "bbox_pred.weight"] = t(nrm("box.w", (4 * num_classes, res5[1]), 0.1))
    sd[pre + "bbox_pred.bias"] = t(u("box.b", (4 * num_classes,), -0.5, 0.5))
    return sd


@pytest.mark.parametrize("bf16", [False, True])
def test_faster_rcnn_c4_at_reduced_depth(tspn, device, bf16):
    blocks, res5, K, D, R = (1, 1, 1), (64, 128, 1), 35, 20, 40
    kw = dict(num_classes=K, blocks=blocks, res5_bottleneck=res5[0], res5_out=res5[1], res5_blocks=res5[2], post_nms_topk=R,
              score_thresh=0.01, detections_per_image=D, pixel_mean=(100.0, 110.0, 120.0), pixel_std=(60.0, 61.0, 62.0))
    model = tspn.FasterRCNNC4(**kw)
    model.load_state_dict(_weights(tspn, blocks, res5, K), strict=True)
    model = model.to(device).eval()
    img = torch.from_numpy(tspn.hashrng.uniform(92, "img", (2, 64, 96, 3), 0, 255)).to(device)
    boxes, scores, classes, count = model(img, bf16=bf16)
    assert boxes.shape == (2, D, 4) and scores.shape == (2, D) and classes.shape == (2, D) and count.shape == (2,)
    assert classes.dtype == torch.int64 and count.dtype == torch.int64 and boxes.dtype == scores.dtype == torch.float32
    b, s, c, n = host(boxes, scores, classes, count)
    assert n.min() >= 0 and n.max() <= D and n.sum() > 0
    for t in range(2):
        live = b[t, :n[t]]
        assert (live[:, 0] >= 0).all() and (live[:, 1] >= 0).all() and (live[:, 2] <= 96).all() and (live[:, 3] <= 64).all()
        assert (live[:, 0] <= live[:, 2]).all() and (live[:, 1] <= live[:, 3]).all()
        assert (np.diff(s[t, :n[t]]) <= 0).all() and (s[t, :n[t]] > 0.01).all()
        assert ((c[t, :n[t]] >= 0) & (c[t, :n[t]] < K)).all()
        assert not b[t, n[t]:].any() and not s[t, n[t]:].any() and not c[t, n[t]:].any()
    # the same from the maps
    x = (img - model.pixel_mean.view(1, 1, 1, 3)) / model.pixel_std.view(1, 1, 1, 3)
    maps = model.backbone(x, bf16=bf16)
    sizes = torch.tensor([[64.0, 96.0]] * 2, device=device)
    for got, want in zip(model.detect_from_maps(maps, sizes), (boxes, scores, classes, count)):
        assert torch.equal(got, want)
    # a saved and reloaded state dict
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    again = tspn.FasterRCNNC4(**kw)
    again.load_state_dict(torch.load(buf, map_location="cpu"), strict=True)
    for got, want in zip(again.to(device).eval()(img, bf16=bf16), (boxes, scores, classes, count)):
        assert torch.equal(got, want)
    # two frames in one call equal each frame alone (and in chunks of one)
    model.frame_chunk = 1
    for got, want in zip(model(img, bf16=bf16), (boxes, scores, classes, count)):
        assert torch.equal(got, want)
    for t in range(2):
        for got, want in zip(model(img[t:t + 1], bf16=bf16), (boxes, scores, classes, count)):
            assert torch.equal(got[0], want[t])
