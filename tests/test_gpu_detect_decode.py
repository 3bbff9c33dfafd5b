"""tspn_rpn_decode_f32 and tspn_box_head_decode_f32 against the float64 form of the restatement
(tests/detector_reference.py), within the bounds DESIGN.md 3 derives, and their exact cases.

Bounds (u = 2^-24; derivation in DESIGN.md 3 "detector decode"), for deltas with |dx / wx|, |dy / wy| <= 1 and
dw / ww, dh / wh >= -1 -- the domain the inputs below are drawn from:
    every corner, before and after the clip:  |fp32 - float64| <= 18 u (|pred_ctr| + pred_w)
    every softmax score:                      |fp32 - float64| <= (K + 2 L + 6) u score,  L = max |z - max z| <= 16"""
import numpy as np
import pytest
import torch

import detector_reference as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_BOX = 18.0
L_MAX = 16.0


def dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


def draw_deltas(rng, shape, weights=(1.0, 1.0, 1.0, 1.0)):
    """[..., 4] with dx / wx, dy / wy in [-1, 1] and dw / ww, dh / wh in [-1, 5] (a tenth of them past the clamp)."""
    d = np.empty(tuple(shape) + (4,), np.float32)
    d[..., :2] = rng.uniform(-1, 1, tuple(shape) + (2,))
    d[..., 2:] = rng.uniform(-1, 1.5, tuple(shape) + (2,))
    far = rng.random(tuple(shape) + (2,)) < 0.1
    d[..., 2:] = np.where(far, rng.uniform(4, 5, tuple(shape) + (2,)), d[..., 2:])
    d *= np.asarray(weights, np.float32) * np.float32(0.999)      # the product with the weight stays inside the domain
    return d


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (9, 7)])
@pytest.mark.parametrize("A", [3, 15])
def test_rpn_decode_is_within_the_derived_bound(tspn, device, H, W, A):
    rng = np.random.default_rng(1000 * H + 10 * W + A)
    B = 2
    cell = ref.cell_anchors() if A == 15 else ref.cell_anchors((32, 64, 128), (1.0,))
    logits = rng.standard_normal((B, H, W, A)).astype(np.float32)
    deltas = draw_deltas(rng, (B, H, W, A)).reshape(B, H, W, 4 * A)
    sizes = np.array([[90.0, 130.0], [4000.0, 3000.0]], np.float32)       # one image that clips a lot, one that hardly does
    HWA = H * W * A
    cand = np.stack([b * HWA + rng.permutation(HWA) for b in range(B)]).astype(np.int64)
    cand[0, 0], cand[1, -1] = -1, 0                                         # no candidate; image 0's index in image 1's row
    for c in (None, cand):
        boxes, lg, valid = tspn.ops.rpn_decode(None if c is None else dev(c, device), dev(logits, device), dev(deltas, device),
                                               dev(cell, device), 16.0, dev(sizes, device))
        want, wl, wv, mag = ref.rpn_decode(c, logits, deltas, cell, 16.0, sizes, np.float64)
        assert np.array_equal(valid.cpu().numpy(), wv)
        assert np.array_equal(lg.cpu().numpy(), wl)                         # a gather: exact
        err = np.abs(boxes.cpu().numpy().astype(np.float64) - want)
        bound = C_BOX * U * np.stack([mag[..., 0], mag[..., 1], mag[..., 0], mag[..., 1]], axis=-1)
        print(f"rpn_decode {H}x{W}x{A}: max err / bound = {float((err / np.maximum(bound, 1e-300))[wv != 0].max(initial=0)):.3f}")
        assert bool((err <= bound)[wv != 0].all())
        if c is not None:
            assert wv[0, 0] == 0 and wv[1, -1] == 0 and not boxes[0, 0].any() and wv.sum() == 2 * HWA - 2


def test_rpn_decode_exact_cases(tspn, device):
    H, W, A, B = 3, 5, 3, 2
    sizes = np.array([[40.0, 70.0], [40.0, 70.0]], np.float32)
    logits = np.arange(B * H * W * A, dtype=np.float32).reshape(B, H, W, A)
    zero = np.zeros((B, H, W, 4 * A), np.float32)
    # integer cell anchors: every fp32 operation of the zero-delta decode is exact, the result is the anchor clipped
    cell = np.array([[-8, -8, 8, 8], [-16, -4, 16, 4], [-3, -11, 5, 13]], np.float32)
    boxes, _, valid = tspn.ops.rpn_decode(None, dev(logits, device), dev(zero, device), dev(cell, device), 16.0, dev(sizes, device))
    anchors = ref.grid_anchors(cell, H, W, 16.0)
    assert np.array_equal(boxes[0].cpu().numpy(), ref.clip(anchors, np.float32(40), np.float32(70))) and bool(valid.all())
    # the default (irrational) anchors: equal to the fp32 restatement, operation for operation (exp(0) = 1 in both)
    cell = ref.cell_anchors((32, 64, 128), (0.5,))
    boxes, _, _ = tspn.ops.rpn_decode(None, dev(logits, device), dev(zero, device), dev(cell, device), 16.0, dev(sizes, device))
    assert np.array_equal(boxes.cpu().numpy(), ref.rpn_decode(None, logits, zero, cell, 16.0, sizes, np.float32)[0])
    # the clamp: any dw past log(1000 / 16) decodes as the clamp itself
    big = zero.copy().reshape(B, H, W, A, 4)
    big[..., 2], big[..., 3] = 100.0, np.inf
    at = big.copy()
    at[..., 2:] = np.float32(ref.SCALE_CLAMP)
    huge = np.array([[1e6, 1e6]] * B, np.float32)
    got = [tspn.ops.rpn_decode(None, dev(logits, device), dev(d.reshape(B, H, W, 4 * A), device), dev(cell, device), 16.0,
                               dev(huge, device)) for d in (big, at)]
    assert torch.equal(got[0][0], got[1][0]) and bool(got[0][2].all())
    # validity: a NaN or infinite delta, an infinite logit, a delta that overflows
    bad = zero.copy().reshape(B, H * W * A, 4)
    bad[0, 1, 0], bad[0, 2, 1], bad[0, 3, 1] = np.nan, -np.inf, 3e38
    lg = logits.copy().reshape(B, -1)
    lg[1, 4], lg[1, 5] = np.inf, np.nan
    boxes, out_lg, valid = tspn.ops.rpn_decode(None, dev(lg.reshape(logits.shape), device), dev(bad.reshape(zero.shape), device),
                                               dev(cell, device), 16.0, dev(sizes, device))
    v = valid.cpu().numpy()
    assert not v[0, 1:4].any() and not v[1, 4:6].any() and v.sum() == v.size - 5
    assert not boxes[0, 1:4].any() and not boxes[1, 4:6].any() and not out_lg[1, 4:6].any()
    assert np.array_equal(v, ref.rpn_decode(None, lg.reshape(logits.shape), bad.reshape(zero.shape), cell, 16.0, sizes)[2])


@pytest.mark.parametrize("R", [1, 65, 300])
@pytest.mark.parametrize("K", [1, 35])
def test_box_head_decode_is_within_the_derived_bounds(tspn, device, R, K):
    rng = np.random.default_rng(100 * R + K)
    B = 2
    weights = (10.0, 10.0, 5.0, 5.0)
    z = np.clip(rng.standard_normal((B * R, K + 1)) * 3, -8, 8).astype(np.float32)          # |z - max z| <= 16
    deltas = draw_deltas(rng, (B * R, K), weights).reshape(B * R, 4 * K)
    xy = rng.uniform(0, 500, (B, R, 2))
    props = np.concatenate([xy, xy + rng.uniform(1, 300, (B, R, 2))], axis=2).astype(np.float32)
    count = np.array([R, max(R - 7, 0)], np.int64)
    sizes = np.array([[600.0, 800.0], [300.0, 5000.0]], np.float32)
    scores, boxes, valid = tspn.ops.box_head_decode(dev(z, device), dev(deltas, device), dev(props, device), dev(count, device),
                                                    dev(sizes, device), 0.05, weights)
    assert scores.shape == (B, K, R) and boxes.shape == (B, K, R, 4) and valid.shape == (B, K, R)      # class-major
    ws, wb, wv, row_ok, mag, s64 = ref.box_head_decode(z, deltas, props, count, sizes, 0.05, weights, np.float64)
    assert row_ok[0].all() and row_ok[1].sum() == count[1]
    s_bound = (K + 2 * L_MAX + 6) * U * s64
    thr = float(np.float32(0.05))
    sure = row_ok[:, None, :] & (np.abs(s64 - thr) > s_bound)              # rows the threshold decides either way
    v = valid.cpu().numpy()
    assert np.array_equal(v[sure], wv[sure]) and not v[~np.broadcast_to(row_ok[:, None, :], v.shape)].any()
    got_s = scores.cpu().numpy().astype(np.float64)
    on = v != 0
    assert not got_s[~on].any()                                            # the score of an absent row is 0
    err_s = np.abs(got_s - s64)
    print(f"box_head_decode R={R} K={K}: max score err / bound = {float((err_s / s_bound)[on].max(initial=0)):.3f}")
    assert bool((err_s <= s_bound)[on].all())
    live = np.broadcast_to(row_ok[:, None, :, None], wb.shape)
    err = np.abs(boxes.cpu().numpy().astype(np.float64) - wb)
    bound = C_BOX * U * np.stack([mag[..., 0], mag[..., 1], mag[..., 0], mag[..., 1]], axis=-1)
    print(f"box_head_decode R={R} K={K}: max box err / bound = {float((err / bound)[live].max(initial=0)):.3f}")
    assert bool((err <= bound)[live].all())
    assert not boxes.cpu().numpy()[~live].any()                            # rows past the count hold zeros


def test_box_head_decode_exact_cases(tspn, device):
    B, R, K = 1, 65, 3
    sizes = np.array([[100.0, 120.0]], np.float32)
    xy = np.arange(R * 2, dtype=np.float32).reshape(1, R, 2) - 10
    props = np.concatenate([xy, xy + np.array([20, 8], np.float32)], axis=2)           # integer corners, even sides
    z = np.zeros((R, K + 1), np.float32)                                                 # every score exactly 1/4
    zero = np.zeros((R, 4 * K), np.float32)
    count = np.array([R], np.int64)
    args = lambda z_, d_, c_: (dev(z_, device), dev(d_, device), dev(props, device), dev(c_, device), dev(sizes, device))   # noqa: E731
    scores, boxes, valid = tspn.ops.box_head_decode(*args(z, zero, count), 0.05)
    want = ref.clip(props[0], np.float32(100), np.float32(120))
    for c in range(K):
        assert np.array_equal(boxes[0, c].cpu().numpy(), want)
    assert bool((scores == 0.25).all()) and bool(valid.all())
    # the threshold is strict
    assert not tspn.ops.box_head_decode(*args(z, zero, count), 0.25)[2].any()
    # the clamp, with the box head's weights (dw / 5)
    big, at = zero.copy(), zero.copy()
    big[:, 2::4], big[:, 3::4] = 1000.0, np.inf
    at[:, 2::4] = at[:, 3::4] = np.float32(5 * 4.2)
    huge = dev(np.array([[1e6, 1e6]], np.float32), device)
    a = tspn.ops.box_head_decode(dev(z, device), dev(big, device), dev(props, device), dev(count, device), huge, 0.05)
    b = tspn.ops.box_head_decode(dev(z, device), dev(at, device), dev(props, device), dev(count, device), huge, 0.05)
    assert torch.equal(a[1], b[1]) and bool(a[2].all())
    # a non-finite logit or delta drops the whole proposal, as detectron2's valid_mask does
    zb, db = z.copy(), zero.copy()
    zb[3, 1], zb[4, K], zb[5, :] = np.nan, np.inf, -np.inf
    db[6, 5], db[7, 0] = np.nan, np.inf
    scores, boxes, valid = tspn.ops.box_head_decode(*args(zb, db, np.array([R - 2], np.int64)), 0.05)
    v = valid.cpu().numpy()[0]
    gone = [3, 4, 5, 6, 7, R - 2, R - 1]
    assert not v[:, gone].any() and v.sum() == K * (R - len(gone))
    assert not scores[0][:, gone].any() and not boxes[0][:, gone].any()
    wv = ref.box_head_decode(zb, db, props, np.array([R - 2]), sizes, 0.05)[2]
    assert np.array_equal(valid.cpu().numpy(), wv)
