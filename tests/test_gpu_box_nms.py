"""tspn_box_nms_f32 on the device against the numpy restatement (tests/detector_reference.py): out_index, out_count and
out_keep must be EQUAL on the same fp32 inputs.  Every call goes through the C ABI with its outputs and its scratch
framed by guard bands (the idea of tests/sentinel_buffers.py, for int64 / uint8 outputs): nothing outside them is
written, every output element is, and the result does not depend on what the scratch held."""
import ctypes

import numpy as np
import pytest
import torch

import detector_reference as ref
from sentinel_buffers import GUARD, p

pytestmark = pytest.mark.gpu

INT_SENTINEL = -0x5a5a5a5a5a5a5a5b
BYTE_SENTINEL = 0xa5


def framed(shape, device, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def check_frame(buf, view, fill, what, all_written=True):
    b = buf.cpu()
    n = view.numel()
    assert bool((b[:GUARD] == fill).all()) and bool((b[GUARD + n:] == fill).all()), f"{what}: wrote outside the output"
    if all_written:
        assert int((b[GUARD:GUARD + n] == fill).sum()) == 0, f"{what}: outputs never written"


def run(tspn, device, boxes, scores, valid, group_off, pre, thr, post, min_size, scratch_fill=BYTE_SENTINEL, keep=True):
    """One call through the ABI -> (index, count, keep) as numpy."""
    lib = tspn._abi.lib()
    n, G = len(scores), len(group_off) - 1
    arr = (ctypes.c_int64 * (G + 1))(*[int(v) for v in group_off])
    select_only = boxes is None
    need = lib.tspn_box_nms_scratch_bytes(arr, G, pre, 1 if select_only else 0)
    assert need > 0 or G == 0
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)   # noqa: E731
    d_boxes, d_scores, d_valid = t(boxes, torch.float32), t(scores, torch.float32), t(valid, torch.uint8)
    if d_scores.numel() == 0:
        d_scores = torch.zeros(4, dtype=torch.float32, device=device)       # a non-null pointer nobody reads
        d_boxes = None if select_only else torch.zeros((4, 4), dtype=torch.float32, device=device)
    ibuf, index = framed((G, post), device, torch.int64, INT_SENTINEL)
    cbuf, count = framed((G,), device, torch.int64, INT_SENTINEL)
    kbuf, kp = framed((n,), device, torch.uint8, BYTE_SENTINEL)
    want_keep = keep and not select_only
    wbuf = torch.full((need + 512,), scratch_fill, dtype=torch.uint8, device=device)
    ws = wbuf[256:256 + need]
    tspn.ops._status_block()
    rc = lib.tspn_box_nms_f32(p(d_boxes), p(d_scores), p(d_valid), n, arr, G, pre, float(thr), post, float(min_size),
                              p(index), p(count), p(kp) if want_keep else None, p(ws), need,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tspn_last_error().decode()
    torch.cuda.synchronize()
    check_frame(ibuf, index, INT_SENTINEL, "out_index")
    check_frame(cbuf, count, INT_SENTINEL, "out_count")
    if want_keep:
        check_frame(kbuf, kp, BYTE_SENTINEL, "out_keep")
    w = wbuf.cpu()
    assert bool((w[:256] == scratch_fill).all()) and bool((w[256 + need:] == scratch_fill).all()), "wrote outside the scratch"
    return index.cpu().numpy(), count.cpu().numpy(), (kp.cpu().numpy() if want_keep else None)


def same_as_reference(tspn, device, boxes, scores, valid, group_off, pre, thr, post, min_size, **kw):
    got = run(tspn, device, boxes, scores, valid, group_off, pre, thr, post, min_size, **kw)
    want = ref.box_nms(boxes, scores, valid, group_off, pre, thr, post, min_size)
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0])
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])
    return got


def grid_boxes(rng, n, extent=24, side=7):
    """Boxes on a coarse integer grid: many pairs overlap, and many IoUs are the same small fractions (1/2, 1/3, 2/3 ...)."""
    xy = rng.integers(0, extent, (n, 2))
    wh = rng.integers(1, side, (n, 2))
    return np.concatenate([xy, xy + wh], axis=1).astype(np.float32)


def tied_scores(rng, n, levels=9):
    return (rng.integers(0, levels, n) / np.float32(8)).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 1025, 2049])
@pytest.mark.parametrize("thr", [0.5, 1.0 / 3.0])
def test_one_group_at_the_block_edges(tspn, device, n, thr):
    """Past one 64-block, past one 1024-thread pass, and (2049 at pre_topk 2048) a selection that cuts; thresholds that
    grid IoUs hit exactly."""
    rng = np.random.default_rng(100 + n)
    boxes, scores = grid_boxes(rng, n, extent=16 + n // 8), tied_scores(rng, n)
    _, count, _ = same_as_reference(tspn, device, boxes, scores, None, [0, n], 2048, thr, 2048, -1.0)
    assert n == 0 or 0 < count[0] <= n


def test_three_unequal_groups_with_an_empty_one(tspn, device):
    rng = np.random.default_rng(7)
    n = 130 + 70
    boxes, scores = grid_boxes(rng, n), tied_scores(rng, n)
    got = same_as_reference(tspn, device, boxes, scores, None, [0, 130, 130, n], 128, 0.5, 40, 0.0)
    assert got[1][1] == 0 and bool((got[0][1] == -1).all())
    # suppression stays inside a group: the same candidates as one group give another answer
    one = ref.box_nms(boxes, scores, None, [0, n], 128, 0.5, 40, 0.0)
    assert set(got[0][got[0] >= 0]) != set(one[0][one[0] >= 0])


def test_all_none_and_exact_threshold(tspn, device):
    same = np.tile(np.array([[2, 3, 9, 11]], np.float32), (200, 1))
    scores = np.linspace(0, 1, 200, dtype=np.float32)
    got = same_as_reference(tspn, device, same, scores, None, [0, 200], 256, 0.5, 200, 0.0)
    assert got[1][0] == 1 and got[0][0, 0] == 199
    apart = np.array([[10 * i, 0, 10 * i + 5, 5] for i in range(200)], np.float32)
    got = same_as_reference(tspn, device, apart, scores, None, [0, 200], 256, 0.5, 200, 0.0)
    assert got[1][0] == 200 and list(got[0][0]) == list(range(199, -1, -1))
    pair = np.array([[0, 0, 2, 1], [0, 0, 1, 1]], np.float32)          # IoU exactly 0.5
    two = np.array([1, 0.5], np.float32)
    assert same_as_reference(tspn, device, pair, two, None, [0, 2], 2, 0.5, 2, 0.0)[1][0] == 2      # strict: not suppressed
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert same_as_reference(tspn, device, pair, two, None, [0, 2], 2, below, 2, 0.0)[1][0] == 1
    chain = np.array([[0, 0, 4, 4], [1, 0, 5, 4], [2, 0, 6, 4]], np.float32)   # A kills B (3/5), so B cannot kill C; A-C 1/3
    got = same_as_reference(tspn, device, chain, np.array([3, 2, 1], np.float32), None, [0, 3], 3, 0.5, 3, 0.0)
    assert list(got[0][0]) == [0, 2, -1]


@pytest.mark.parametrize("post", [1, 5, 64, 300])
def test_post_topk_below_and_above_the_survivors(tspn, device, post):
    rng = np.random.default_rng(11)
    boxes, scores = grid_boxes(rng, 300, extent=40), tied_scores(rng, 300, levels=5)
    same_as_reference(tspn, device, boxes, scores, None, [0, 300], 300, 0.4, post, 0.0)


def test_invalid_rows_inside_and_outside_the_topk_and_min_size(tspn, device):
    rng = np.random.default_rng(13)
    n = 500
    boxes, scores = grid_boxes(rng, n, extent=40), rng.standard_normal(n).astype(np.float32)
    valid = (rng.random(n) > 0.3).astype(np.uint8)
    order = ref.select_order(scores, n)
    valid[order[0]] = 0                   # the best candidate, inside the top-k
    valid[order[-1]] = 0                  # the worst, outside it
    got = same_as_reference(tspn, device, boxes, scores, valid, [0, 200, n], 150, 0.5, 150, 0.0)
    assert order[0] not in got[0]
    # detectron2's order: the cut comes first, then the drop -- an invalid row in the top-k is not replaced from below
    only = np.zeros(n, np.uint8)
    only[order[150:]] = 1
    assert same_as_reference(tspn, device, boxes, scores, only, [0, n], 150, 0.5, 150, 0.0)[1][0] == 0
    for min_size in (0.0, 2.0, 5.5, -1.0):
        same_as_reference(tspn, device, boxes, scores, None, [0, n], 400, 0.5, 400, min_size)
    flat = boxes.copy()
    flat[::3, 2] = flat[::3, 0]           # zero width: dropped at min_size 0, kept with the filter off
    a = same_as_reference(tspn, device, flat, scores, None, [0, n], 512, 0.5, 512, 0.0)
    b = same_as_reference(tspn, device, flat, scores, None, [0, n], 512, 0.5, 512, -1.0)
    assert a[1][0] < b[1][0]


def test_nan_and_infinite_scores_and_boxes(tspn, device):
    rng = np.random.default_rng(17)
    n = 260
    boxes, scores = grid_boxes(rng, n), tied_scores(rng, n)
    scores[[3, 77, 200]] = np.nan
    scores[[5, 150]] = np.inf
    scores[[9, 151, 152]] = -np.inf
    scores[10] = -0.0
    got = same_as_reference(tspn, device, boxes, scores, None, [0, n], 256, 0.5, 256, 0.0)
    assert got[0][0, 0] == 3              # NaN first, the lowest index of them
    boxes[40] = np.nan                    # a NaN box compares false: kept with the size filter off, dropped with it on
    boxes[41, 2] = np.inf
    same_as_reference(tspn, device, boxes, scores, None, [0, n], 256, 0.5, 256, -1.0)
    same_as_reference(tspn, device, boxes, scores, None, [0, n], 256, 0.5, 256, 0.0)


def test_the_selection_alone(tspn, device):
    rng = np.random.default_rng(19)
    scores = tied_scores(rng, 3000, levels=40)
    scores[rng.integers(0, 3000, 20)] = np.nan
    for off, pre, post in (([0, 1000, 1000, 3000], 700, 700), ([0, 3000], 2500, 100), ([0, 10, 3000], 64, 64)):
        same_as_reference(tspn, device, None, scores, None, off, pre, 0.0, post, 0.0)


def test_the_result_does_not_depend_on_the_scratch(tspn, device):
    rng = np.random.default_rng(23)
    n = 700
    boxes, scores = grid_boxes(rng, n, extent=30), tied_scores(rng, n)
    valid = (rng.random(n) > 0.1).astype(np.uint8)
    args = (boxes, scores, valid, [0, 300, 300, n], 350, 0.5, 100, 1.0)
    runs = [run(tspn, device, *args, scratch_fill=f) for f in (0x00, 0xff, 0xa5)]
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
    want = ref.box_nms(*args)
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], want))


def test_the_wrapper_agrees_and_refuses_a_short_workspace(tspn, device):
    rng = np.random.default_rng(29)
    n = 400
    boxes, scores = grid_boxes(rng, n), tied_scores(rng, n)
    off = [0, 150, n]
    tb, ts = torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device)
    index, count, keep = tspn.ops.box_nms(tb, ts, off, 256, 0.5, 80, min_size=0.0, want_keep=True)
    want = ref.box_nms(boxes, scores, None, off, 256, 0.5, 80, 0.0)
    assert np.array_equal(index.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
    assert np.array_equal(keep.cpu().numpy(), want[2])
    need = tspn.ops.box_nms_workspace_bytes(off, 256)
    with pytest.raises(ValueError, match="workspace too small"):
        tspn.ops.box_nms(tb, ts, off, 256, 0.5, 80, workspace=torch.empty(need - 1, dtype=torch.uint8, device=device))
    lib = tspn._abi.lib()
    arr = (ctypes.c_int64 * 3)(*off)
    ibuf, iv = framed((2, 80), device, torch.int64, INT_SENTINEL)
    cbuf, cv = framed((2,), device, torch.int64, INT_SENTINEL)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    rc = lib.tspn_box_nms_f32(p(tb), p(ts), None, n, arr, 2, 256, 0.5, 80, 0.0, p(iv), p(cv), None, p(ws), need - 1, None)
    assert rc == tspn._abi.TSPN_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ibuf.cpu() == INT_SENTINEL).all()) and bool((cbuf.cpu() == INT_SENTINEL).all())
