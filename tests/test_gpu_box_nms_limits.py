"""tspn_box_nms_f32, its selection and the final top-k at the sizes the detector's defaults take and the older tests stop
short of, each against the numpy restatement (tests/detector_reference.py) and, where the answer has a closed form, against
that form written out:

* column blocks 64 .. 127 of `box_nms_scan_kernel` (the removed bits a lane keeps in its second word): groups of more than
  4096 selected candidates;
* `tspn::select_topk_sorted` at the 8192 capacity with an 8192-slot sort (M in 4097 .. 8192), more than 65 536 candidates
  and a cut among ties above index 65 536;
* the second and the third launch of `box_nms_offsets_kernel` (more than 255 and more than 511 groups);
* `detections_topk_kernel` at Q = K R = 35 000 and 80 000 with D = 1024, and the two compositions at shapes that reach the
  above (7200 anchors at pre_nms_topk 6000; 8 x 35 = 280 class groups).

Everything here is exact: index, count and keep are compared with np.array_equal, through the C ABI with framed outputs and
a framed scratch (the helpers of tests/test_gpu_box_nms.py).  Every test first asserts, on the restatement's own output,
that its input reaches the path it is there for."""
import functools

import numpy as np
import pytest

import detector_reference as ref
from test_gpu_box_nms import grid_boxes, run, same_as_reference, tied_scores
from test_gpu_detector import dev, host

pytestmark = pytest.mark.gpu

HALF = 64 * 64          # sorted positions from here on live in column blocks 64 .. 127: the scan's second word per lane


def equal(got, want):
    """(index, count, keep) of one run against the same triple computed before."""
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0])
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])


def positions(scores, valid, boxes, min_size, pre, keep):
    """Per sorted position of one group: is the candidate alive before the scan, and is it kept."""
    order = ref.select_order(scores, pre)
    alive = np.ones(len(order), bool) if valid is None else valid[order] != 0
    if min_size >= 0:
        b = boxes[order]
        alive &= ((b[:, 2] - b[:, 0]) > np.float32(min_size)) & ((b[:, 3] - b[:, 1]) > np.float32(min_size))
    return alive, keep[order] != 0


# ------------------------------------------------------------------- A. random grids past 4096 selected candidates
@pytest.mark.parametrize("n,pre", [(4096, 8192), (4097, 8192), (6000, 6000), (8192, 8192), (8300, 8192)])
def test_random_grids_past_4096_selected(tspn, device, n, pre):
    """Blocks 63 / 64 (4096: the second word stays dead; 4097: one candidate in block 64), the detector's default, the
    capacity, and a selection that cuts at the capacity.  A scan that reads the first word for a block >= 64, or never
    ORs into the second, keeps or drops candidates past position 4096: survivors AND suppressed ones exist there."""
    rng = np.random.default_rng(4000 + n)
    boxes, scores = grid_boxes(rng, n, extent=60), tied_scores(rng, n)
    args = (boxes, scores, None, [0, n], pre, 0.5, pre, 0.0)
    want = ref.box_nms(*args)
    alive, kept = positions(scores, None, boxes, 0.0, pre, want[2])
    assert len(alive) == min(n, pre) and alive.all()
    if n >= 6000:
        assert kept[HALF:].sum() > 100 and (~kept[HALF:]).sum() > 100, (kept[HALF:].sum(), (~kept[HALF:]).sum())
    elif n == 4097:
        assert not kept[HALF]             # the one candidate of block 64 is removed by a row of the first 64 blocks
    equal(run(tspn, device, *args), want)


def test_dead_rows_past_4096_selected(tspn, device):
    """Invalid and small rows at sorted positions >= 4096 enter the second word through the ballot; a scan that seeds only
    the first word lets them through (an index of -1 among the kept ones, a larger count)."""
    rng = np.random.default_rng(4321)
    n = 8192
    boxes, scores = grid_boxes(rng, n, extent=60), tied_scores(rng, n)
    valid = (rng.random(n) > 0.25).astype(np.uint8)
    args = (boxes, scores, valid, [0, n], n, 0.5, n, 2.0)
    want = ref.box_nms(*args)
    order = ref.select_order(scores, n)
    alive, kept = positions(scores, valid, boxes, 2.0, n, want[2])
    assert (valid[order[HALF:]] == 0).sum() > 100 and (valid[order[:HALF]] == 0).sum() > 100
    assert ((valid[order[HALF:]] != 0) & ~alive[HALF:]).sum() > 100          # valid but not larger than min_size
    assert kept[HALF:].sum() > 50 and (alive[HALF:] & ~kept[HALF:]).sum() > 50
    equal(run(tspn, device, *args), want)


# ----------------------------------------------------------------------------------------- B. closed-form cases
def apart(i):
    """Boxes no two of which touch unless their i are equal: [10 i, 0, 10 i + 5, 5]."""
    i = np.asarray(i, np.float32)
    return np.stack([10 * i, 0 * i, 10 * i + 5, 0 * i + 5], axis=1).astype(np.float32)


def descending(n):
    """Strictly descending scores: sorted position == index."""
    return np.arange(n, 0, -1).astype(np.float32)


def closed_form(tspn, device, boxes, valid, pre, post, expected):
    """The restatement gives `expected` (the kept flat indices in order), and the device gives the restatement."""
    n = len(boxes)
    expected = np.asarray(expected, np.int64)
    want = ref.box_nms(boxes, descending(n), valid, [0, n], pre, 0.5, post, 0.0)
    assert want[1][0] == len(expected) <= post
    assert np.array_equal(want[0][0, :len(expected)], expected) and bool((want[0][0, len(expected):] == -1).all())
    keep = np.zeros(n, np.uint8)
    keep[expected] = 1
    assert np.array_equal(want[2], keep)
    got = run(tspn, device, boxes, descending(n), valid, [0, n], pre, 0.5, post, 0.0)
    equal(got, want)
    return got


def test_lower_half_suppresses_upper_half(tspn, device):
    """Rows 4096 .. 8191 repeat rows 0 .. 4095, except every third (j = 1 mod 3 of the second half), which stands alone:
    4096 + 1365 = 5461 survive.  A scan that loses the OR of a kept row's words into the second word keeps 8192; one that
    ORs the first half's words into it keeps too few."""
    n = 8192
    boxes = apart(np.arange(n) % HALF)
    j = np.arange(HALF)
    fresh = HALF + j[j % 3 == 1]
    boxes[fresh] = apart(fresh)
    expected = np.concatenate([np.arange(HALF), fresh])
    assert len(expected) == 5461
    closed_form(tspn, device, boxes, None, n, n, expected)


def upper_on_upper():
    n = 8192
    boxes = apart(np.arange(n))
    boxes[6144:] = boxes[4096:6144]
    return boxes


def test_upper_half_suppresses_upper_half(tspn, device):
    """Rows 6144 .. 8191 repeat rows 4096 .. 6143: suppressor and suppressed both live in column blocks >= 64 (the
    `lane + 64 > blk` side of the OR).  6144 survive, 0 .. 6143 in order; a scan that ORs only rows of the first 64 blocks
    into the second word keeps 8192."""
    closed_form(tspn, device, upper_on_upper(), None, 8192, 8192, np.arange(6144))


def test_a_dead_row_past_4096_suppresses_nobody(tspn, device):
    """The same with rows 4096 .. 4159 (block 64) invalid: they are not kept, and their 64 copies 6144 .. 6207 survive.  The
    count is 6144 as before, the kept set is not: a scan that ORs the words of a dead row, or that does not mark it
    removed in the second word, differs."""
    valid = np.ones(8192, np.uint8)
    valid[4096:4160] = 0
    expected = np.concatenate([np.arange(4096), np.arange(4160, 6144), np.arange(6144, 6208)])
    assert len(expected) == 6144 - 64 + 64
    got = closed_form(tspn, device, upper_on_upper(), valid, 8192, 8192, expected)
    assert not np.array_equal(got[0][0, :6144], np.arange(6144))


def early_exit_boxes():
    n = 7000
    idx = np.arange(n)
    idx[:4200] %= 50
    return apart(idx)


# 50 survivors in block 0, none in blocks 1 .. 64, then rows 4200 .. 4223 of block 65 (24 of them) and every later row:
# 49 / 50 / 51 stop before, at and after the jump; 74 puts the last survivor on row 4223, the last of block 65
@pytest.mark.parametrize("post", [350, 49, 50, 51, 50 + 24])
def test_early_exit_deep_in_the_list(tspn, device, post):
    """Rows 0 .. 4199 cycle through 50 boxes, rows 4200 .. 6999 stand alone: the kept ones are 0 .. 49, then 4200 onwards,
    cut at post_topk.  A scan that stops a block early or late, counts a block's survivors past post_topk, or ranks the
    survivors of block 65 from the wrong base gives other indices or another count; every slot of out_index holds a
    survivor, none is -1."""
    boxes = early_exit_boxes()
    expected = np.concatenate([np.arange(50), np.arange(4200, 7000)])[:post]
    if post == 74:
        assert expected[-1] == 4223 == 66 * 64 - 1
    got = closed_form(tspn, device, boxes, None, 7000, post, expected)
    assert got[1][0] == post and bool((got[0] >= 0).all()) and got[2].sum() == post


@pytest.mark.parametrize("post", [4095, 4096, 4097])
def test_survivors_on_both_sides_of_the_half_boundary(tspn, device, post):
    """4160 boxes that never touch: the first post_topk survive, the last of them in block 63 or the first of block 64.  A
    scan whose count or exit is off by one block at the change of words gives another count."""
    closed_form(tspn, device, apart(np.arange(4160)), None, 4160, post, np.arange(post))


# --------------------------------------------------------------------------- C. unequal groups under one capacity
def test_unequal_groups_under_one_capacity(tspn, device):
    """Groups of 8192, 0, 70 and 4100 share a scratch laid out for 8192: the small groups own mask rows and column blocks
    nobody writes, so a scan or a mask kernel that takes the capacity for the group's own count reads what the fill left
    there, and the three fills differ."""
    off = [0, 8192, 8192, 8262, 12362]
    rng = np.random.default_rng(31)
    n = off[-1]
    boxes, scores = grid_boxes(rng, n, extent=6), tied_scores(rng, n)      # crowded: fewer than 300 survive in any group
    args = (boxes, scores, None, off, 8192, 0.5, 300, 0.0)
    want = ref.box_nms(*args)
    assert want[1][1] == 0 and 0 < want[1][2] < 70
    assert 0 < want[1][0] < 300 and 0 < want[1][3] < 300      # neither large scan stops early: 128 and 65 blocks walked
    _, kept = positions(scores[:8192], None, boxes[:8192], 0.0, 8192, want[2][:8192])
    assert kept[HALF:].any()
    runs = [run(tspn, device, *args, scratch_fill=f) for f in (0x00, 0xff, 0xa5)]
    for r in runs:
        equal(r, want)
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))


# ----------------------------------------------------------------------- D. group counts on the offsets-chunk edges
# seeds at which the last group shows suppression (asserted below): from 256 groups on, the last chunk of offsets holds the
# last group's alone or little more
GROUP_SEEDS = {255: 755, 256: 762, 257: 763, 511: 1017, 512: 1051, 513: 1019}


@functools.lru_cache(maxsize=None)
def many_groups(G):
    rng = np.random.default_rng(GROUP_SEEDS[G])
    sizes = rng.integers(0, 6, G)
    sizes[-1] = 5
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    boxes, scores = grid_boxes(rng, n, extent=6), tied_scores(rng, n, levels=4)
    want = ref.box_nms(boxes, scores, None, off, 4, 0.3, 3, 0.0)
    return off, sizes, boxes, scores, want


@pytest.mark.parametrize("G", [255, 256, 257, 511, 512, 513])
def test_group_counts_on_the_offset_chunk_edges(tspn, device, G):
    """G + 1 offsets travel 256 per launch: one launch at 255, two from 256 (the second carries the end of the last group
    alone), three from 512.  A launcher that drops a chunk, or writes it to the wrong place, leaves the groups behind it
    with the fill's offsets: other indices, other counts, or nothing written."""
    off, sizes, boxes, scores, want = many_groups(G)
    suppressed = want[1] < np.minimum(sizes, 3)
    for c in range((G + 1 + 255) // 256):
        # the groups whose offsets the chunk holds: from 256 c on, or, where the chunk holds the last offset alone, the
        # last group
        first = 256 * c if 256 * c < G else G - 1
        assert suppressed[first:].any() and (want[1][first:] > 0).any(), (G, c)
    assert sizes[-1] > 0 and want[1][-1] > 0
    equal(run(tspn, device, boxes, scores, None, off, 4, 0.3, 3, 0.0), want)
    same_as_reference(tspn, device, None, scores, None, off, 4, 0.0, 3, 0.0)
    if G == 257:
        index, count, keep = tspn.ops.box_nms(dev(boxes, device), dev(scores, device), off.tolist(), 4, 0.3, 3, min_size=0.0,
                                              want_keep=True)
        equal(host(index, count, keep), want)


# --------------------------------------------------------------------- E. the selection alone at the big capacity
BIG_Q = 70000


def step_scores(n=BIG_Q):
    s = np.zeros(n, np.float32)
    s[100:1100] = 1.0
    s[60000:] = 0.5
    return s


@pytest.mark.parametrize("M", [4096, 4097, 8191, 8192])
def test_selection_alone_at_the_big_capacity(tspn, device, M):
    """70 000 candidates: 1000 ones, then the first M - 1000 of the 10 000 halves from index 60 000 on.  M = 4097 .. 8192
    sort 8192 slots with up to 4095 pad slots (pad slots sorted in front would show as index 0x7fffffff); at M = 8192 the
    cut among the ties falls on index 67 191, above 65 536: a tie-break that drops the third index byte cuts elsewhere."""
    scores = step_scores()
    expected = np.concatenate([np.arange(100, 1100), np.arange(60000, 60000 + M - 1000)])
    if M == 8192:
        assert expected[-1] == 67191 > 65536
    want = ref.box_nms(None, scores, None, [0, BIG_Q], M, 0.0, M, 0.0)
    assert want[1][0] == M and np.array_equal(want[0][0], expected)
    equal(run(tspn, device, None, scores, None, [0, BIG_Q], M, 0.0, M, 0.0), want)


@pytest.mark.parametrize("M", [4097, 8192])
def test_selection_alone_with_nans_above_65536(tspn, device, M):
    """NaN sorts first, the lower index first among them: 20 NaNs, three above index 65 536 and behind the cut of the
    halves, lead the selection in ascending order.  A tie-break that compares only the low 16 bits of the index, or a sort
    that breaks ties among equal keys by slot, orders them otherwise."""
    scores = step_scores()
    rng = np.random.default_rng(77)
    nans = np.sort(np.concatenate([rng.choice(60000, 17, replace=False), [69000, 69500, BIG_Q - 1]]))
    scores[nans] = np.nan
    assert len(nans) == 20 and (nans > 65536).sum() == 3 and nans[-3] > 60000 + M
    want = ref.box_nms(None, scores, None, [0, BIG_Q], M, 0.0, M, 0.0)
    assert np.array_equal(want[0][0, :20], nans) and want[1][0] == M
    equal(run(tspn, device, None, scores, None, [0, BIG_Q], M, 0.0, M, 0.0), want)


def test_selection_alone_three_groups_and_a_prefix(tspn, device):
    """Groups of 70 000, 10 and 4990 at M = 8192, post_topk 100: what is written is the first 100 of each group's
    selection (the middle group has 10, then -1).  A kernel that sorts post_topk slots where it selected M, or that keeps
    the first group's count for the next, writes something else."""
    rng = np.random.default_rng(79)
    off = [0, 70000, 70010, 75000]
    scores = np.concatenate([step_scores(), tied_scores(rng, 5000, levels=40)])
    scores[200:1200:7] = 2.0                          # the first 100 are not simply the first 100 ones
    want = ref.box_nms(None, scores, None, off, 8192, 0.0, 100, 0.0)
    full = ref.box_nms(None, scores, None, off, 8192, 0.0, 8192, 0.0)
    assert np.array_equal(want[0], full[0][:, :100]) and list(want[1]) == [100, 10, 100] and list(full[1]) == [8192, 10, 4990]
    assert full[0][0].max() > 65536 and bool((want[0][1, 10:] == -1).all())
    equal(run(tspn, device, None, scores, None, off, 8192, 0.0, 100, 0.0), want)


# ---------------------------------------------------------- F. the compositions and the final top-k at these sizes
@pytest.mark.parametrize("pre,post", [(6000, 6000), (6000, 1000)])
def test_rpn_proposals_where_6000_cuts(tspn, device, pre, post):
    """A 20 x 24 map of 15 anchors is 7200 candidates per image: the smallest at which pre_nms_topk = 6000 cuts, so the
    selection sorts 8192 slots and the NMS walks 94 column blocks.  Compared with the restatement of the selection stages
    fed the device's decode, as tests/test_gpu_detector.py does at 945 anchors."""
    rng = np.random.default_rng(pre + post)
    ops = tspn.ops
    B, H, W, A = 2, 20, 24, 15
    HWA = H * W * A
    cell = ref.cell_anchors()
    logits = (rng.integers(-20, 20, (B, H, W, A)) / np.float32(4)).astype(np.float32)
    deltas = (rng.standard_normal((B, H, W, 4 * A)) * 0.5).astype(np.float32)
    deltas.reshape(-1)[rng.integers(0, deltas.size, 12)] = np.nan
    deltas.reshape(-1)[rng.integers(0, deltas.size, 6)] = np.inf
    logits.reshape(-1)[rng.integers(0, logits.size, 5)] = np.inf
    sizes = np.array([[320.0, 384.0], [300.0, 370.0]], np.float32)
    d = [dev(x, device) for x in (logits, deltas, cell, sizes)]
    assert HWA == 7200 > pre
    cand, _, _ = ops.box_nms(None, d[0].reshape(-1), range(0, (B + 1) * HWA, HWA), pre, 0.0, pre)
    assert np.array_equal(cand.cpu().numpy(), ref.rpn_proposals_select(logits, pre))
    boxes, lg, valid = host(*ops.rpn_decode(cand, *d[:3], 16.0, d[3]))
    if post == pre:                                    # nothing stops the scan: image 0 at min_size 0, position by position
        _, _, keep = ref.box_nms(boxes[0], lg[0], valid[0], [0, pre], pre, 0.7, pre, 0.0)
        alive, kept = positions(lg[0], valid[0], boxes[0], 0.0, pre, keep)
        assert (alive[HALF:] & ~kept[HALF:]).sum() > 100 and kept[HALF:].sum() > 20
    for min_size in (0.0, 12.0):
        want = ref.rpn_proposals_finish(boxes, lg, valid, post, 0.7, min_size)
        got = host(*ops.rpn_proposals(*d[:3], 16.0, d[3], pre, post, 0.7, min_size))
        assert got[0].shape == (B, post, 4) and got[1].shape == (B, post)
        assert np.array_equal(got[2], want[2]) and 0 < got[2].min() and got[2].max() <= post
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_box_detections_with_280_class_groups(tspn, device):
    """The detector's default chunk: 8 images x 35 classes = 280 NMS groups of R = 70, past one launch of the group
    offsets; groups 256 .. 279 are image 7's classes 11 .. 34.  If their offsets were lost, image 7 would lose those
    classes' detections or gain suppressed ones."""
    rng = np.random.default_rng(280)
    ops = tspn.ops
    B, K, R = 8, 35, 70
    sizes = np.tile(np.array([[240.0, 320.0]], np.float32), (B, 1))
    xy = rng.integers(0, 80, (B, R, 2))                                                   # crowded: many IoUs above 0.5
    props = np.concatenate([xy, xy + rng.integers(30, 90, (B, R, 2))], axis=2).astype(np.float32)
    count = np.full(B, R, np.int64)
    count[2], count[5] = 41, 0
    z = (rng.integers(-6, 6, (B * R, K + 1)) / np.float32(2)).astype(np.float32)           # coarse logits: tied scores
    bd = (rng.standard_normal((B * R, 4 * K)) * 0.8).astype(np.float32)
    z[rng.integers(0, B * R, 3), rng.integers(0, K + 1, 3)] = np.nan
    bd[rng.integers(0, B * R, 3), rng.integers(0, 4 * K, 3)] = np.inf
    dz, dbd, dp, dc, ds = (dev(x, device) for x in (z, bd, props, count, sizes))
    for thr, nms, D in ((0.02, 0.5, 100), (0.0, 0.3, 1000)):
        sc, bx, vl = host(*ops.box_head_decode(dz, dbd, dp, dc, ds, thr))
        _, cnt, keep = ref.box_nms(bx.reshape(-1, 4), sc.reshape(-1), vl.reshape(-1), np.arange(B * K + 1) * R, R, nms, R, -1.0)
        tail = slice(256 * R, B * K * R)               # the candidates of groups 256 .. 279
        assert B * K == 280 and keep[tail].sum() > 24 and ((vl.reshape(-1)[tail] != 0) & (keep[tail] == 0)).sum() > 24
        want = ref.detections_finish(sc, bx, vl, nms, D)
        assert want[3][5] == 0 and want[3][7] > 0 and (want[2][7, :want[3][7]] >= 11).any()
        got = host(*ops.box_detections(dz, dbd, dp, dc, ds, thr, nms, D))
        assert np.array_equal(got[3], want[3])
        for g, w in zip(got[:3], want[:3]):
            assert g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("K,R", [(35, 1000), (80, 1000)])
@pytest.mark.parametrize("D", [100, 1024])
def test_detections_topk_at_the_box_heads_size(tspn, device, K, R, D):
    """Q = K R = 35 000 (the default head) and 80 000 candidates per image at D = 100 and at the limit 1024 (D = 1025 is
    refused: tests/test_detect_refusals_host.py), four score levels, more than D kept.  At Q = 80 000 the second image
    holds D / 2 top scores below i = r K + c = 66 000 and ties from there on, so the cut among ties lies above 65 536: a
    tie-break that loses the third index byte, or one that orders by the class-major position c R + r, picks other rows."""
    rng = np.random.default_rng(K + D)
    B, top = 2, np.float32(0.75)
    scores = (rng.integers(0, 4, (B, K, R)) / np.float32(4)).astype(np.float32)
    boxes = rng.uniform(0, 50, (B, K, R, 4)).astype(np.float32)
    keep = (rng.random((B, K, R)) < 0.4).astype(np.uint8)
    flat = np.arange(R)[None, :] * K + np.arange(K)[:, None]                             # i = r K + c at [c, r]
    if K * R > 65536:
        low = flat < 66000
        scores[1][low & (scores[1] == top)] = 0.5
        few = rng.choice(np.flatnonzero((low & (keep[1] != 0)).reshape(-1)), D // 2, replace=False)
        scores[1].reshape(-1)[few] = top
    ob, os_, oc, cnt = host(*tspn.ops.detections_topk(dev(scores, device), dev(boxes, device), dev(keep, device), D))
    for b in range(B):
        r, c = np.nonzero(keep[b].T)                                                     # ascending r K + c
        order = np.lexsort((r * K + c, -scores[b][c, r].astype(np.float64)))
        assert len(order) > D
        last, nxt = order[D - 1], order[D]
        assert scores[b][c[last], r[last]] == scores[b][c[nxt], r[nxt]] == top           # the cut falls among ties
        if b == 1 and K * R > 65536:
            assert r[last] * K + c[last] > 65536
        order = order[:D]
        assert cnt[b] == D
        assert np.array_equal(oc[b], c[order]) and np.array_equal(os_[b], scores[b][c[order], r[order]])
        assert np.array_equal(ob[b], boxes[b][c[order], r[order]])
