"""Tracklet linking on the device (csrc/link/tspn_link.hip) against the numpy restatement (tests/link_reference.py):
every output array of the link pass, the fill pass and the segment cut, bit for bit.  The shapes are the smallest at which
the kernels take another path: candidate counts around a wave and at the limit, live counts around a wave, a pass of the
waves and a pass of the workgroup, frame counts around a pass of the fill wave."""
import ctypes

import numpy as np
import pytest
import torch

import link_reference as ref
import sentinel_buffers as sb

pytestmark = pytest.mark.gpu

KEYS = ("track_of_det", "n_tracks", "dropped", "first", "last", "hits", "cls", "score")


def to_dev(det, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in det)


def gpu_link(tspn, device, det, off, **kw):
    out = tspn.ops.link_detections(*to_dev(det, device), off, **kw)
    return dict(zip(KEYS, (o.cpu().numpy() for o in out)))


def same(got, want, what=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def check(tspn, device, det, off=None, stats=None, **kw):
    off = [0, len(det[3])] if off is None else off
    want = ref.link(*det, off, stats=stats, **kw)
    got = gpu_link(tspn, device, det, off, **kw)
    same(got, want)
    return want


def check_fill(tspn, device, det, off, res, sv, st):
    want_b, want_s = ref.fill(res, det[0], off, sv, st)
    d = torch.device(device)
    got_b, got_s = tspn.ops.link_fill(torch.from_numpy(det[0]).to(d), torch.from_numpy(res["track_of_det"]).to(d),
                                      torch.from_numpy(res["first"]).to(d), torch.from_numpy(res["last"]).to(d),
                                      torch.from_numpy(np.asarray(sv, np.int64)).to(d),
                                      torch.from_numpy(np.asarray(st, np.int64)).to(d), off)
    assert got_b.dtype == torch.float32 and got_s.dtype == torch.uint8
    assert np.array_equal(got_b.cpu().numpy(), want_b) and np.array_equal(got_s.cpu().numpy(), want_s)
    return want_b, want_s


def concat(dets):
    """Several videos' detections (equal D) -> one batch and its offsets."""
    off = np.concatenate([[0], np.cumsum([len(d[3]) for d in dets])]).tolist()
    return tuple(np.concatenate([d[k] for d in dets]) for k in range(4)), off


def no_frames(det):
    """A video without a frame, with the D of `det`."""
    return tuple(x[:0] for x in det[:4])


def grid_boxes(n, rng, jitter=0.0, size=20.0, pitch=40.0, cols=40):
    i = np.arange(n)
    x = (i % cols) * pitch + (rng.uniform(-jitter, jitter, n) if jitter else 0)
    y = (i // cols) * pitch + (rng.uniform(-jitter, jitter, n) if jitter else 0)
    return np.stack([x, y, x + size, y + size], 1).astype(np.float32)


def grid_frames(counts, D, rng, jitter=1.5, which=None):
    """Frames with counts[f] detections, each a jittered cell of one fixed grid, in a random order."""
    F = len(counts)
    boxes, scores = np.zeros((F, D, 4), np.float32), np.zeros((F, D), np.float32)
    classes, count = np.zeros((F, D), np.int64), np.zeros(F, np.int64)
    total = max(max(counts), 1) if which is None else max(int(max(w.max() for w in which if len(w))) + 1, 1)
    for f, n in enumerate(counts):
        cells = rng.permutation(total)[:n] if which is None else rng.permutation(np.asarray(which[f], np.int64))
        all_boxes = grid_boxes(total, rng, jitter)
        boxes[f, :n] = all_boxes[cells]
        scores[f, :n] = rng.uniform(0.3, 1.0, n).astype(np.float32)
        classes[f, :n] = 1 + cells % 3
        count[f] = n
    return boxes, scores, classes, count


# ------------------------------------------------------------------------------------------ shape and capacity edges
def test_candidate_counts_at_the_block_edges(tspn, device):
    rng = np.random.RandomState(0)
    det = grid_frames([1024, 0, 1, 63, 64, 65, 100, 257, 1024, 1024], 1024, rng)
    stats = {}
    want = check(tspn, device, det, stats=stats, min_hits=1, max_live=2048)
    assert stats["max_live_seen"] >= 1024 and want["n_tracks"][0] >= 1024 and want["hits"][0].max() >= 3


def test_live_counts_past_a_wave_and_a_pass(tspn, device):
    rng = np.random.RandomState(1)
    for live in (1, 64, 65, 256, 257, 1025):
        n = min(live, 1024)
        every, third = np.arange(n), np.arange(0, n, 3)
        extra = np.arange(n, live)                                # the 1025th track comes in a frame of its own
        which = [every, extra, every, third, third, every]        # max_age 1: two thirds die and the rest moves down
        det = grid_frames([len(w) for w in which], max(n, 4), rng, which=which)
        stats = {}
        want = check(tspn, device, det, stats=stats, min_hits=1, max_age=1, max_live=2048)
        assert stats["max_live_seen"] == live and want["dropped"][0] == 0, live
        assert want["n_tracks"][0] > live or live == 1, live      # the tracks that died come back under new ids


def test_births_past_max_live_and_max_tracks(tspn, device):
    det = ref.generated_scene(0)[:4]
    want = check(tspn, device, det, max_live=5, max_tracks=7)
    assert want["dropped"][0] > 0 and want["n_tracks"][0] == 7 and want["first"].shape == (1, 7)
    want = check(tspn, device, det, max_live=5)
    assert want["dropped"][0] > 0 and want["n_tracks"][0] > 7


def test_a_frame_that_needs_four_rounds(tspn, device):
    for links, rounds in ((7, 4), (6, 3), (15, 8)):
        stats = {}
        check(tspn, device, ref.chain_frame(links), stats=stats, min_hits=1)
        assert stats["max_rounds"] == rounds


def test_integer_grid_ties(tspn, device):
    for seed in range(3):
        rng = np.random.RandomState(seed)
        frames = []
        for _ in range(6):
            xy = 4 * rng.randint(0, 12, (40, 2))
            frames.append([(x, y, x + 8, y + 8, 0.5, 1) for x, y in xy])
        stats = {}
        want = check(tspn, device, ref.pack(frames, 40), stats=stats, iou_thresh=0.1, min_hits=1, class_aware=False)
        assert stats["max_rounds"] >= 2 and want["hits"][0].max() >= 3


# ------------------------------------------------------------------------------------------------ lifetime and gates
def test_both_age_edges_and_the_tentative_death(tspn, device):
    box = (10, 10, 50, 50, 0.9, 1)
    cases = [([[box], [], [], [box]], [0, -1, -1, 0]), ([[box], [], [], [], [box]], [0, -1, -1, -1, 1])]
    for frames, ids in cases:                                     # a gap of max_age survives, one more does not
        want = check(tspn, device, ref.pack(frames, 1), min_hits=1, max_age=3)
        assert list(want["track_of_det"][:, 0]) == ids
    cases = [([[box], [], [box]], [0, -1, 1]), ([[box], [box], [], [box]], [0, 0, -1, 1]),
             ([[box], [box], [box], [], [box]], [0, 0, 0, -1, 0])]
    for frames, ids in cases:                                     # tentative tracks die at their first miss
        want = check(tspn, device, ref.pack(frames, 1))
        assert list(want["track_of_det"][:, 0]) == ids
    want = check(tspn, device, ref.pack([[box], [box]], 1), min_hits=1, max_age=0)
    assert list(want["track_of_det"][:, 0]) == [0, 1]


def test_class_aware_on_and_off(tspn, device):
    a, b = (0, 0, 40, 40, 0.9, 1), (4, 0, 44, 40, 0.8, 2)
    frames = [[a, b], [(4, 0, 44, 40, 0.9, 1), (0, 0, 40, 40, 0.8, 2)], [(2, 0, 42, 40, 0.9, 2)]]
    on = check(tspn, device, ref.pack(frames, 2), min_hits=1)
    off = check(tspn, device, ref.pack(frames, 2), min_hits=1, class_aware=False)
    assert list(on["track_of_det"][1]) == [0, 1] and list(off["track_of_det"][1]) == [1, 0]   # the class, or the better IoU
    big = np.int64(2 ** 40 + 1)                                   # classes are compared as int64
    frames = [[(0, 0, 40, 40, 0.9, 1)], [(0, 0, 40, 40, 0.9, big)], [(0, 0, 40, 40, 0.9, big)]]
    want = check(tspn, device, ref.pack(frames, 1), min_hits=1)
    assert list(want["track_of_det"][:, 0]) == [0, 1, 1] and want["cls"][0, 1] == big


def test_non_finite_boxes_and_scores(tspn, device):
    nan, inf = float("nan"), float("inf")
    frame = [(0, 0, 40, 40, 0.9, 1), (100, 0, nan, 40, 0.9, 1), (200, 0, 240, inf, 0.9, 1), (300, 0, 340, 40, nan, 1),
             (400, 0, 440, 40, inf, 1), (500, -inf, 540, 40, 0.9, 1), (600, 0, 640, 40, -inf, 1), (700, 0, 740, 40, 0.5, 1)]
    det = ref.pack([frame, frame, frame], 8)
    want = check(tspn, device, det, min_hits=1)
    assert list(want["track_of_det"][2]) == [0, -1, -1, -1, -1, -1, -1, 1]
    det[3][:] = [2000, -3, 1]                                     # a count past D, a negative one, one that cuts
    want = check(tspn, device, det, min_hits=1)
    assert list(want["track_of_det"][1]) == [-1] * 8 and list(want["track_of_det"][2]) == [0] + [-1] * 7
    # a velocity that carries the prediction past the largest float: the IoU is 0 or a NaN, never an edge
    frames = [[(0, 0, 2e38, 1e-3, 0.9, 1)], [(1e38, 0, 3e38, 1e-3, 0.9, 1)], [(2e38, 0, 3.3e38, 1e-3, 0.9, 1)],
              [(-3e38, 0, 3e38, 1e-3, 0.9, 1)], [(-3e38, 0, 3e38, 1e-3, 0.9, 1)]]
    want = check(tspn, device, ref.pack(frames, 1), min_hits=1)
    assert list(want["track_of_det"][:3, 0]) == [0, 0, 1]
    # inverted and empty boxes are finite: candidates, with areas of either sign
    frames = [[(40, 40, 0, 0, 0.9, 1), (5, 5, 5, 5, 0.9, 1), (0, 0, 40, 40, 0.9, 1)]] * 3
    check(tspn, device, ref.pack(frames, 3), min_hits=1, iou_thresh=0.01)


def test_scores_at_and_just_under_min_score(tspn, device):
    q = np.float32(0.25)
    under, over = np.nextafter(q, np.float32(0)), np.nextafter(q, np.float32(1))
    frame = [(100 * i, 0, 100 * i + 40, 40, s, 1) for i, s in enumerate((q, under, over, 0.0, -0.0, -1e-30, 1e-45))]
    det = ref.pack([frame, frame], 7)
    want = check(tspn, device, det, min_hits=1, min_score=0.25)
    assert list(want["track_of_det"][0]) == [0, -1, 1, -1, -1, -1, -1]
    want = check(tspn, device, det, min_hits=1)                   # the default 0.0: -0.0 passes, a negative score does not
    assert list(want["track_of_det"][0]) == [0, 1, 2, 3, 4, -1, 5]
    want = check(tspn, device, det, min_hits=1, min_score=-1.0)
    assert want["n_tracks"][0] == 7


# -------------------------------------------------------------------------------------- the scenes of the host tests
def test_constant_velocity_scene(tspn, device):
    det = ref.constant_velocity_scene()
    want = check(tspn, device, det)
    assert want["n_tracks"][0] == 2 and list(want["hits"][0, :2]) == [37, 40]
    tb, state = check_fill(tspn, device, det, [0, 40], want, *ref.confirmed(want))
    assert list(state[0, 9:13]) == [1, 2, 2, 1] and np.array_equal(tb[0, 10], [400, 100, 480, 180])


def test_generated_scenes(tspn, device):
    scenes = [ref.generated_scene(seed) for seed in range(8)]
    det, off = concat([s[:4] for s in scenes])
    got = gpu_link(tspn, device, det, off)
    for v, scene in enumerate(scenes):                            # every video against the restatement of it alone
        want = ref.link(*scene[:4], [0, 120])
        for k in KEYS:
            part = got[k][off[v]:off[v + 1]] if k == "track_of_det" else got[k][v:v + 1]
            assert np.array_equal(part, want[k]), (v, k)
        ids = np.nonzero(got["hits"][v] >= 3)[0]
        tod = got["track_of_det"][off[v]:off[v + 1]]
        owners = [set(scene[4][tod == k].tolist()) for k in ids]
        assert len(ids) == 6 and sorted(next(iter(o)) for o in owners) == list(range(6)) and all(len(o) == 1 for o in owners)


# ------------------------------------------------------------------------------------------------------------ batches
def test_batches_equal_their_videos_alone(tspn, device):
    cv = ref.constant_velocity_scene()
    rng = np.random.RandomState(3)
    grid = grid_frames([4, 3, 4, 4, 2, 4, 4], 4, rng)
    empty = no_frames(cv)
    for videos in ([cv], [grid, empty, cv], [(cv, grid, empty)[i % 3] for i in range(70)]):
        det, off = concat(videos)
        want = check(tspn, device, det, off, min_hits=2)
        assert len(want["n_tracks"]) == len(videos)
        sv, st = ref.confirmed(want, 2)
        tb, state = check_fill(tspn, device, det, off, want, sv, st)
        assert tb.shape[1] == 40
        for v in sorted(set(range(len(videos))) & {0, 1, 2, 69}):
            alone = ref.link(*videos[v], [0, len(videos[v][3])], min_hits=2)
            assert np.array_equal(want["track_of_det"][off[v]:off[v + 1]], alone["track_of_det"])
            assert all(np.array_equal(want[k][v], alone[k][0]) for k in KEYS[1:])
            if len(videos[v][3]):
                a_sv, a_st = ref.confirmed(alone, 2)
                a_tb, a_state = check_fill(tspn, device, videos[v], [0, len(videos[v][3])], alone, a_sv, a_st)
                mine = sv == v
                assert np.array_equal(tb[mine][:, :a_tb.shape[1]], a_tb) and np.array_equal(state[mine][:, :a_tb.shape[1]], a_state)
                assert not state[mine][:, a_tb.shape[1]:].any()


# ---------------------------------------------------------------------------------------------------------- fill pass
def fill_scene(num_frames, D=3):
    """A moving object with gaps of one frame, a slow one seen every 30th frame (gaps of max_age) and lone detections."""
    frames = []
    for t in range(num_frames):
        rows = []
        if t % 5 != 3:
            rows.append((10 + 7.3 * t, 20 + 0.7 * t, 90 + 7.3 * t, 100 + 0.7 * t, 0.9, 1))
        if t % 30 == 0:
            rows.append((3000 + t / 3.0, 500, 3100 + t / 3.0, 640, 0.8, 2))
        if t % 17 == 5:
            rows.append((100.0 * t, 2000, 100.0 * t + 50, 2050, 0.6, 3))
        frames.append(rows)
    return ref.pack(frames, D)


def test_fill_lengths_gaps_and_single_frame_tracks(tspn, device):
    videos = [fill_scene(n) for n in (1, 63, 64, 65, 300)]
    det, off = concat(videos)
    want = check(tspn, device, det, off, min_hits=1)
    sv, st = ref.confirmed(want, 1)
    tb, state = check_fill(tspn, device, det, off, want, sv, st)
    assert tb.shape == (len(sv), 300, 4)
    last = sv == 4
    assert (want["first"][4, st[last]] == want["last"][4, st[last]]).sum() >= 10         # tracks of a single detection
    runs = ["".join(map(str, r)) for r in state[last]]
    assert any("1" + "2" * 29 + "1" in r for r in runs) and any("121" in r for r in runs) and any(r.count("1") == 1 for r in runs)
    assert not state[sv == 0][:, 1:].any() and state[sv == 0][:, 0].all()                 # the one-frame video


def test_fill_of_a_caller_selected_subset(tspn, device):
    videos = [fill_scene(65), fill_scene(40)]
    det, off = concat(videos)
    want = check(tspn, device, det, off, min_hits=1)
    n0, n1 = int(want["n_tracks"][0]), int(want["n_tracks"][1])
    # some tracks out of order, a twin, a track never born, ids and videos outside the tables
    sv = [1, 0, 0, 1, 0, 1, 2, -1, 0, 0]
    st = [1, n0 - 1, 0, 1, n0, 0, 0, 0, 16384, -1]
    tb, state = check_fill(tspn, device, det, off, want, sv, st)
    assert np.array_equal(tb[0], tb[3]) and state[0].any() and not state[4].any() and not state[6:].any() and n1 > 1
    check_fill(tspn, device, det, off, want, [], [])


# ---------------------------------------------------------------------------------------------------- memory contract
def guarded(shape, device, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), fill, dtype=dtype, device=device)
    return buf, buf[32:32 + n].view(shape)


def inside_only(buf, view, fill, what, all_written=True):
    b, n = buf.cpu(), view.numel()
    assert bool((b[:32] == fill).all()) and bool((b[32 + n:] == fill).all()), f"{what}: wrote outside"
    if all_written:
        assert int((b[32:32 + n] == fill).sum()) == 0, f"{what}: outputs never written"


def test_outputs_and_scratch_are_written_inside_only(tspn, device):
    lib, A_ = tspn._abi.lib(), tspn._abi
    scene = ref.generated_scene(1, num_frames=40)
    det, off = concat([scene[:4], no_frames(scene), ref.generated_scene(2, num_frames=33)[:4]])
    F, D, V, MT = det[1].shape[0], det[1].shape[1], 3, 50
    want = ref.link(*det, off, max_tracks=MT)
    b, s, c, n = to_dev(det, device)
    arr = (ctypes.c_int64 * len(off))(*off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fill = {torch.int32: -77, torch.int64: -77, torch.uint8: 77}
    outs = {k: guarded(sh, device, dt, fill[dt]) for k, sh, dt in (
        ("track_of_det", (F, D), torch.int32), ("n_tracks", (V,), torch.int64), ("dropped", (V,), torch.int64),
        ("first", (V, MT), torch.int32), ("last", (V, MT), torch.int32), ("hits", (V, MT), torch.int32),
        ("cls", (V, MT), torch.int64))}
    score_buf, score = sb.held((V, MT), device)
    need = lib.tspn_link_scratch_bytes(V, 64, MT, 0, 0, 0)
    ws_buf, ws = sb.held((need // 4,), device)
    tspn.ops._status_block()
    rc = lib.tspn_link_detections_f32(sb.p(b), sb.p(s), sb.p(c), sb.p(n), arr, V, F, D, 0.3, 30, 3, 0.0, 1, 64, MT,
                                      *[sb.p(outs[k][1]) for k in KEYS[:-1]], sb.p(score), sb.p(ws), need, stream)
    assert rc == A_.TSPN_OK, lib.tspn_last_error()
    torch.cuda.synchronize()
    for k in KEYS[:-1]:
        # -77 is no value of any output but cls, whose table holds the scene's classes 1 ... 3 and -1
        inside_only(outs[k][0], outs[k][1], -77, k)
        assert np.array_equal(outs[k][1].cpu().numpy(), want[k]), k
    sb.assert_written_inside_only(score_buf, score, "trk_score")
    assert np.array_equal(score.cpu().numpy(), want["score"])
    edge = ws_buf.cpu()
    assert bool((edge[:sb.GUARD] == sb.sentinel_of(edge)).all()) and bool((edge[-sb.GUARD:] == sb.sentinel_of(edge)).all())
    # the fill pass
    sv, st = ref.confirmed(want)
    want_b, want_s = ref.fill(want, det[0], off, sv, st)
    R, Fmax = want_s.shape
    d_sv, d_st = torch.from_numpy(sv).to(device), torch.from_numpy(st).to(device)
    box_buf, boxes = sb.held((R, Fmax, 4), device)
    state_buf, state = guarded((R, Fmax), device, torch.uint8, 77)
    need = lib.tspn_link_scratch_bytes(V, 0, MT, R, Fmax, 1)
    ws_buf, ws = sb.held((need // 4,), device)
    rc = lib.tspn_link_fill_f32(sb.p(b), sb.p(outs["track_of_det"][1]), arr, V, F, D, sb.p(outs["first"][1]),
                                sb.p(outs["last"][1]), MT, sb.p(d_sv), sb.p(d_st), R, sb.p(boxes), sb.p(state), sb.p(ws), need,
                                stream)
    assert rc == A_.TSPN_OK, lib.tspn_last_error()
    torch.cuda.synchronize()
    sb.assert_written_inside_only(box_buf, boxes, "out_boxes")
    inside_only(state_buf, state, 77, "out_state")
    assert np.array_equal(boxes.cpu().numpy(), want_b) and np.array_equal(state.cpu().numpy(), want_s) and R >= 6
    edge = ws_buf.cpu()
    assert bool((edge[:sb.GUARD] == sb.sentinel_of(edge)).all()) and bool((edge[-sb.GUARD:] == sb.sentinel_of(edge)).all())
    # a refused call writes nothing
    rc = lib.tspn_link_fill_f32(sb.p(b), sb.p(outs["track_of_det"][1]), arr, V, F, D, sb.p(outs["first"][1]),
                                sb.p(outs["last"][1]), MT, sb.p(d_sv), sb.p(d_st), R, sb.p(boxes), sb.p(state), sb.p(ws),
                                need - 1, stream)
    sb.refused(tspn, rc, A_.TSPN_EWORKSPACE, "short scratch")


def test_the_result_does_not_depend_on_the_scratch(tspn, device):
    det, off = concat([ref.generated_scene(3, num_frames=60)[:4], fill_scene(60, 16)])
    ops = tspn.ops
    d = to_dev(det, device)
    need = tspn._abi.lib().tspn_link_scratch_bytes(2, 1024, 16384, 0, 0, 0)
    results = []
    for pattern in (0, 0xFF, None):
        ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=device) if pattern is None else \
            torch.full((need,), pattern, dtype=torch.uint8, device=device)
        out = ops.link_detections(*d, off, workspace=ws)
        at = torch.nonzero(out[5] >= 3)
        fneed = tspn._abi.lib().tspn_link_scratch_bytes(2, 0, 16384, at.shape[0], 60, 1)
        fws = torch.randint(0, 256, (fneed,), dtype=torch.uint8, device=device) if pattern is None else \
            torch.full((fneed,), pattern, dtype=torch.uint8, device=device)
        tb, state = ops.link_fill(d[0], out[0], out[3], out[4], at[:, 0].contiguous(), at[:, 1].contiguous(), off,
                                  workspace=fws)
        results.append([o.cpu().numpy() for o in out] + [tb.cpu().numpy(), state.cpu().numpy()])
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    want = ref.link(*det, off)
    same(dict(zip(KEYS, results[0][:8])), want)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.link_detections(*d, off, workspace=torch.empty(need - 1, dtype=torch.uint8, device=device))


# --------------------------------------------------------------------------------------------------------- downstream
def test_segment_and_video_tracklets(tspn, device):
    scenes = [ref.generated_scene(4)[:4], ref.generated_scene(5, num_frames=75)[:4]]
    det, off = concat(scenes)
    want = ref.link(*det, off)
    sv, st = ref.confirmed(want)
    want_b, want_s = ref.fill(want, det[0], off, sv, st)
    tracks, segments = tspn.video_tracklets(to_dev(det, device), seg_len=30, stride=15, max_tracklets=4, video_off=off)
    assert isinstance(tracks, tspn.Tracks) and np.array_equal(tracks.track_boxes.cpu().numpy(), want_b)
    assert np.array_equal(tracks.state.cpu().numpy(), want_s) and np.array_equal(tracks.sel_track.cpu().numpy(), st)
    spans = [(v, s, e) for v, n in enumerate((120, 75)) for s, e in ref.segments_of(n)]
    assert [(g["video"], g["fstart"], g["fend"]) for g in segments] == spans and len(spans) == 7 + 4
    for g in segments:
        for cap in (4, 64):
            boxes, ids, classes, scores = ref.segment_tracklets(want, want_b, sv, st, g["video"], g["fstart"], g["fend"], cap)
            got = g if cap == 4 else dict(zip(("boxes", "ids", "classes", "scores"),
                                              tspn.segment_tracklets(tracks, g["video"], g["fstart"], g["fend"])))
            assert np.array_equal(got["boxes"].cpu().numpy(), boxes) and np.array_equal(got["ids"].cpu().numpy(), ids)
            assert np.array_equal(got["classes"].cpu().numpy(), classes) and np.array_equal(got["scores"].cpu().numpy(), scores)
            assert len(ids) == (4 if cap == 4 else 6) and got["boxes"].dtype == torch.float32 and got["ids"].dtype == torch.int64
    # a caller's selection, in an order of its own
    pick = (torch.tensor([1, 0, 0, 1], device=device), torch.tensor([2, 5, 1, 0], device=device))
    mine = tspn.link_detections(to_dev(det, device), off, select=pick)
    b2, _ = ref.fill(want, det[0], off, [1, 0, 0, 1], [2, 5, 1, 0])
    assert np.array_equal(mine.track_boxes.cpu().numpy(), b2)
    got = tspn.segment_tracklets(mine, 0, 0, 120)
    exp = ref.segment_tracklets(want, b2, np.array([1, 0, 0, 1]), np.array([2, 5, 1, 0]), 0, 0, 120)
    assert all(np.array_equal(g.cpu().numpy(), e) for g, e in zip(got, exp)) and len(exp[1]) >= 1
    with pytest.raises(ValueError, match="outside"):
        tspn.segment_tracklets(tracks, 1, 60, 90)


def test_traj_cls_accepts_the_segments(tspn, device):
    det = ref.generated_scene(6, num_frames=45)[:4]
    _, segments = tspn.video_tracklets(to_dev(det, device))
    assert [(g["fstart"], g["fend"]) for g in segments] == [(0, 30), (15, 45)]
    for g in segments:
        n = g["ids"].shape[0]
        logits = torch.nn.functional.one_hot(g["classes"], 35).float()
        trajs = tspn.dataset.tracklets_to_traj_cls(g["boxes"], logits, g["fstart"], vsig="v", scores=g["scores"])
        assert n >= 4 and len(trajs) == n and all(t["pstart"] == g["fstart"] and t["pend"] == g["fend"] for t in trajs)
        assert [t["category"] for t in trajs] == g["classes"].tolist() and len(trajs[0]["rois"]) == 30
        assert trajs[0]["rois"][0] == tuple(float(x) for x in g["boxes"][0, 0].tolist())
