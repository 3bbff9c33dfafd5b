"""Numpy restatement of tracklet linking ("tracklet linking"): the deterministic IoU tracker with
constant-velocity prediction of csrc/link/tspn_link.hip, in fp32 and in the statement order of the design, with the greedy
match as a walk over the sorted edges.  `match_rounds` is the mutual-best form the kernel runs and counts its rounds; both
forms give the same pairs.  `use_velocity=False` switches the prediction off (a switch of the tests only).

Everything here is written for this project; no tracker's text is restated."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(iou_thresh=0.3, max_age=30, min_hits=3, min_score=0.0, class_aware=True, max_live=1024, max_tracks=16384)
ABSENT, DETECTED, INTERPOLATED = 0, 1, 2


def finite_f32(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v) <= F32(3.402823466e38)           # false for NaN


def iou_f32(p, boxes):
    """IoU of the (predicted) track box p [4] with the detections [n, 4], fp32, in suppresses()'s order: i the track, j the
    detection; a NaN of the track box stays in the maxima and minima as the kernel's comparisons leave it."""
    p = np.asarray(p, F32)
    b = np.asarray(boxes, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        iarea = (p[2] - p[0]) * (p[3] - p[1])
        jarea = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        xx1 = np.where(p[0] < b[:, 0], b[:, 0], p[0])
        yy1 = np.where(p[1] < b[:, 1], b[:, 1], p[1])
        xx2 = np.where(b[:, 2] < p[2], b[:, 2], p[2])
        yy2 = np.where(b[:, 3] < p[3], b[:, 3], p[3])
        dw, dh = xx2 - xx1, yy2 - yy1
        w = np.where(F32(0) < dw, dw, F32(0))
        h = np.where(F32(0) < dh, dh, F32(0))
        inter = (w * h).astype(F32)
        return (inter / ((iarea + jarea).astype(F32) - inter)).astype(F32)


def predict(last, prev, t_last, t_prev, hits, t, use_velocity=True):
    """The box a track is matched with at frame t."""
    if hits < 2 or not use_velocity:
        return last.copy()
    with np.errstate(all="ignore"):
        step = (last - prev).astype(F32) / F32(t_last - t_prev)
        return (last + (step * F32(t - t_last)).astype(F32)).astype(F32)


def edge_matrix(pred, tcls, cbox, ccls, iou_thresh, class_aware):
    """(iou [L, C] fp32, edge [L, C] bool) between the live tracks and the candidates."""
    L, C = len(pred), len(cbox)
    iou = np.zeros((L, C), F32)
    for i in range(L):
        iou[i] = iou_f32(pred[i], cbox)
    with np.errstate(invalid="ignore"):
        edge = iou >= F32(iou_thresh)
    if class_aware and L and C:
        edge &= np.asarray(tcls)[:, None] == np.asarray(ccls)[None, :]
    return iou, edge


def match_sorted(iou, edge):
    """Greedy over the edges in the order (IoU descending, track ascending, candidate ascending): [(track, candidate)]."""
    ti, ci = np.nonzero(edge)
    order = np.lexsort((ci, ti, -iou[ti, ci].astype(np.float64)))
    tused, cused, pairs = set(), set(), []
    for k in order:
        i, c = int(ti[k]), int(ci[k])
        if i not in tused and c not in cused:
            tused.add(i)
            cused.add(c)
            pairs.append((i, c))
    return sorted(pairs)


def match_rounds(iou, edge):
    """The same pairs by rounds of mutual best: a round takes every edge that is its track's best (IoU descending,
    candidate ascending) and its candidate's best (IoU descending, track ascending).  Returns (pairs, rounds that took
    at least one pair)."""
    edge = edge.copy()
    key = np.where(edge, iou, F32(-1))
    pairs, rounds = [], 0
    while edge.any():
        key = np.where(edge, iou, F32(-1))
        row_best = key.argmax(axis=1)                    # the first maximum: the lowest candidate
        col_best = key.argmax(axis=0)                    # the lowest track
        took = [(i, int(row_best[i])) for i in range(edge.shape[0])
                if edge[i, row_best[i]] and col_best[row_best[i]] == i]
        assert took
        for i, c in took:
            edge[i, :] = False
            edge[:, c] = False
        pairs += took
        rounds += 1
    return sorted(pairs), rounds


def link(boxes, scores, classes, count, video_off, iou_thresh=0.3, max_age=30, min_hits=3, min_score=0.0, class_aware=True,
         max_live=1024, max_tracks=16384, use_velocity=True, stats=None):
    """The link pass.  Returns a dict of track_of_det int32 [F, D], n_tracks / dropped int64 [V] and the per-track tables
    first / last / hits int32, cls int64, score fp32, each [V, max_tracks] (-1, -1, 0, -1, 0 past n_tracks).  `stats`: a
    dict that receives max_rounds and max_live_seen."""
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    classes = np.asarray(classes, np.int64)
    count = np.asarray(count, np.int64)
    video_off = [int(v) for v in video_off]
    V = len(video_off) - 1
    F, D = scores.shape
    out = dict(track_of_det=np.full((F, D), -1, np.int32), n_tracks=np.zeros(V, np.int64), dropped=np.zeros(V, np.int64),
               first=np.full((V, max_tracks), -1, np.int32), last=np.full((V, max_tracks), -1, np.int32),
               hits=np.zeros((V, max_tracks), np.int32), cls=np.full((V, max_tracks), -1, np.int64),
               score=np.zeros((V, max_tracks), F32))
    max_rounds = max_live_seen = 0
    for v in range(V):
        f0, Fv = video_off[v], video_off[v + 1] - video_off[v]
        live, n_ids, dropped = [], 0, 0           # live: dicts, ascending id
        for t in range(Fv):
            f = f0 + t
            live = [k for k in live if (t - k["t_last"] <= max_age if k["hits"] >= min_hits else t - k["t_last"] == 1)]
            n = int(min(max(count[f], 0), D))
            ok = finite_f32(boxes[f, :n]).all(axis=1) & finite_f32(scores[f, :n])
            with np.errstate(invalid="ignore"):
                ok &= scores[f, :n] >= F32(min_score)
            cand = np.nonzero(ok)[0]
            pred = [predict(k["last"], k["prev"], k["t_last"], k["t_prev"], k["hits"], t, use_velocity) for k in live]
            iou, edge = edge_matrix(pred, [k["cls"] for k in live], boxes[f, cand], classes[f, cand], iou_thresh, class_aware)
            pairs = match_sorted(iou, edge)
            if stats is not None:
                by_rounds, r = match_rounds(iou, edge)
                assert by_rounds == pairs
                max_rounds = max(max_rounds, r)
            taken = set()
            for i, c in pairs:
                k, d = live[i], int(cand[c])
                k["prev"], k["t_prev"] = k["last"], k["t_last"]
                k["last"], k["t_last"] = boxes[f, d].copy(), t
                k["hits"] += 1
                k["score_sum"] += float(scores[f, d])
                out["track_of_det"][f, d] = k["id"]
                taken.add(d)
            for d in cand:
                d = int(d)
                if d in taken:
                    continue
                if len(live) < max_live and n_ids < max_tracks:
                    live.append(dict(id=n_ids, cls=int(classes[f, d]), first=t, t_last=t, t_prev=t, hits=1,
                                     last=boxes[f, d].copy(), prev=boxes[f, d].copy(), score_sum=float(scores[f, d])))
                    out["track_of_det"][f, d] = n_ids
                    out["first"][v, n_ids], out["cls"][v, n_ids] = t, int(classes[f, d])
                    n_ids += 1
                else:
                    dropped += 1
            for k in live:                              # the tables follow every update
                out["last"][v, k["id"]], out["hits"][v, k["id"]] = k["t_last"], k["hits"]
                out["score"][v, k["id"]] = F32(k["score_sum"] / k["hits"])
            max_live_seen = max(max_live_seen, len(live))
        out["n_tracks"][v], out["dropped"][v] = n_ids, dropped
    if stats is not None:
        stats["max_rounds"], stats["max_live_seen"] = max_rounds, max_live_seen
    return out


def confirmed(res, min_hits=3):
    """(video, track) of the default selection: the confirmed tracks, by video, ascending id."""
    sv, st = [], []
    for v in range(len(res["n_tracks"])):
        ids = np.nonzero(res["hits"][v, :res["n_tracks"][v]] >= min_hits)[0]
        sv += [v] * len(ids)
        st += [int(i) for i in ids]
    return np.asarray(sv, np.int64), np.asarray(st, np.int64)


def fill(res, boxes, video_off, sel_video, sel_track):
    """The fill pass: (track_boxes fp32 [R, Fmax, 4], state uint8 [R, Fmax]) of the selected tracks; a selection outside the
    tables gives an absent row."""
    boxes = np.asarray(boxes, F32)
    video_off = [int(v) for v in video_off]
    V = len(video_off) - 1
    Fmax = max([video_off[v + 1] - video_off[v] for v in range(V)] + [0])
    R = len(sel_video)
    tb, state = np.zeros((R, Fmax, 4), F32), np.zeros((R, Fmax), np.uint8)
    tod = res["track_of_det"]
    for r in range(R):
        v, k = int(sel_video[r]), int(sel_track[r])
        if not (0 <= v < V and 0 <= k < res["first"].shape[1]):
            continue
        f0, Fv = video_off[v], video_off[v + 1] - video_off[v]
        first, last = int(res["first"][v, k]), int(res["last"][v, k])
        hit = {}
        for t in range(Fv):
            d = np.nonzero(tod[f0 + t] == k)[0]
            if len(d):
                hit[t] = boxes[f0 + t, int(d[-1])]
        for t in range(max(first, 0), min(last, Fv - 1) + 1):
            if t in hit:
                tb[r, t], state[r, t] = hit[t], DETECTED
                continue
            ta = max([u for u in hit if u < t and u >= first], default=None)
            tbn = min([u for u in hit if u > t and u <= last], default=None)
            if ta is None or tbn is None:
                continue
            a, b = hit[ta], hit[tbn]
            with np.errstate(all="ignore"):
                w = F32(t - ta) / F32(tbn - ta)
                tb[r, t] = (a + ((b - a).astype(F32) * w).astype(F32)).astype(F32)
            state[r, t] = INTERPOLATED
    return tb, state


def segment_tracklets(res, tb, sel_video, sel_track, video, fstart, fend, max_tracklets=64):
    """The segment cut: of the selected rows of `video` those that span [fstart, fend), the best max_tracklets by score
    descending then id ascending.  Returns (boxes [n, fend - fstart, 4], ids, classes, scores)."""
    rows = [r for r in range(len(sel_video)) if int(sel_video[r]) == video
            and res["first"][video, sel_track[r]] <= fstart and res["last"][video, sel_track[r]] >= fend - 1]
    rows.sort(key=lambda r: (-float(res["score"][video, sel_track[r]]), int(sel_track[r])))
    rows = rows[:max_tracklets]
    ids = np.asarray([sel_track[r] for r in rows], np.int64)
    return (tb[rows, fstart:fend].reshape(len(rows), fend - fstart, 4), ids, res["cls"][video, ids].astype(np.int64),
            res["score"][video, ids].astype(F32))


def segments_of(num_frames, seg_len=30, stride=15):
    """[(fstart, fend)] of the full segments of a video."""
    return [(s, s + seg_len) for s in range(0, num_frames - seg_len + 1, stride)]


# ---------------------------------------------------------------------------------------------------------- scenes
def pack(frames, D, dtype=F32):
    """Per-frame lists of (x1, y1, x2, y2, score, class) -> (boxes [F, D, 4], scores [F, D], classes [F, D], count [F])."""
    F = len(frames)
    boxes, scores = np.zeros((F, D, 4), F32), np.zeros((F, D), F32)
    classes, count = np.zeros((F, D), np.int64), np.zeros(F, np.int64)
    for f, rows in enumerate(frames):
        assert len(rows) <= D
        count[f] = len(rows)
        for d, r in enumerate(rows):
            boxes[f, d], scores[f, d], classes[f, d] = r[:4], r[4], r[5]
    return boxes, scores, classes, count


def constant_velocity_scene():
    """Two 80 x 80 objects moving +30 and -30 px a frame for 40 frames; the first is missing at frames 10, 11 and 25."""
    frames = []
    for t in range(40):
        rows = []
        if t not in (10, 11, 25):
            rows.append((100 + 30 * t, 100, 180 + 30 * t, 180, 0.9, 1))
        rows.append((1400 - 30 * t, 300, 1480 - 30 * t, 380, 0.8, 2))
        frames.append(rows)
    return pack(frames, 4)


def generated_scene(seed, num_objects=6, num_frames=120, dropout=0.1, false_positives=3, D=16):
    """Objects on smooth paths with jitter, `dropout` of their detections missing, and low-score false positives at random
    places.  Returns (boxes, scores, classes, count, owner int [F, D]: the object of a detection, -1 for a false positive).
    Objects keep to lanes 150 px apart, so that no two of them overlap."""
    rng = np.random.RandomState(seed)
    frames, owners = [], []
    x0 = rng.uniform(100, 400, num_objects)
    vx = rng.uniform(-6, 6, num_objects)
    size = rng.uniform(60, 100, num_objects)
    for t in range(num_frames):
        rows, own = [], []
        for o in range(num_objects):
            if rng.uniform() < dropout and 0 < t < num_frames - 1:
                continue
            cx = x0[o] + vx[o] * t + rng.uniform(-2, 2)
            cy = 100 + 150 * o + rng.uniform(-2, 2)
            s = size[o] + rng.uniform(-2, 2)
            rows.append((cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2, rng.uniform(0.7, 1.0), 1 + o % 3))
            own.append(o)
        for _ in range(false_positives):
            cx, cy, s = rng.uniform(0, 2000), rng.uniform(0, 1000), rng.uniform(20, 120)
            rows.append((cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2, rng.uniform(0.05, 0.3), int(rng.randint(1, 4))))
            own.append(-1)
        order = rng.permutation(len(rows))
        frames.append([rows[i] for i in order])
        owners.append([own[i] for i in order])
    boxes, scores, classes, count = pack(frames, D)
    owner = np.full((num_frames, D), -1, np.int64)
    for f, own in enumerate(owners):
        owner[f, :len(own)] = own
    return boxes, scores, classes, count, owner


def chain_frame(links=7, width=100.0, first_step=50.0, shrink=2.0):
    """Two frames on which the mutual-best match needs ceil(links / 2) rounds: boxes in a row, alternately a track (frame 0)
    and a detection (frame 1), each overlapping the next more than the one before."""
    xs, x, step = [], 0.0, first_step
    for _ in range(links + 1):
        xs.append(x)
        x += step
        step -= shrink
    tracks = [(x, 0, x + width, 10, 0.9, 1) for x in xs[0::2]]
    dets = [(x, 0, x + width, 10, 0.9, 1) for x in xs[1::2]]
    return pack([tracks, dets], max(len(tracks), len(dets)))
