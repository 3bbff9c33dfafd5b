"""Per-frame detections -> tracklets ("tracklet linking"): the stage between FasterRCNNC4 and everything
that takes dense [N, T, 4] tracklet boxes per segment (Res5RoIHead, the scorer, the association, the evaluators).

A deterministic IoU tracker with constant-velocity prediction, on the device (csrc/link/tspn_link.hip): the link pass
gives every detection its track, the fill pass gives the selected tracks dense boxes over their video, and the segment
cut is torch indexing on those.  Build-defined; there is no Kalman filter, no assignment solver and no appearance metric.
"""
from collections import namedtuple

import torch

from . import ops

__all__ = ["Tracks", "link_detections", "segment_tracklets", "video_tracklets"]

ABSENT, DETECTED, INTERPOLATED = 0, 1, 2

Tracks = namedtuple("Tracks", [
    "video_off",        # host list [V + 1] of frame offsets
    "track_of_det",     # int32 [F, D]: the video-local track id of a detection, -1: none
    "n_tracks",         # int64 [V]: ids used per video
    "dropped",          # int64 [V]: candidates that could not start a track (max_live / max_tracks)
    "first", "last", "hits",   # int32 [V, max_tracks]: first and last detected frame (video-local), detections
    "cls",              # int64 [V, max_tracks]: the class of the detection that started the track
    "score",            # fp32 [V, max_tracks]: mean detection score
    "sel_video", "sel_track",  # int64 [R]: the selected tracks, the rows of track_boxes
    "track_boxes",      # fp32 [R, Fmax, 4]
    "state",            # uint8 [R, Fmax]: ABSENT, DETECTED, INTERPOLATED
])


def link_detections(detections, video_off=None, select=None, iou_thresh=0.3, max_age=30, min_hits=3, min_score=0.0,
                    class_aware=True, max_live=1024, max_tracks=16384):
    """detections = (boxes [F,D,4], scores [F,D], classes int64 [F,D], count int64 [F]) as FasterRCNNC4.forward returns
    them; video_off: V + 1 host frame offsets (None: one video).  `select`: (sel_video, sel_track) int64 [R] device tensors
    of the tracks to fill (None: the confirmed ones, hits >= min_hits, by video and ascending id -- their number is read
    back from the device).  Returns a Tracks."""
    boxes, scores, classes, count = detections
    F = boxes.shape[0]
    off = [0, F] if video_off is None else [int(v) for v in (video_off.tolist() if isinstance(video_off, torch.Tensor)
                                                              else video_off)]
    tod, n_tracks, dropped, first, last, hits, cls, score = ops.link_detections(
        boxes, scores, classes, count, off, iou_thresh, max_age, min_hits, min_score, class_aware, max_live, max_tracks)
    if select is None:
        at = torch.nonzero(hits >= int(min_hits))            # [R, 2], by video then id
        sel_video, sel_track = at[:, 0].contiguous(), at[:, 1].contiguous()
    else:
        sel_video, sel_track = select
    track_boxes, state = ops.link_fill(boxes, tod, first, last, sel_video, sel_track, off)
    return Tracks(off, tod, n_tracks, dropped, first, last, hits, cls, score, sel_video, sel_track, track_boxes, state)


def segment_tracklets(tracks, video, fstart, fend, max_tracklets=64):
    """The selected tracks of `video` that span the segment (first <= fstart and last >= fend - 1), the best max_tracklets
    of them by score descending then id ascending.  Returns (boxes fp32 [n, fend - fstart, 4], ids int64 [n], classes
    int64 [n], scores fp32 [n]): the form Res5RoIHead, tracklets_to_traj_cls and pair_list take."""
    video, fstart, fend = int(video), int(fstart), int(fend)
    V = len(tracks.video_off) - 1
    if not 0 <= video < V:
        raise ValueError(f"segment_tracklets: video {video} outside [0, {V})")
    fv = tracks.video_off[video + 1] - tracks.video_off[video]
    if not 0 <= fstart < fend <= fv:
        raise ValueError(f"segment_tracklets: segment [{fstart}, {fend}) outside the video's {fv} frames")
    ids = tracks.sel_track
    known = (tracks.sel_video == video) & (ids >= 0) & (ids < tracks.first.shape[1])
    at = ids.clamp(0, tracks.first.shape[1] - 1)
    keep = known & (tracks.first[video][at] <= fstart) & (tracks.last[video][at] >= fend - 1)
    rows = torch.nonzero(keep)[:, 0]
    rows = rows[torch.sort(ids[rows], stable=True)[1]]                                  # id ascending ...
    rows = rows[torch.sort(tracks.score[video][ids[rows]], descending=True, stable=True)[1]]   # ... under score descending
    rows = rows[:int(max_tracklets)]
    ids = ids[rows]
    return (tracks.track_boxes[rows, fstart:fend].contiguous(), ids, tracks.cls[video][ids], tracks.score[video][ids])


def video_tracklets(detections, seg_len=30, stride=15, max_tracklets=64, video_off=None, **link):
    """Link the detections and cut every full segment [s, s + seg_len), s = 0, stride, ..., of every video.  Returns
    (tracks, segments): segments is a list of dicts video, fstart, fend, boxes, ids, classes, scores in video and time
    order."""
    tracks = link_detections(detections, video_off, **link)
    out = []
    for v in range(len(tracks.video_off) - 1):
        fv = tracks.video_off[v + 1] - tracks.video_off[v]
        for s in range(0, fv - int(seg_len) + 1, int(stride)):
            boxes, ids, classes, scores = segment_tracklets(tracks, v, s, s + int(seg_len), max_tracklets)
            out.append({"video": v, "fstart": s, "fend": s + int(seg_len), "boxes": boxes, "ids": ids, "classes": classes,
                        "scores": scores})
    return tracks, out
