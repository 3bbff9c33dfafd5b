"""Pair labels from ground-truth relation instances (DESIGN.md §2 "pair labels"): a plain numpy / Python restatement in the
statement order of the reference's `VRDataset._get_proposals_rel_feature` (lib/dataset/vrdataset.py:85-138) -- the
`gt_tid_to_idx` dict (the last occurrence of an id wins), `product(overlap_tids1, overlap_tids2)`, and a dict assignment per
covered pair that a later instance overwrites (merge "last") -- and the case list the host and GPU tests share.

What the restatement adds to the reference's statements is what the build froze: rows in pair order (not in dict insertion
order), the float32 threshold, `merge="or"`, pair tables that repeat or leave out pairs, the spans, and `inst_cols`.

Granularities of the kernels (csrc/pairlabels/tspn_pair_labels.hip; tests/pairlabels_kernel_variants.py): TILE = 256 pairs per
workgroup, one thread per pair, so P of 1, 255, 256, 257 sit around one tile and 2 * 256 + 3 = 515 has three workgroups with
a ragged last one; a pair's predicate mask is ceil(K / 64) 64-bit words, so K of 1, 63, 64, 65 sit around one word, 132 is
three words with a ragged last one and 512 is the limit (8 words); the label store takes 16-byte pieces of the tile's
rows * K elements, so K = 1, 63, 65 with a ragged tile leave a scalar tail; 256 instances per workgroup of the resolve kernel
(R of 0, 1, 70); G of 1, 4, 16 span rows, 16 the limit; S of 1 (null offsets) and 3 (binary search over the offsets, with an
empty segment and a segment without instances)."""
import functools
from itertools import product

import numpy as np

TILE = 256
MAX_K, MAX_G = 512, 16
SEG_LEN = 30


def f32_next(x, up):
    return np.nextafter(np.float32(x), np.float32(2.0 if up else -1.0), dtype=np.float32)


# ------------------------------------------------------------------------------------------------- the restatement
def segment_ref(seg, K, G, thr, merge):
    """(labels fp32 [P,K], spans int64 [P,G,2], span_count int32 [P], inst_cols int32 [R,2]) of one segment: a dict with
    trackid int64 [M], iou fp32 [M,M], pairs int64 [P,2], insts int64 [R,5], frames (fstart, fend)."""
    trackid, iou, pairs, insts = seg["trackid"], seg["iou"], seg["pairs"], seg["insts"]
    fstart, fend = seg["frames"]
    M, P = len(trackid), len(pairs)
    thr32 = np.float32(thr)
    assert iou.dtype == np.float32 and iou.shape == (M, M)
    pair_to_finds = {}                               # the reference's pair_to_find, for a table that may repeat a pair
    for find, (t1, t2) in enumerate(pairs):
        pair_to_finds.setdefault((int(t1), int(t2)), []).append(find)
    gt_tid_to_idx = dict([(int(tid), ind) for ind, tid in enumerate(trackid) if tid >= 0])
    pred_labels = {}
    found = {find: [] for find in range(P)}          # the distinct spans of a pair, in the order they were met
    inst_cols = np.full((len(insts), 2), -1, np.int32)
    for r, (sub_tid, obj_tid, pred_idx, begin, end) in enumerate(insts.tolist()):
        if not 0 <= pred_idx < K:
            inst_cols[r] = -2
            continue
        inst_cols[r] = (gt_tid_to_idx.get(sub_tid, -1), gt_tid_to_idx.get(obj_tid, -1))
        if sub_tid in gt_tid_to_idx and obj_tid in gt_tid_to_idx:
            iou1 = iou[:, gt_tid_to_idx[sub_tid]]
            iou2 = iou[:, gt_tid_to_idx[obj_tid]]
            overlap_tids1 = np.where(iou1 >= thr32)[0]
            overlap_tids2 = np.where(iou2 >= thr32)[0]
            onehot = np.zeros(K, np.float32)
            onehot[pred_idx] = 1.0
            span = (max(begin, fstart) - fstart, min(end, fend) - fstart)
            for traj_idx1, traj_idx2 in product(overlap_tids1.tolist(), overlap_tids2.tolist()):
                if traj_idx1 != traj_idx2 and trackid[traj_idx1] < 0 and trackid[traj_idx2] < 0:
                    for find in pair_to_finds.get((traj_idx1, traj_idx2), ()):
                        if merge == "last":
                            pred_labels[find] = onehot
                        else:
                            pred_labels[find] = np.maximum(pred_labels.get(find, 0.0), onehot)
                        if span[1] > span[0] and span not in found[find]:
                            found[find].append(span)
    labels = np.zeros((P, K), np.float32)
    for find, row in pred_labels.items():
        labels[find] = row
    spans = np.zeros((P, G, 2), np.int64)
    span_count = np.zeros(P, np.int32)
    for find in range(P):
        a, b = pairs[find]
        if not (0 <= a < M and 0 <= b < M):
            span_count[find] = -1
            continue
        for g, span in enumerate(found[find][:G]):
            spans[find, g] = span
        span_count[find] = min(len(found[find]), G + 1)
    if G == 0:
        span_count[:] = 0
    return labels, spans, span_count, inst_cols


def case_ref(case):
    """The four outputs of a case, its segments back to back."""
    parts = [segment_ref(s, case["K"], case["G"], case["thr"], case["merge"]) for s in case["segments"]]
    K, G = case["K"], case["G"]
    empty = (np.zeros((0, K), np.float32), np.zeros((0, G, 2), np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    return tuple(np.concatenate([p[i] for p in parts] + [empty[i]]) for i in range(4))


def batch_of(case):
    """The concatenated operands of a case as the entry takes them: a dict of numpy arrays."""
    segs = case["segments"]
    cat = lambda key, empty: np.concatenate([s[key].reshape((-1,) + empty.shape[1:]) for s in segs] + [empty])  # noqa: E731
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)  # noqa: E731
    return {"pairs": cat("pairs", np.zeros((0, 2), np.int64)), "trackid": cat("trackid", np.zeros(0, np.int64)),
            "iou": cat("iou", np.zeros(0, np.float32)), "insts": cat("insts", np.zeros((0, 5), np.int64)),
            "seg_frames": np.array([s["frames"] for s in segs], np.int64).reshape(-1, 2),
            "pair_off": off([len(s["pairs"]) for s in segs]), "track_off": off([len(s["trackid"]) for s in segs]),
            "iou_off": off([len(s["trackid"]) ** 2 for s in segs]), "inst_off": off([len(s["insts"]) for s in segs])}


# ------------------------------------------------------------------------------------------------------ the inputs
ABSENT_TID = 77                                      # a ground-truth id no trackid holds


def make_segment(seed, n_prop, gt_ids, P, R, K, thr, layout="tail", dense=False, fstart=45):
    """A segment of n_prop proposals and the ground-truth tracks `gt_ids` (an id may repeat: the last column wins).
    layout "tail": proposals first (the layout of the h5 files); "mixed": ground truth among the proposals.
    The pair table: first the pairs that must not be labelled (s == o, a ground-truth track on either side, an index
    outside [0, M) on either side, where P leaves room), then a repeated pair, then the ordered pairs in a shuffled order.
    iou: uniform, `dense`: every proposal overlaps every ground-truth column (every live instance covers every proposal
    pair); the rows of proposals 0 .. 3 hold, in the column of the first ground-truth id, float32(thr), one ulp below, one
    ulp above and NaN, and 0.9 in the other ground-truth columns.
    The instances: ids drawn from the ground-truth ids, ABSENT_TID and negative ids, sometimes sub == obj; pred mostly in
    [0, K), sometimes -1 or K; durations from a pool that holds spans clipped at the start, at the end, at both, empty
    after clipping, inside, and (dense) more distinct spans than the largest G."""
    rs = np.random.RandomState(seed)
    gt_ids = list(gt_ids)
    M = n_prop + len(gt_ids)
    trackid = np.full(M, -1, np.int64)
    gt_pos = np.arange(n_prop, M) if layout == "tail" else np.sort(rs.choice(M, len(gt_ids), replace=False))
    trackid[gt_pos] = gt_ids
    props = np.flatnonzero(trackid < 0)
    iou = rs.uniform(0.0, 1.0, (M, M)).astype(np.float32)
    if dense:
        iou[np.ix_(props, gt_pos)] = 0.9
    if len(gt_ids) and n_prop >= 4:
        col0 = int(np.flatnonzero(trackid == gt_ids[0])[-1])
        iou[np.ix_(props[:4], gt_pos)] = 0.9
        iou[props[:4], col0] = [np.float32(thr), f32_next(thr, False), f32_next(thr, True), np.float32("nan")]
    fend = fstart + SEG_LEN
    # the pair table
    special = []
    if M:
        special += [(props[0] if len(props) else 0,) * 2]
        if len(gt_pos) and len(props):
            special += [(gt_pos[0], props[0]), (props[0], gt_pos[-1])]
        special += [(-1, 0), (0, M), (M + 5, -3)]
    full = np.array([(a, b) for a in range(M) for b in range(M) if a != b], np.int64).reshape(-1, 2)
    full = full[rs.permutation(len(full))]
    rows = [tuple(int(v) for v in x) for x in special] + ([tuple(full[0])] if len(full) else []) + [tuple(x) for x in full.tolist()]
    if P <= 6:                                               # a table too short for the special rows: ordinary pairs
        rows = [tuple(x) for x in full.tolist()]
    assert len(rows) >= P, (len(rows), P)
    pairs = np.array(rows[:P], np.int64).reshape(-1, 2)
    # the instances
    pool = [(fstart - 10, fstart + 12), (fstart + 20, fend + 9), (fstart - 3, fend + 3), (fstart - 20, fstart),
            (fend, fend + 7), (fstart + 5, fstart + 5), (fstart + 4, fstart + 11), (fstart + 4, fstart + 11),
            (fstart, fend), (fstart - 1, fend)]
    if dense:
        pool += [(fstart + a, fstart + a + 3) for a in range(0, 2 * (MAX_G + 2), 2)][:MAX_G + 2]
    ids = gt_ids + [ABSENT_TID, -1, -5] if gt_ids else [ABSENT_TID, -1]
    weights = np.array([6.0] * len(gt_ids) + [1.0] * (len(ids) - len(gt_ids)))
    insts = np.zeros((R, 5), np.int64)
    for r in range(R):
        sub, obj = rs.choice(ids, 2, p=weights / weights.sum())
        u = rs.uniform()
        pred = -1 if u < 0.04 else K if u < 0.08 else K - 1 if u < 0.2 else int(rs.randint(0, K))
        insts[r] = (sub, obj, pred) + pool[r % len(pool) if dense else rs.randint(len(pool))]
    return {"trackid": trackid, "iou": iou, "pairs": pairs, "insts": insts, "frames": (fstart, fend)}


def _case(cid, K, G, thr, segments):
    return [{"id": f"{cid}-{merge}", "K": K, "G": G, "thr": thr, "merge": merge, "segments": segments, "single": len(segments) == 1}
            for merge in ("last", "or")]


GT4 = (0, 1, 2, 1)                                   # id 1 twice: its last column wins


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for P in (1, 255, 256, 257, 2 * TILE + 3):               # around one tile, three workgroups
        out += _case(f"P{P}", 132, 4, 0.5, [make_segment(P, 22, GT4, P, 70, 132, 0.5)])
    for K in (1, 63, 64, 65, 512):                           # around one mask word, the limit
        out += _case(f"K{K}", K, 0 if K in (63, 512) else 4, 0.7, [make_segment(100 + K, 22, GT4, 257, 70, K, 0.7, layout="mixed")])
    for R in (0, 1):
        out += _case(f"R{R}", 132, 4, 0.5, [make_segment(200 + R, 22, GT4, 257, R, 132, 0.5)])
    for G in (1, 4, 16):                                     # every proposal pair overflows G
        out += _case(f"G{G}-dense", 65, G, 0.5, [make_segment(300 + G, 12, GT4, 140, 70, 65, 0.5, dense=True)])
    out += _case("no-gt", 132, 4, 0.5, [make_segment(400, 8, (), 56, 5, 132, 0.5)])
    three = [make_segment(500, 22, GT4, 300, 20, 132, 0.7, fstart=0),
             make_segment(501, 6, (3,), 0, 4, 132, 0.7, fstart=15),                   # no pairs
             make_segment(502, 14, (5, 9), 100, 0, 132, 0.7, layout="mixed", fstart=30)]  # no instances
    out += _case("S3", 132, 4, 0.7, three)
    out += _case("S3-empty-ends", 64, 16, 0.5, [make_segment(510, 0, (), 0, 0, 64, 0.5, fstart=0),
                                                 make_segment(511, 12, GT4, 140, 70, 64, 0.5, dense=True, fstart=15),
                                                 make_segment(512, 0, (), 0, 0, 64, 0.5, fstart=30)])
    out += _case("S1-offsets", 132, 4, 0.5, [make_segment(520, 22, GT4, 257, 70, 132, 0.5)])
    out[-1]["single"] = out[-2]["single"] = False            # one segment through the offset form
    return out


def case_ids():
    return [c["id"] for c in cases()]


SMALL_IDS = ("P1-last", "P255-or", "K1-last", "K65-or", "R1-last", "G1-dense-last", "G4-dense-or", "no-gt-last", "S3-last")


def edge_segment(thr):
    """Four proposals against one subject column (fp32 thr, one ulp below, one ulp above, NaN) and a fifth, ordinary one;
    one instance (0 -> 1, predicate 5, the whole segment)."""
    seg = make_segment(7, 5, (0, 1), 30, 1, 8, thr)
    seg["insts"][0] = (0, 1, 5, seg["frames"][0], seg["frames"][1])
    seg["pairs"] = np.array([(a, b) for a in range(7) for b in range(7) if a != b][:30], np.int64)
    return seg
