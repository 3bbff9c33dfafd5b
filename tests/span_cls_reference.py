"""Training the predicate head on ground-truth-span-pooled features (DESIGN.md §2 "span-pooled predicate training"): a plain
numpy / float64 restatement of the per-span predicate labels (in the statement order of tests/pair_labels_reference.py:
instance by instance, a later instance overwriting under merge "last") and of the loss of the span-pooled head with its
gradients dv, db, dG, dW, and the operands the host and GPU tests share.

Rows: r = p G + g; with c = span_count[p]: c >= 1 and g < min(c, G) is a row over spans[p, g]; c == 0 and g == 0 a negative
pair over [0, T) with a zero label; anything else is no row, and so is every row of a pair naming a tracklet outside
[0, NT).

Granularities of the kernels (csrc/spancls/tspn_span_cls.hip; tests/spancls_kernel_variants.py): the label kernel takes
TILE = 256 rows (p, g) per workgroup with ceil(K / 64) mask words per row (the pair-label cases already sit around one
tile and one word; P G of 1, 255, 256, 257, 1020, 4 * 515); the loss kernel takes one wave per row, four rows per
workgroup, lanes 64 apart over K (K of 1, 5, 145: below one wave, and two full passes and a ragged third); the finish
kernel and the row count take 256 threads per segment; the bias gradient 256 predicates per workgroup; the projection
gradient one thread per (tracklet, column), 256 per workgroup (NT 2K of 10 .. 1450)."""
from itertools import product

import numpy as np

import pair_labels_reference as plr

TILE, WAVES, MAX_K, MAX_G = 256, 4, 512, 16


# ------------------------------------------------------------------------------------------------- the labels
def span_labels_segment(seg, K, G, thr, merge, spans, span_count):
    """span_labels fp32 [P,G,K] of one segment (the dict of pair_labels_reference.segment_ref) given the spans int64
    [P,G,2] and span_count int32 [P] that restatement returns."""
    trackid, iou, pairs, insts = seg["trackid"], seg["iou"], seg["pairs"], seg["insts"]
    fstart, fend = seg["frames"]
    P = len(pairs)
    thr32 = np.float32(thr)
    pair_to_finds = {}
    for find, (t1, t2) in enumerate(pairs):
        pair_to_finds.setdefault((int(t1), int(t2)), []).append(find)
    gt_tid_to_idx = dict([(int(tid), ind) for ind, tid in enumerate(trackid) if tid >= 0])
    out = np.zeros((P, G, K), np.float32)
    for sub_tid, obj_tid, pred_idx, begin, end in insts.tolist():
        if not 0 <= pred_idx < K or sub_tid not in gt_tid_to_idx or obj_tid not in gt_tid_to_idx:
            continue
        overlap_tids1 = np.where(iou[:, gt_tid_to_idx[sub_tid]] >= thr32)[0]
        overlap_tids2 = np.where(iou[:, gt_tid_to_idx[obj_tid]] >= thr32)[0]
        span = (max(begin, fstart) - fstart, min(end, fend) - fstart)
        for traj_idx1, traj_idx2 in product(overlap_tids1.tolist(), overlap_tids2.tolist()):
            if traj_idx1 != traj_idx2 and trackid[traj_idx1] < 0 and trackid[traj_idx2] < 0:
                for find in pair_to_finds.get((traj_idx1, traj_idx2), ()):
                    for g in range(min(int(span_count[find]), G)):
                        if tuple(spans[find, g].tolist()) == span:
                            if merge == "last":
                                out[find, g] = 0.0
                            out[find, g, pred_idx] = 1.0
    return out


def case_span_labels(case):
    """(labels, spans, span_count, inst_cols, span_labels) of a pair-label case with G > 0, its segments back to back."""
    K, G = case["K"], case["G"]
    parts = []
    for seg in case["segments"]:
        lab, spans, count, cols = plr.segment_ref(seg, K, G, case["thr"], case["merge"])
        parts.append((lab, spans, count, cols, span_labels_segment(seg, K, G, case["thr"], case["merge"], spans, count)))
    empty = (np.zeros((0, K), np.float32), np.zeros((0, G, 2), np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.int32),
             np.zeros((0, G, K), np.float32))
    return tuple(np.concatenate([p[i] for p in parts] + [empty[i]]) for i in range(5))


def label_cases():
    """The pair-label cases that have span rows, and one at the K limit (the pair-label case of K = 512 has G = 0)."""
    out = [c for c in plr.cases() if c["G"] > 0]
    seg = plr.make_segment(612, 22, plr.GT4, 257, 70, 512, 0.5, dense=True)
    out += [{"id": f"K512-G4-{m}", "K": 512, "G": 4, "thr": 0.5, "merge": m, "segments": [seg], "single": True} for m in ("last", "or")]
    return out


# ------------------------------------------------------------------------------------------------- the loss
def row_table(pairs, spans, span_count, NT, T, G):
    """(valid bool [P,G], a int64 [P,G], e int64 [P,G]): the rows and their frames, through the row rewrite of span pooling
    (oracle.span_frames: 0 <= a < e <= T)."""
    P = len(pairs)
    valid = np.zeros((P, G), bool)
    a, e = np.zeros((P, G), np.int64), np.ones((P, G), np.int64)
    for p in range(P):
        c = int(span_count[p])
        if not (0 <= pairs[p, 0] < NT and 0 <= pairs[p, 1] < NT):
            continue
        rows = min(c, G) if c >= 1 else (1 if c == 0 else 0)
        for g in range(rows):
            a0, e0 = (0, T) if c == 0 else (int(spans[p, g, 0]), int(spans[p, g, 1]))
            lo = 0 if a0 < 0 else min(a0, T - 1)
            hi = (T if a0 < 0 else lo + 1) if e0 < lo + 1 else min(e0, T)
            valid[p, g], a[p, g], e[p, g] = True, lo, hi
    return valid, a, e


def loss_ref(feats, pairs, spans, span_count, span_labels, cls_w, cls_b, pair_off=None):
    """The float64 restatement: dict of loss (the sum over the segments), seg_loss [S], seg_rows [S], valid [P G], v, q,
    dv [P G, K], db [K], dG [NT,T,2K], dW [K,2D]."""
    f = feats.astype(np.float64)
    NT, T, D = f.shape
    P, G = spans.shape[:2]
    K = cls_w.shape[0]
    w = cls_w.astype(np.float64)
    off = np.array([0, P], np.int64) if pair_off is None else np.asarray(pair_off, np.int64)
    S = len(off) - 1
    valid, a, e = row_table(pairs, spans, span_count, NT, T, G)
    v = np.zeros((P, G, K))
    y = np.zeros((P, G, K))
    for p, g in zip(*np.nonzero(valid)):
        s, o = pairs[p]
        x = np.concatenate([f[s, a[p, g]:e[p, g]].sum(0), f[o, a[p, g]:e[p, g]].sum(0)]) / float(e[p, g] - a[p, g])
        v[p, g] = w @ x + (0.0 if cls_b is None else cls_b.astype(np.float64))
        if span_count[p] >= 1:
            y[p, g] = span_labels[p, g]
    with np.errstate(over="ignore", invalid="ignore"):
        el = np.maximum(v, 0.0) - v * y + np.log1p(np.exp(-np.abs(v)))
        el = np.where(np.isnan(v), np.nan, el)                  # np.maximum(nan, 0) is nan already; stated for the reader
        sg = 1.0 / (1.0 + np.exp(-v))
    seg_rows = np.array([valid[off[s]:off[s + 1]].sum() for s in range(S)], np.float64)
    seg_loss, dv = np.zeros(S), np.zeros((P, G, K))
    for s in range(S):
        m = valid[off[s]:off[s + 1]]
        if seg_rows[s] > 0:
            seg_loss[s] = el[off[s]:off[s + 1]][m].sum() / (K * seg_rows[s])
            dv[off[s]:off[s + 1]][m] = ((sg - y)[off[s]:off[s + 1]][m]) / (K * seg_rows[s])
    dG = np.zeros((NT, T, 2 * K))
    for p, g in zip(*np.nonzero(valid)):
        for h in range(2):
            dG[pairs[p, h], a[p, g]:e[p, g], h::2] += dv[p, g] / float(e[p, g] - a[p, g])
    with np.errstate(invalid="ignore"):
        dW2 = np.einsum("ntj,ntc->jc", dG, f)                   # [2K, D]: row 2k + h is half h of row k
    return {"loss": seg_loss.sum(), "seg_loss": seg_loss, "seg_rows": seg_rows, "valid": valid.reshape(-1),
            "v": v.reshape(P * G, K), "q": np.where(valid[..., None], sg, 0.0).reshape(P * G, K).astype(np.float32),
            "dv": dv.reshape(P * G, K), "db": dv.reshape(P * G, K).sum(0), "dG": dG, "dW": dW2.reshape(K, 2 * D)}


def loss_case(seed, N, S, T, D, K, G, table="canonical", P=None):
    """Operands of one loss case: S segments of N tracklets (ids global), a pair table per segment -- "canonical": all
    ordered pairs; "shuffled": those shuffled, with a duplicated row, a pair naming a tracklet outside [0, NT) and
    tracklet N - 1 of the last segment named by no row -- or P random rows per segment; spans of length 1, of length T, two
    adjacent spans [a, m), [m, f) of one pair where G >= 2; span counts of -1, 0, G and G + 1 among the pairs."""
    rs = np.random.RandomState(seed)
    NT = S * N
    feats = rs.uniform(-1.0, 1.0, (NT, T, D)).astype(np.float32)
    cls_w = (rs.randn(K, 2 * D) / np.sqrt(2 * D)).astype(np.float32)
    cls_b = (0.1 * rs.randn(K)).astype(np.float32)
    tables = []
    for s in range(S):
        full = np.array([(i, j) for i in range(N) for j in range(N) if i != j], np.int64).reshape(-1, 2)
        if P is not None:
            full = np.stack([rs.randint(0, N, P), rs.randint(0, N, P)], 1).astype(np.int64)
        elif table == "shuffled":
            full = full[rs.permutation(len(full))]
            if s == S - 1:
                full = full[(full != N - 1).all(1)]
            full = np.concatenate([full, full[:1]])
        tables.append(full + s * N)
    pairs = np.concatenate(tables)
    pair_off = np.concatenate([[0], np.cumsum([len(x) for x in tables])]).astype(np.int64)
    Pn = len(pairs)
    if table == "shuffled" and Pn > 3:
        pairs[2] = (NT + 3, 0)                                     # no rows: nothing is read through it
    span_count = rs.choice([0, 1, G, G + 1], Pn).astype(np.int32)
    if Pn > 4:
        span_count[3] = -1
    spans = np.zeros((Pn, G, 2), np.int64)
    for p in range(Pn):
        for g in range(min(max(int(span_count[p]), 0), G)):
            a = rs.randint(0, T)
            spans[p, g] = (a, rs.randint(a + 1, T + 1))
    if Pn > 0:
        span_count[0], spans[0, 0] = max(1, min(G, 2)), (T - 1, T)               # length 1
        if G >= 2 and T >= 2:
            m = T // 2
            spans[0, 0], spans[0, 1] = (0, m), (m, T)               # two adjacent spans of one pair
    if Pn > 1:
        span_count[1], spans[1, 0] = 1, (0, T)                      # the whole segment
    if Pn > 5:
        span_count[5], spans[5, 0] = 1, (0, 1)                      # length 1
    span_labels = (rs.uniform(size=(Pn, G, K)) < 0.1).astype(np.float32)
    return {"feats": feats, "pairs": pairs, "pair_off": pair_off if S > 1 else None, "spans": spans, "span_count": span_count,
            "span_labels": span_labels, "cls_w": cls_w, "cls_b": cls_b, "dims": (NT, T, D, K, G, S)}
