"""Training the predicate head on ground-truth-span-pooled features on the GPU (csrc/spancls/tspn_span_cls.hip:
tspn_span_labels_f32, tspn_span_predicate_loss_f32 / _finish, tspn_span_predicate_grad_f32 and their ops wrappers) against
the numpy restatement (tests/span_cls_reference.py).

Labels: bit-equal on every pair-label case with span rows (P of 1, 255, 256, 257, 515; K of 1, 64, 65, 132, 512; G of 1, 4, 16;
S = 3 with offsets; R = 0; pairs with span_count -1 and saturated at G + 1), sentinel-guarded and off the 16-byte alignment.
Loss and gradients at N = 5, S of 1, 2, T of 1, 2, 33, D of 16, 40, K of 1, 5, 145, G of 1, 3, canonical and shuffled pair
tables (a duplicated row, a tracklet named by no row, a pair outside [0, NT), spans of length 1 and T, two adjacent spans
of one pair), and P G = 15872 rows.  Tolerances are those of tests/test_gpu_training_shapes.py: loss rtol 2e-5, dW / db
atol 2e-4 max|ref| + 1e-9 (dv and dG are held to the same bound); q is bit-equal to ops.span_predicate."""
import functools
import importlib
from itertools import product

import numpy as np
import pytest
import torch

import pair_labels_reference as plr
import sentinel_buffers as sb
import span_cls_reference as ref

pytestmark = pytest.mark.gpu


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------------- the labels
@functools.lru_cache(maxsize=None)
def label_reference(cid):
    case = next(c for c in ref.label_cases() if c["id"] == cid)
    out = ref.case_span_labels(case)
    for a in out:
        a.setflags(write=False)
    return case, out


LABEL_IDS = [c["id"] for c in ref.label_cases()]


def label_operands(device, case, want):
    b = {k: _t(v).to(device) for k, v in plr.batch_of(case).items()}
    b.update(spans=_t(want[1]).to(device), span_count=_t(want[2]).to(device), inst_cols=_t(want[3]).to(device))
    return b


def same_rows(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    bad = np.flatnonzero((g.view(np.int32) != want.view(np.int32)).reshape(len(want), -1).any(axis=1)) if len(want) else []
    assert len(bad) == 0, f"{what}: differs in {len(bad)} rows, first {bad[:5]}"


@pytest.mark.parametrize("cid", LABEL_IDS)
def test_span_labels_equal_the_restatement(tspn, device, cid):
    """The restatement's spans / span_count / inst_cols as inputs; then the device's own (ops.pair_labels) as inputs: the
    same rows, bit for bit."""
    case, want = label_reference(cid)
    b = label_operands(device, case, want)
    offs = () if case["single"] else (b["pair_off"], b["track_off"], b["iou_off"], b["inst_off"])
    M = len(b["trackid"])
    iou = b["iou"].view(M, M) if case["single"] else b["iou"]
    got = tspn.ops.span_labels(b["pairs"], b["trackid"], iou, b["insts"], case["K"], b["spans"], b["span_count"], b["inst_cols"],
                               b["seg_frames"], case["thr"], case["merge"], *offs)
    same_rows(got, want[4], cid)
    dev = tspn.ops.pair_labels(b["pairs"], b["trackid"], iou, b["insts"], case["K"], case["thr"], case["merge"], case["G"],
                               b["seg_frames"], *offs)
    again = tspn.ops.span_labels(b["pairs"], b["trackid"], iou, b["insts"], case["K"], dev[1], dev[2], dev[3], b["seg_frames"],
                                 case["thr"], case["merge"], *offs)
    assert torch.equal(got, again)
    if cid.startswith(("G4-dense", "P257")):
        count = want[2]
        assert (count == case["G"] + 1).any() if cid.startswith("G4") else (count == -1).any()


@pytest.mark.parametrize("cid,offset", [("P257-or", 0), ("P257-last", 1), ("K65-or", 3), ("K1-last", 2), ("G16-dense-or", 1),
                                        ("S3-last", 1), ("K512-G4-or", 0), ("R0-or", 2)])
def test_span_labels_sentinels_and_unaligned_output(tspn, device, cid, offset):
    """The output held between guard bands, `offset` elements off its alignment (off 16 bytes takes the scalar stores) and
    filled with a sentinel: every element written exactly inside, the result unchanged."""
    case, want = label_reference(cid)
    b = label_operands(device, case, want)
    P, K, G = len(want[0]), case["K"], case["G"]
    buf, out = sb.held((P, G, K), device, offset=offset)
    rc = tspn._abi.lib().tspn_span_labels_f32(
        sb.p(b["pairs"]), sb.p(b["pair_off"]), sb.p(b["trackid"]), sb.p(b["track_off"]), sb.p(b["iou"]), sb.p(b["iou_off"]),
        sb.p(b["insts"]), sb.p(b["inst_off"]), sb.p(b["seg_frames"]), len(case["segments"]), P, len(b["trackid"]),
        len(b["insts"]), K, G, case["thr"], tspn.ops.PAIR_LABEL_MERGES[case["merge"]], sb.p(b["spans"]), sb.p(b["span_count"]),
        sb.p(b["inst_cols"]), sb.p(out), tspn.ops._stream())
    torch.cuda.synchronize(device)
    assert rc == 0, tspn._abi.lib().tspn_last_error()
    sb.assert_written_inside_only(buf, out, cid)
    same_rows(out, want[4], cid)


# ------------------------------------------------------------------------------------------------------- the loss
def model_module(tspn):
    return importlib.import_module(tspn.BaseModel.__module__)


def upload(device, c):
    return {k: (None if v is None else _t(v).to(device)) for k, v in c.items() if k != "dims"}


def run_ops(tspn, device, c):
    d = upload(device, c)
    NT, T = c["dims"][:2]
    out, q, dv, seg_rows, scratch = tspn.ops.span_predicate_loss(d["feats"], d["pairs"], d["spans"], d["span_count"],
                                                                 d["span_labels"], d["cls_w"], d["cls_b"], pair_off=d["pair_off"])
    db, dG = tspn.ops.span_predicate_grad(dv, d["pairs"], d["spans"], d["span_count"], NT, T, scratch=scratch)
    dW = model_module(tspn)._span_cls_weight_grad(dG, d["feats"])
    return d, {"out": out, "q": q, "dv": dv, "seg_rows": seg_rows, "db": db, "dG": dG, "dW": dW}


def close(name, got, want, what):
    g, scale = got.cpu().numpy().astype(np.float64), np.abs(want).max() if want.size else 0.0
    err = float(np.abs(g - want).max()) if want.size else 0.0
    print(f"{what}: {name} max|ref| {scale:.3g}, error {err:.3g}")
    np.testing.assert_allclose(g, want, rtol=0, atol=2e-4 * scale + 1e-9, err_msg=f"{what}: {name}")


def check_case(tspn, device, c, what):
    r = ref.loss_ref(c["feats"], c["pairs"], c["spans"], c["span_count"], c["span_labels"], c["cls_w"], c["cls_b"], c["pair_off"])
    d, got = run_ops(tspn, device, c)
    NT, T, D, K, G, S = c["dims"]
    valid = r["valid"]
    assert valid.any() and (~valid).any()
    # q: span pooling's own bits on the rows, zero elsewhere
    rows = np.flatnonzero(valid)
    p_of, g_of = rows // G, rows % G
    spans = np.where((c["span_count"][p_of] == 0)[:, None], np.array([[0, T]]), c["spans"][p_of, g_of])
    pooled = tspn.ops.span_predicate(d["feats"], _t(c["pairs"][p_of]).to(device), _t(spans.astype(np.int64)).to(device),
                                     d["cls_w"], d["cls_b"])
    q = got["q"].cpu()
    assert torch.equal(q[_t(rows)], pooled.cpu()), f"{what}: q differs from ops.span_predicate"
    assert not q[_t(np.flatnonzero(~valid))].any() and not got["dv"].cpu()[_t(np.flatnonzero(~valid))].any()
    out = got["out"].cpu().numpy()
    print(f"{what}: loss {out[0]:.10g} vs {r['loss']:.10g}")
    np.testing.assert_allclose(out[0], r["loss"], rtol=2e-5, err_msg=what)
    np.testing.assert_allclose(out[1:], r["seg_loss"], rtol=2e-5, atol=0, err_msg=what)
    assert out[0] == np.cumsum(out[1:])[-1] and np.array_equal(got["seg_rows"].cpu().numpy(), r["seg_rows"])
    for name in ("dv", "db", "dG", "dW"):
        close(name, got[name], r[name], what)
    return r, got


@pytest.mark.parametrize("S,T,D,K,G", list(product((1, 2), (1, 2, 33), (16, 40), (1, 5, 145), (1, 3))))
def test_loss_and_gradients_against_the_restatement(tspn, device, S, T, D, K, G):
    for table in ("canonical", "shuffled"):
        c = ref.loss_case(1000 + 7 * T + D + K + G + S, 5, S, T, D, K, G, table=table)
        r, got = check_case(tspn, device, c, f"S={S} T={T} D={D} K={K} G={G} {table}")
        if table == "shuffled":
            NT = c["dims"][0]
            assert not (c["pairs"][r["valid"].reshape(-1, G).any(1)] == NT - 1).any()
            assert not got["dG"][NT - 1].any()                         # a tracklet no row names: written, zero
            assert len({tuple(x) for x in c["pairs"].tolist()}) < len(c["pairs"])   # the duplicated row


def test_loss_and_gradients_on_many_rows(tspn, device):
    """P = 992 random rows of N = 5 tracklets at G = 16, K = 145: 15872 rows, 3968 workgroups of the loss kernel, 62 strides
    of the finish kernel, every (tracklet, column) thread of the projection gradient walking 992 pairs."""
    c = ref.loss_case(77, 5, 1, 9, 16, 145, 16, P=992)
    check_case(tspn, device, c, "P=992 G=16")


def call_abi(tspn, device, d, dims, held):
    """Both loss entries and the gradient entry through the C ABI on caller-held outputs."""
    NT, T, D, K, G, S = dims
    lib, P, st = tspn._abi.lib(), d["pairs"].shape[0], tspn.ops._stream()
    need = lib.tspn_span_predicate_workspace_bytes(NT, T, D, K)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    o = {k: v[1] for k, v in held.items()}
    rc = lib.tspn_span_predicate_loss_f32(sb.p(d["feats"]), NT, T, D, sb.p(d["pairs"]), sb.p(d["pair_off"]), S, P, sb.p(d["spans"]),
                                          sb.p(d["span_count"]), sb.p(d["span_labels"]), G, sb.p(d["cls_w"]), sb.p(d["cls_b"]), K,
                                          sb.p(o["q"]), sb.p(o["dv"]), sb.p(o["partials"]), sb.p(o["seg_rows"]), sb.p(scratch),
                                          need, st)
    assert rc == 0, lib.tspn_last_error()
    rc = lib.tspn_span_predicate_loss_finish(sb.p(o["partials"]), sb.p(o["seg_rows"]), sb.p(d["pair_off"]), S, P, G, K,
                                             sb.p(o["out"]), st)
    assert rc == 0, lib.tspn_last_error()
    rc = lib.tspn_span_predicate_grad_f32(sb.p(o["dv"]), sb.p(d["pairs"]), sb.p(d["spans"]), sb.p(d["span_count"]), NT, T, P, G, K,
                                          sb.p(o["db"]), sb.p(o["dG"]), sb.p(scratch), need, st)
    assert rc == 0, lib.tspn_last_error()
    torch.cuda.synchronize(device)


def held_outputs(device, P, dims):
    NT, T, D, K, G, S = dims
    f64 = torch.float64
    return {"q": sb.held((P * G, K), device), "dv": sb.held((P * G, K), device), "partials": sb.held((P * G,), device, f64),
            "seg_rows": sb.held((S,), device, f64), "out": sb.held((1 + S,), device, f64), "db": sb.held((K,), device),
            "dG": sb.held((NT, T, 2 * K), device)}


@pytest.mark.parametrize("S,T,D,K,G", [(2, 33, 40, 145, 3), (1, 2, 16, 5, 1), (2, 1, 16, 1, 3)])
def test_outputs_are_written_inside_only_and_reproducible(tspn, device, S, T, D, K, G):
    """Every output between guard bands and filled with a sentinel: every element written, nothing outside; a second run
    gives dv, db, dG, q and the losses bit for bit; and the wrapper returns the same bits."""
    c = ref.loss_case(2000 + T + K, 5, S, T, D, K, G, table="shuffled")
    d = upload(device, c)
    runs = []
    for _ in range(2):
        held = held_outputs(device, len(c["pairs"]), c["dims"])
        call_abi(tspn, device, d, c["dims"], held)
        for name, (buf, v) in held.items():
            sb.assert_written_inside_only(buf, v, name)
        runs.append({k: v[1].clone() for k, v in held.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name].view(torch.uint8), runs[1][name].view(torch.uint8)), name
    _, got = run_ops(tspn, device, c)
    for name in ("out", "q", "dv", "seg_rows", "db", "dG"):
        assert torch.equal(got[name].view(torch.uint8), runs[0][name].view(torch.uint8)), name


def test_nan_reaches_exactly_the_rows_that_read_it(tspn, device):
    """A NaN in frame 0 of a tracklet whose pairs all have span_count -1 (no rows: nothing is read through them) leaves every
    output bit for bit; a NaN in a frame inside one row's span makes the loss NaN and dv NaN in exactly the rows the
    restatement names (the rows of that tracklet whose span holds the frame), finite in every other row."""
    c = ref.loss_case(3000, 5, 2, 33, 16, 5, 3, table="canonical")
    NT, T, D, K, G, S = c["dims"]
    lone = 7
    c["span_count"][(c["pairs"] == lone).any(1)] = -1
    _, clean = run_ops(tspn, device, c)
    dirty = dict(c, feats=c["feats"].copy())
    dirty["feats"][lone, 0, 3] = np.nan
    _, got = run_ops(tspn, device, dirty)
    for name in ("out", "q", "dv", "seg_rows", "db", "dG"):
        assert torch.equal(got[name].view(torch.uint8), clean[name].view(torch.uint8)), name
    # inside a row's span: pair 0 holds [0, 16) and [16, 33); frame 20 of its subject
    s0 = int(c["pairs"][0, 0])
    inside = dict(c, feats=c["feats"].copy())
    inside["feats"][s0, 20, 1] = np.nan
    r = ref.loss_ref(inside["feats"], c["pairs"], c["spans"], c["span_count"], c["span_labels"], c["cls_w"], c["cls_b"], c["pair_off"])
    _, got = run_ops(tspn, device, inside)
    dv, out = got["dv"].cpu().numpy(), got["out"].cpu().numpy()
    hit = np.isnan(r["dv"]).any(1)
    assert hit[1] and not hit[0] and 0 < hit.sum() < r["valid"].sum()          # row (0, 1) reads frame 20, row (0, 0) does not
    assert np.array_equal(np.isnan(dv), np.isnan(r["dv"])) and np.isnan(dv[hit]).all()
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.isfinite(out[2])      # the tracklet's own segment only
    np.testing.assert_allclose(dv[~hit], r["dv"][~hit], rtol=0, atol=2e-4 * np.abs(r["dv"][~hit]).max() + 1e-9)


def test_empty_operands_and_wrapper_refusals(tspn, device):
    ops = tspn.ops
    i64, i32 = torch.int64, torch.int32
    feats, w, b = torch.randn(4, 3, 8, device=device), torch.randn(5, 16, device=device), torch.zeros(5, device=device)
    none = (torch.zeros((0, 2), dtype=i64, device=device), torch.zeros((0, 2, 2), dtype=i64, device=device),
            torch.zeros((0,), dtype=i32, device=device))
    out, q, dv, seg_rows, scratch = ops.span_predicate_loss(feats, none[0], none[1], none[2], torch.zeros((0, 2, 5), device=device), w, b)
    assert out.cpu().tolist() == [0.0, 0.0] and q.shape == dv.shape == (0, 5) and seg_rows.cpu().tolist() == [0.0]
    db, dG = ops.span_predicate_grad(dv, *none, 4, 3, scratch=scratch)
    assert not db.any() and not dG.any() and dG.shape == (4, 3, 10)
    # a batch whose pairs all have no rows: zero loss, zero gradient
    pairs = torch.tensor([[0, 1], [2, 3]], dtype=i64, device=device)
    spans, count = torch.zeros((2, 2, 2), dtype=i64, device=device), torch.full((2,), -1, dtype=i32, device=device)
    out, q, dv, _, scratch = ops.span_predicate_loss(feats, pairs, spans, count, torch.ones((2, 2, 5), device=device), w, b)
    assert out.cpu().tolist() == [0.0, 0.0] and not q.any() and not dv.any()
    with pytest.raises(ValueError, match=r"span_labels must be \[P,G,K\]"):
        ops.span_predicate_loss(feats, pairs, spans, count, torch.ones((2, 2, 4), device=device), w, b)
    with pytest.raises(ValueError, match="1 <= G <= 16"):
        ops.span_predicate_loss(feats, pairs, torch.zeros((2, 17, 2), dtype=i64, device=device), count,
                                torch.ones((2, 17, 5), device=device), w, b)
    with pytest.raises(ValueError, match=r"dv must be \[P\*G,K\]"):
        ops.span_predicate_grad(torch.zeros((3, 5), device=device), pairs, spans, count, 4, 3)
    with pytest.raises(ValueError, match="workspace too small"):
        ops.span_predicate_grad(dv, pairs, spans, count, 4, 3, scratch=torch.empty(8, dtype=torch.uint8, device=device))
