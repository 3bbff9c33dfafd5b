"""Every workspace-taking entry of the C ABI held to its scratch contract (include/tspn_mi355x.h, Conventions; the table
is tests/workspace_contracts.py): a workspace may hold anything on entry, `need` bytes suffice, nothing outside them is
touched, a shorter one is refused before any device work.

Each entry runs through its ordinary Python wrapper while `ops._ws` is replaced (tests/workspace_contract.py) by a
function that hands out a view of EXACTLY the bytes the size helper asked for, between two 64 KiB guard bands, in one
of three states: zeros, 0xFF in every byte (a NaN in fp32 / bf16 / fp16, -1 in every integer width), or what a launch of
the same entry on other inputs and other weights of the same shape left there.  Asserted per case:
  * the outputs of the three runs are equal bit for bit (compared as integers);
  * the 0xFF run has no NaN in its outputs and meets the float64 / oracle reference of the entry's own test, at that
    test's bound (the helpers and the inputs' distributions are imported from those tests; nothing here has a
    tolerance of its own);
  * both guard bands are intact after every run; outputs the wrapper lets the caller hold (`out=`, `out_heads=`,
    `out_logits=`) sit in sentinel-filled buffers: every element written, nothing outside, and a row the entry documents
    as skipped keeps the sentinel;
  * with one byte less than `need`, or no workspace at all, the entry refuses and neither the outputs nor the (0xFF)
    workspace change.  The memory behind the short view is the full view: an entry that fails to refuse runs on valid
    memory and trips a guard band.
One test scores videos of different shapes one after the other through a BaseModel whose persistent workspace starts as
0xFF -- the production pattern: every piece of a layout holds what another layout left there.  The split buffer of
tspn_heads_pairgrid_f16x3 is no `void* workspace` but promises the same (workspace_contracts.OTHER_SCRATCH): it is held
the same way, and one buffer is carried from a call to the next with other weights, H and C."""

import numpy as np
import pytest
import torch

import cases
import oracle
import pairf16_reference as pfref
import pairlist_reference as plref
import sentinel_buffers as sb
import span_bf16_reference as sbref
import span_relations_reference as srref
import workspace_contract as wsc
from oracle import roi_head_oracle as ro

import test_gpu_pairlist_bf16 as t_pl
import test_gpu_span_predicate as t_sp
import test_gpu_span_relations as t_sr
import test_gpu_wino63 as t_w63
import test_gpu_wino63_f16x3_tail as t_tail
from test_gpu_bf16 import check_against_oracle, oracle_weights, r16

pytestmark = pytest.mark.gpu

A = 4


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------ the contract
def check_held(helds, what):
    """helds: (buffer, view, unwritten) of sentinel_buffers.held outputs; `unwritten` = None (every element written) or
    a bool mask over the view of the elements that must KEEP the sentinel."""
    for buf, v, unwritten in helds:
        b = buf.cpu()
        n, lo = v.numel(), v.storage_offset()
        s = sb.sentinel_of(b)
        assert bool((b[:lo] == s).all()) and bool((b[lo + n:] == s).all()), f"{what}: wrote outside an output"
        kept = (b[lo:lo + n] == s).view(v.shape)
        want = torch.zeros(v.shape, dtype=torch.bool) if unwritten is None else unwritten
        assert torch.equal(kept, want), \
            f"{what}: {int((kept & ~want).sum())} outputs never written, {int((want & ~kept).sum())} written that must be skipped"


def hold(tspn, what, run, a, b, check):
    """run(inputs, helds) -> tuple of output tensors, through the entry's wrapper WITHOUT a workspace argument (so the
    wrapper asks ops._ws); it appends the sentinel-held outputs it passes to `helds`.  a: the inputs under test, b:
    other inputs and other weights of the same shape (the stale run's predecessor); check(outputs): the reference."""
    ops = tspn.ops
    got = {}
    for fill in ("zero", "ones"):
        helds = []
        with wsc.guarded_ops_ws(ops, fill):
            got[fill] = run(a, helds)
        check_held(helds, f"{what} [{fill}]")
    with wsc.guarded_ops_ws(ops, "stale") as before:
        run(b, [])
    helds = []
    with wsc.guarded_ops_ws(ops, "stale", reuse=before) as rec:
        got["stale"] = run(a, helds)
    assert rec.calls == before.calls
    check_held(helds, f"{what} [stale]")
    for fill in ("ones", "stale"):
        assert len(got[fill]) == len(got["zero"])
        for k, (x, y) in enumerate(zip(got["zero"], got[fill])):
            assert wsc.same_bits(x, y), f"{what}: output {k} depends on what the workspace held (zero vs {fill})"
    for k, o in enumerate(got["ones"]):
        if o.is_floating_point():
            assert not bool(torch.isnan(o).any()), f"{what}: output {k} has NaN: the 0xFF of the workspace leaked"
    check(got["ones"])


class _NoWorkspace:
    """What a wrapper sees of a workspace: a null pointer that claims `need` bytes."""

    def __init__(self, nbytes):
        self.n = max(int(nbytes), 256)

    def data_ptr(self):
        return 0

    def numel(self):
        return self.n

    def element_size(self):
        return 1


def refused_untouched(tspn, what, run, a):
    ops, E = tspn.ops, tspn._abi
    helds = []
    with wsc.guarded_ops_ws(ops, "ones", short=1) as rec:
        with pytest.raises(E.TspnError) as e:
            run(a, helds)
    assert e.value.code == E.TSPN_EWORKSPACE, f"{what}: need - 1 bytes gave {e.value}"
    rec.assert_untouched(f"{what} (need - 1 bytes)")
    for buf, _, _ in helds:
        sb.assert_untouched(buf, f"{what} (need - 1 bytes)")
    helds, orig = [], ops._ws
    ops._ws = lambda nbytes, device: _NoWorkspace(nbytes)
    try:
        with pytest.raises(E.TspnError) as e:
            run(a, helds)
    finally:
        ops._ws = orig
    assert e.value.code in (E.TSPN_EWORKSPACE, E.TSPN_EINVAL), f"{what}: a null workspace gave {e.value}"
    torch.cuda.synchronize()
    for buf, _, _ in helds:
        sb.assert_untouched(buf, f"{what} (null workspace)")


# ------------------------------------------------------------------------------------------------ predicate heads
def case_predicate_head(tspn, device, P, F, K):
    """tests/test_gpu_ops.py::test_predicate_head_shapes: its distribution, its bound (5e-6)."""
    def inputs(seed):
        return (tspn.hashrng.uniform(seed, "x", (P, F), -1.0, 1.0), tspn.hashrng.normal(seed, "w", (K, F), std=0.05),
                tspn.hashrng.normal(seed, "b", (K,), std=0.1))

    def run(inp, helds):
        return (tspn.ops.predicate_head(*(t(v).to(device) for v in inp)),)

    a = inputs(21)

    def check(outs):
        ref = oracle.predicate_head(*(t(v).double() for v in a)).float().numpy()
        np.testing.assert_allclose(outs[0].cpu().numpy(), ref, rtol=0, atol=5e-6)
    return run, a, inputs(22), check


def case_predicate_head_norm(tspn, device, P, F, K, norm):
    """tests/test_gpu_ops.py::test_predicate_head_fused_preprocess_vs_oracle: its distribution (one all-zero block), 5e-6."""
    def inputs(seed):
        x = tspn.hashrng.uniform(seed, "x", (P, F), -1.0, 1.0)
        x[min(2, P - 1), norm[0]:norm[0] + norm[1]] = 0
        return x, tspn.hashrng.normal(seed, "w", (K, F), std=0.05), tspn.hashrng.normal(seed, "b", (K,), std=0.1)

    def run(inp, helds):
        return (tspn.ops.predicate_head(*(t(v).to(device) for v in inp), norm=norm),)

    a = inputs(25)

    def check(outs):
        x, w, b = (t(v).double() for v in a)
        ref = oracle.predicate_head(oracle.feature_preprocess(x, *norm), w, b)
        np.testing.assert_allclose(outs[0].cpu().numpy(), ref.float().numpy(), rtol=0, atol=5e-6)
    return run, a, inputs(26), check


@pytest.mark.parametrize("P,F,K", [(65, 257, 145), (200, 1001, 132)])
def test_predicate_head(tspn, device, P, F, K):
    """More than one K-slice, ragged row (P % 64) and column (K % 144, K > 144) tiles of the split-K GEMM."""
    assert tspn._abi.lib().tspn_predicate_head_workspace_bytes(P, F, K) > P * K * 4
    hold(tspn, f"predicate_head P={P} F={F} K={K}", *case_predicate_head(tspn, device, P, F, K))


@pytest.mark.parametrize("P,F,K,norm", [(3, 40, 5, (4, 6, 5)), (65, 257, 145, (1, 16, 16)), (200, 1001, 132, (1, 250, 4))])
def test_predicate_head_norm(tspn, device, P, F, K, norm):
    """Blocks narrower than a wave (6 and 16 columns: one short slice each), and blocks cut into several slices."""
    hold(tspn, f"predicate_head norm={norm} P={P} F={F} K={K}", *case_predicate_head_norm(tspn, device, P, F, K, norm))


# ------------------------------------------------------------------------------------------------ F(6,3) convolutions
def case_conv3_wino63(tspn, device, B, T, Cin, M):
    """tests/test_gpu_wino63.py::test_conv3_winograd63_vs_fp64: its distribution, its bound (6e-5)."""
    def inputs(seed):
        return (tspn.hashrng.uniform(seed, "x", (B, T, Cin), -1, 1), tspn.hashrng.normal(seed, "w", (M, Cin, 3), std=0.1),
                tspn.hashrng.normal(seed, "b", (M,), std=0.1))

    def run(inp, helds):
        x, w, b = (t(v).to(device) for v in inp)
        return (tspn.ops.conv3_tc_wino63(x, tspn.ops.pack_conv3_wino63(w), b, relu=False),)

    a = inputs(61)

    def check(outs):
        np.testing.assert_allclose(outs[0].cpu().numpy(), t_w63.conv_ref(*a, False), rtol=0, atol=6e-5)
    return run, a, inputs(62), check


@pytest.mark.parametrize("B,T,Cin,M", [(3, 7, 32, 256), (3, 149, 32, 160), (3, 150, 32, 256)])
def test_conv3_wino63(tspn, device, B, T, Cin, M):
    """T = 7, 149: the last sextet of a tracklet has one / five frames; 3 * ceil(T / 6) = 6, 75 sextets leave the
    64-sextet column tile partly padded; M = 160: a partial 128-row tile."""
    hold(tspn, f"conv3_tc_wino63 B={B} T={T} Cin={Cin} M={M}", *case_conv3_wino63(tspn, device, B, T, Cin, M))


def case_conv3_wino63_f16x3(tspn, device, B, T, Cin, M):
    """tests/test_gpu_wino63_f16x3_tail.py: its operands, its sampled float64 reference and bounds."""
    w, pk = t_tail.weights(tspn, device, M, Cin)
    g = torch.Generator(device=device).manual_seed(7)
    bias = torch.randn((M,), generator=g, device=device) * 0.05
    w2 = torch.randn((M, Cin, 3), generator=g, device=device) * 0.1
    a = (t_tail.make_x(device, B, T, Cin, 2000 + T), pk, bias)
    b = (t_tail.make_x(device, B, T, Cin, 2500 + T), tspn.ops.pack_conv3_wino63_f16x3(w2), bias * 2)

    def run(inp, helds):
        return (tspn.ops.conv3_tc_wino63_f16x3(*inp),)

    def check(outs):
        t_tail.check_against_float64(outs[0], a[0], w, bias, f"f16x3 B={B} T={T}")
    return run, a, b, check


@pytest.mark.parametrize("T,scenario", [(150, "r0"), (149, "f4"), (7, "small")])
def test_conv3_wino63_f16x3(tspn, device, T, scenario):
    """Cin = 64, M = 256 (the entry admits no partial row tile: M % 256 == 0); a grid that fills its last round (r0), one
    whose last round is cut in four (f4), one with fewer tiles than CUs (small) -- each with the tail split on and off:
    every tile, whole or cut, parks the accumulators of seven of its eight points in the workspace and reads them back."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    Cin, M, nq = 64, 256, -(-T // 6)
    tiles_n = t_tail.grid_for(scenario, M // t_tail.F_BM, cus)
    assert tiles_n is not None
    B = tiles_n * t_tail.F_BN // nq
    case = case_conv3_wino63_f16x3(tspn, device, B, T, Cin, M)
    assert tspn.ops.wino63_f16x3_set_tail_split(1) == 1
    try:
        for on in (1, 0):
            tspn.ops.wino63_f16x3_set_tail_split(on)
            hold(tspn, f"conv3_tc_wino63_f16x3 {scenario} T={T} B={B} tail split {on}", *case)
    finally:
        tspn.ops.wino63_f16x3_set_tail_split(1)


# ------------------------------------------------------------------------------------------------ decode
def case_decode_topk(tspn, device, S, N, K, kp, ks):
    """tests/test_gpu_ops.py::test_decode_topk_vs_oracle_with_ties: quantised scores (ties at both levels), bit equality."""
    P = N * (N - 1)
    pairs = np.stack([cases.ref_pairs(N)] * S)

    def inputs(seed):
        logit = np.round(tspn.hashrng.uniform(seed, "dec", (S, P, K)) * 16) / 16
        logit[:, :, 3] = 1.0
        feat = tspn.hashrng.uniform(seed, "feat", (S, P, 75))
        feat[:, :, 2] = feat[:, :, 9]
        return logit.astype(np.float32), feat.astype(np.float32)

    def run(inp, helds):
        logit, feat = inp
        return tspn.ops.decode_topk(t(logit).to(device), t(pairs).to(device), t(feat).to(device), row_mul=N - 1,
                                    topk_per_pair=kp, topk_per_seg=ks)

    a = inputs(61)

    def check(outs):
        sc, trip, tids = outs
        for s in range(S):
            rs, rt, ri = oracle.decode_topk(t(a[0][s]), t(a[1][s, :, :70]), t(pairs[s]), N, kp, ks)
            np.testing.assert_array_equal(sc[s].cpu().numpy(), rs.numpy())
            np.testing.assert_array_equal(trip[s].cpu().numpy(), rt.numpy())
            np.testing.assert_array_equal(tids[s].cpu().numpy(), ri.numpy())
    return run, a, inputs(63), check


@pytest.mark.parametrize("S,N,K,kp,ks", [(3, 8, 132, 20, 200), (1, 2, 5, 20, 200)])
def test_decode_topk(tspn, device, S, N, K, kp, ks):
    """Three segments; K = 5 < topk_per_pair = 20: five candidates per pair, ten in the segment (< topk_per_seg)."""
    hold(tspn, f"decode_topk S={S} N={N} K={K}", *case_decode_topk(tspn, device, S, N, K, kp, ks))


# ------------------------------------------------------------------------------------------------ fused fp32 pass
def dpn_weights(tspn, seed, D, K):
    sd = tspn.synth.make_weights(seed, c=2 * D, a=A, k=K, bias_std=0.05)
    return oracle_weights(sd)


def explicit_table(N):
    """Local ids: a third of the canonical table, two (i, i) rows, and four rows a second time."""
    can = oracle.pair_index(N)
    return torch.cat([can[::3], torch.tensor([[1, 1], [N - 1, N - 1]]), can[:4]]).contiguous()


# algo -> (weights seed and K of the test whose bound is used, pack, bound on the heads, bound on the logits)
#   direct: tests/test_gpu_kernel_variants.py::test_forward_fused_conv_and_pair_paths (float64 oracle, 2e-5)
#   wino63: tests/test_gpu_wino63.py::test_fused_winograd63_vs_dense_oracle (1e-5 on the heads) and
#           tests/test_gpu_ops.py::test_forward_fused_vs_dense_oracle (1e-5 on the logits, which no conv algorithm touches)
#   f16x3:  tests/test_gpu_kernel_variants.py::test_forward_fused_f16x3_against_dense_oracle (6e-5 / 2e-5)
FUSED_ALGOS = {
    "direct": (7, 37, lambda ops, w, D: ops.pack_conv3(w, split=D), 2e-5, 2e-5),
    "wino63": (50, 132, lambda ops, w, D: ops.pack_conv3_wino63(w, split=D), 1e-5, 1e-5),
    "f16x3": (7, 37, lambda ops, w, D: ops.pack_conv3_wino63_f16x3(w, split=D), 6e-5, 2e-5),
}


def case_forward_fused(tspn, device, B, N, T, D, algo, canonical, conv_check=0):
    seed, K, pack, tol_h, tol_l = FUSED_ALGOS[algo]
    local = oracle.pair_index(N) if canonical else explicit_table(N)
    pairs = torch.cat([local + v * N for v in range(B)]).contiguous()
    P = pairs.shape[0]
    dv = lambda v: v.to(device).contiguous()   # noqa: E731

    def inputs(wseed, vseed):
        w = dpn_weights(tspn, wseed, D, K)
        vids = [tspn.synth.make_video(vseed + v, N, T, D) for v in range(B)]
        return w, vids

    def run(inp, helds):
        w, vids = inp
        feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
        hw = dv(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]))
        hb = dv(torch.cat([w["rel_b"], w["dur_b"]]))
        hh, hl = sb.held((P, 3 * A, T), device), sb.held((P, K), device)
        helds += [(*hh, None), (*hl, None)]
        kw = dict(conv_weight=dv(w["conv_w"]), conv_check=conv_check) if conv_check else {}
        return tspn.ops.forward_fused(dv(feats), dv(pairs), B, N, pack(tspn.ops, dv(w["conv_w"]), D), dv(w["conv_b"]), hw, hb,
                                      dv(w["cls_w"]), dv(w["cls_b"]), canonical_pairs=canonical, out_heads=hh[1],
                                      out_logits=hl[1], **kw)

    a = inputs(seed, 60)

    def check(outs):
        heads, logits = (o.cpu().numpy() for o in outs)
        w, vids = a
        w64 = {k: v.double() for k, v in w.items()}
        per = local.shape[0]
        for v in range(B):
            ref = oracle.forward_dense(t(vids[v]["tracklet_feats"]).double(), t(vids[v]["tracklet_boxes"]).double(), local, w64)
            sl = slice(v * per, (v + 1) * per)
            np.testing.assert_allclose(heads[sl, :A], ref["relness"].numpy(), rtol=0, atol=tol_h)
            np.testing.assert_allclose(heads[sl, A:], ref["duration"].numpy(), rtol=0, atol=tol_h)
            np.testing.assert_allclose(logits[sl], ref["rel_logits"].numpy(), rtol=0, atol=tol_l)
    return run, a, inputs(seed + 1, 160), check


FUSED_CASES = [
    (3, 5, 30, 16, "direct"),     # channels-last conv; canonical: ldy = 32, two pad frames per row of y
    (1, 9, 33, 16, "direct"),     # odd T: ldy = T
    (3, 5, 33, 18, "direct"),     # D % 16 != 0: the xt transpose piece and tspn_conv3_f32
    (3, 5, 7, 32, "wino63"),      # the second sextet of a tracklet has one frame; 30 sextets in a 64-sextet column tile
    (1, 9, 149, 32, "wino63"),    # five frames in the last sextet; 225 sextets = 3.5 column tiles
    (1, 9, 150, 32, "wino63"),    # whole sextets; canonical: ldy = 152
    (3, 5, 7, 64, "f16x3"),
    (1, 9, 149, 64, "f16x3"),
    (1, 9, 150, 64, "f16x3"),
]


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "table"])
@pytest.mark.parametrize("B,N,T,D,algo", FUSED_CASES, ids=["-".join(map(str, c)) for c in FUSED_CASES])
def test_forward_fused(tspn, device, B, N, T, D, algo, canonical):
    """tspn_forward_fused_f32 on each conv algorithm and both pair stages; "table" = an explicit pair table with repeated
    rows and (i, i) rows (the indexed pair stage, ldy = T)."""
    hold(tspn, f"forward_fused {algo} B={B} N={N} T={T} D={D} canonical={canonical}",
         *case_forward_fused(tspn, device, B, N, T, D, algo, canonical))


@pytest.mark.parametrize("algo", ["wino63", "f16x3"])
def test_forward_fused_accuracy_guard_scratch(tspn, device, algo):
    """F(6,3) with conv_check > 0 and an attached status block: the last piece of the layout (`hot`) is the spot check's
    scratch -- its meeting words and the 64 slots the input transform reports the largest |x| into.  Whatever the
    workspace held, the largest key names the planted outlier's sextet, the meeting words are left zeroed, and the
    spot check reaches the status block (as tests/test_gpu_status_guard.py asserts on a zeroed workspace)."""
    E = tspn._abi
    B, N, T, D, rows = 2, 3, 40, 64, 16
    run, a, b, check = case_forward_fused(tspn, device, B, N, T, D, algo, True, conv_check=rows)
    trk, frame, ch = 4, 27, 13                                     # video 1, tracklet 1
    a[1][1]["tracklet_feats"][trk - N, frame, ch] = -37.5
    words = tspn.ops.status_words(device)                          # attaches the block
    nq = (T + 5) // 6

    def run_and_look(inp, helds):
        words[E.STATUS_CONV_ERR] = 0
        words[E.STATUS_CONV_CHECKS] = 0
        outs = run(inp, helds)
        torch.cuda.synchronize(device)
        if inp is a:
            _, view, need = tspn.ops._ws.records[-1]
            scratch = view[need - E.CONV_CHECK_SCRATCH_BYTES:need].view(torch.int64)
            slots = scratch[E.CONV_CHECK_HOT_OFFSET // 8::32][:64].cpu().numpy().astype(np.uint64)
            key = int(slots.max())
            assert key & 0xFFFFFFFF == trk * nq + frame // 6, f"hot slots hold {key:#x}"
            if algo == "wino63":
                assert np.array([key >> 32], dtype=np.uint32).view(np.float32)[0] == np.float32(37.5)
            assert bool((scratch[:4] == 0).all()), "the spot check did not leave its meeting words zeroed"
            err = float(words[E.STATUS_CONV_ERR:E.STATUS_CONV_ERR + 1].view(np.float32)[0])
            checks = int(words[E.STATUS_CONV_CHECKS])
            assert 0.0 < err < 1e-4 and checks % rows == 0 and rows * 18 <= checks <= rows * 24, (err, checks)
        return outs

    try:
        hold(tspn, f"forward_fused {algo} with the accuracy guard", run_and_look, a, b, check)
    finally:
        words[E.STATUS_CONV_ERR] = 0
        words[E.STATUS_CONV_CHECKS] = 0


# ------------------------------------------------------------------------------------------------ bf16 passes
def bf16_table(kind, B, N):
    """(global table [P,2], mask of the rows that are skipped).  sparse: with N = 17 the compacted 17 x 17 slot grid has
    four 16 x 16 tiles, and the one of (subject 16, object 16) holds no row; cross: one row joins two videos."""
    can = oracle.pair_index(N)
    if kind == "canonical":
        tab = torch.cat([can + v * N for v in range(B)])
        return tab.contiguous(), torch.zeros(len(tab), dtype=torch.bool)
    keep = torch.cat([can[can[:, 1] < N - 1][::2], torch.tensor([[0, N - 1], [2, N - 1]])])
    local = torch.cat([keep, torch.tensor([[2, 2]]), keep[:3]])
    tab = torch.cat([local + v * N for v in range(B)])
    skipped = torch.zeros(len(tab), dtype=torch.bool)
    if kind == "cross":
        assert B > 1
        tab[5] = torch.tensor([1, N + 2])
        skipped[5] = True
    return tab.contiguous(), skipped


def case_forward_fused_bf16(tspn, device, B, N, T, D, kind):
    """tests/test_gpu_bf16.py / test_gpu_pairlist_bf16.py: every weight rounded to bf16, oracle.forward_bf16 per video,
    check_against_oracle (2e-3 of the output range: a few flipped bf16 activations)."""
    K = 132
    table, skipped = bf16_table(kind, B, N)
    P = table.shape[0]
    canonical = kind == "canonical"

    def inputs(wseed, vseed):
        sd = tspn.synth.make_weights(wseed, c=2 * D, bias_std=0.05)
        return oracle_weights(sd), [tspn.synth.make_video(vseed + v, N, T, D) for v in range(B)]

    def run(inp, helds):
        w0, vids = inp
        w = {k: r16(x.numpy()).to(device) for k, x in w0.items()}
        feats = torch.cat([t(v["tracklet_feats"]) for v in vids]).to(torch.bfloat16).to(device)
        hw = torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]).contiguous()
        hb = torch.cat([w["rel_b"], w["dur_b"]]).contiguous()
        hh, hl = sb.held((P, 3 * A, T), device), sb.held((P, K), device)
        helds += [(*hh, skipped.view(-1, 1, 1).expand(P, 3 * A, T)), (*hl, None)]
        return tspn.ops.forward_fused_bf16(feats, table.to(device), B, N, tspn.ops.pack_conv3_bf16(w["conv_w"], split=D),
                                           w["conv_b"], tspn.ops.pack_heads_bf16(hw), hb, w["cls_w"], w["cls_b"],
                                           out_heads=hh[1], out_logits=hl[1], canonical_pairs=canonical, check_pairs=False)

    a = inputs(0, 90)

    def check(outs):
        heads, logits = (o.cpu() for o in outs)
        w0, vids = a
        for v in range(B):
            rows = torch.nonzero((table[:, 0] // N == v) & ~skipped).flatten()
            want = oracle.forward_bf16(t(vids[v]["tracklet_feats"]), table[rows] - v * N, w0)
            check_against_oracle(heads[rows, :A], want["relness"], f"relness of video {v}")
            check_against_oracle(heads[rows, A:], want["duration"], f"duration of video {v}")
            check_against_oracle(logits[rows], want["rel_logits"], f"rel_logits of video {v}")
    return run, a, inputs(1, 190), check


BF16_CASES = [(1, 17, 7, 16, "canonical"), (2, 16, 30, 32, "canonical"), (1, 17, 30, 16, "sparse"), (2, 17, 7, 32, "cross"),
              (2, 16, 31, 16, "sparse")]


@pytest.mark.parametrize("B,N,T,D,kind", BF16_CASES, ids=["-".join(map(str, c)) for c in BF16_CASES])
def test_forward_fused_bf16(tspn, device, B, N, T, D, kind):
    """tspn_forward_fused_bf16 (canonical) and tspn_forward_fused_bf16_pairs (sparse, cross).  N = 17: Np = 32, fifteen
    padded slots per list and video; N = 16: none.  The row that joins two videos is skipped: its row of the heads keeps
    the sentinel, every other row is written."""
    hold(tspn, f"forward_fused_bf16 {kind} B={B} N={N} T={T} D={D}", *case_forward_fused_bf16(tspn, device, B, N, T, D, kind))


def case_heads_pairlist(tspn, device, B, N, T, C, kind):
    """tests/test_gpu_pairlist_bf16.py: its operands (seed 83), pairlist_reference.heads_list_ref64, 3e-5."""
    table, skipped = bf16_table(kind, B, N)
    P, H = table.shape[0], t_pl.H

    def inputs(seed):
        return (t(tspn.hashrng.normal(seed, "y", (B * N, T, 2 * C), std=1.0)), r16(tspn.hashrng.normal(seed, "hw", (H, C), std=0.1)),
                t(tspn.hashrng.normal(seed, "hb", (H,), std=0.1)))

    def run(inp, helds):
        y, hw, hb = inp
        ho = sb.held((P, H, T), device)
        helds.append((*ho, skipped.view(-1, 1, 1).expand(P, H, T)))
        return (t_pl.run_list(tspn, device, y, table.numpy(), B, N, hw, hb, out=ho[1], check_pairs=False),)

    a = inputs(83)

    def check(outs):
        keep = torch.nonzero(~skipped).flatten()
        want = plref.heads_list_ref64(a[0], table[keep].numpy(), a[1], a[2])
        np.testing.assert_allclose(outs[0].cpu()[keep].numpy(), want.numpy(), rtol=0, atol=t_pl.ATOL)
    return run, a, inputs(84), check


@pytest.mark.parametrize("B,N,T,C,kind", [(1, 17, 20, 32, "sparse"), (2, 16, 37, 64, "canonical"), (2, 17, 20, 32, "cross"),
                                          (2, 5, 18, 32, "cross")])
def test_heads_pairlist_bf16(tspn, device, B, N, T, C, kind):
    """The plan's arrays in an exact workspace: Np = 32 with N = 17 (an empty tile, list slots past the counts), N = 16,
    the 8 x 8 form (N = 5), a skipped row (on no chain: next = -1, its output row untouched)."""
    hold(tspn, f"heads_pairlist_bf16 {kind} B={B} N={N} T={T} C={C}", *case_heads_pairlist(tspn, device, B, N, T, C, kind))


# ------------------------------------------------------------------------------------------------ span pooling
def case_span_predicate(tspn, device, NT, T, D, K):
    """tests/test_gpu_span_predicate.py: its operands, rule rows (spans that touch frame 0 and T, empty, reversed, (-1, -1)),
    float64 reference and derived tolerance."""
    pairs = t_sp.all_pairs_with_self(NT, 40)

    def inputs(seed):
        rs, f, w, b = t_sp.make_operands(seed, NT, T, D, K)
        return f, pairs, t_sp.draw_spans(rs, len(pairs), T), w, b

    def run(inp, helds):
        return (tspn.ops.span_predicate(*(t(x).to(device) for x in inp)),)

    a = inputs(704 + NT)

    def check(outs):
        ref, z, S, _ = t_sp.span_predicate_ref(*a)
        t_sp.check_against_ref(outs[0].cpu().numpy(), ref, z, S, f"span_predicate NT={NT} T={T} D={D} K={K}")
    return run, a, inputs(904 + NT), check


@pytest.mark.parametrize("NT,T,D,K", [(3, 1, 16, 3), (4, 9, 40, 145), (5, 9, 13, 7)])
def test_span_predicate(tspn, device, NT, T, D, K):
    """T = 1; T = 9 with the rule rows; 2K = 290: two column tiles plus two columns; D = 13."""
    hold(tspn, f"span_predicate NT={NT} T={T} D={D} K={K}", *case_span_predicate(tspn, device, NT, T, D, K))


def case_span_predicate_bf16(tspn, device, NT, T, D, K):
    """tests/test_gpu_span_predicate_bf16.py / span_bf16_reference.py: operands, reference and tolerance."""
    pairs = t_sp.all_pairs_with_self(NT, 40)
    P = len(pairs)

    def inputs(seed):
        rs, f, w, b = sbref.make_operands(seed, NT, T, D, K)
        return f, pairs, sbref.draw_spans(rs, P, T), w, b

    def run(inp, helds):
        f, pr, sp, w, b = inp
        ho = sb.held((P, K), device)
        helds.append((*ho, None))
        return (tspn.ops.span_predicate_bf16(t(f).to(torch.bfloat16).to(device), t(pr).to(device), t(sp).to(device),
                                             tspn.ops.pack_span_cls_bf16(t(w).to(device)), t(b).to(device), K, out=ho[1]),)

    a = inputs(800 + T)

    def check(outs):
        r, z, S, _ = sbref.span_predicate_ref(*a)
        sbref.check_against_ref(outs[0].cpu().numpy(), r, z, S, D, f"span_predicate_bf16 NT={NT} T={T} D={D} K={K}")
    return run, a, inputs(850 + T), check


@pytest.mark.parametrize("NT,T,D,K", [(3, 1, 16, 3), (4, 9, 16, 145), (5, 9, 48, 17)])
def test_span_predicate_bf16(tspn, device, NT, T, D, K):
    """D = 16: one k-step; T = 1; T = 9 with the rule rows; K = 145: ten 16-column tiles, the last with one column."""
    hold(tspn, f"span_predicate_bf16 NT={NT} T={T} D={D} K={K}", *case_span_predicate_bf16(tspn, device, NT, T, D, K))


# ------------------------------------------------------------------------------------------------ span relations
def relations_case(tspn, device, bf16, S, N, T, D, K, J, seed, empty_pair):
    c = (t_sr.make_case(device, S, N, T, D, K, J, seed=seed))
    if bf16:
        c["feats"] = c["feats"].to(torch.bfloat16)
        c["packed"] = tspn.ops.pack_span_cls_bf16(c["w"])
    heads = c["heads"].clone()
    if empty_pair:
        heads[1] = float("nan")                                   # pair 1 of segment 0: no proposal, count = 0
    t_sr.with_spans(tspn, c, heads)
    if empty_pair:
        assert int(c["count"][1]) == 0 and int((c["count"] > 0).sum()) > 0
    return c


def case_decode_span_relations(tspn, device, bf16, S, N, T, D, K, J, R, M, empty_pair):
    """tests/test_gpu_span_relations.py / _bf16.py: the fused entry equals, bit for bit, the composition of span pooling
    (the entry's own wrapper, outside the guarded runs) with the numpy selection of span_relations_reference."""
    a = relations_case(tspn, device, bf16, S, N, T, D, K, J, 100 + K + J, empty_pair)
    b = relations_case(tspn, device, bf16, S, N, T, D, K, J, 300 + K + J, False)

    def run(c, helds):
        out = t_sr.sentinel_out(c, R, M, device)
        if bf16:
            return tspn.ops.decode_span_relations_bf16(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["packed"],
                                                       c["b"], c["K"], c["cls"], topk_per_span=R, topk_per_seg=M, out=out)
        return tspn.ops.decode_span_relations(c["feats"], c["pairs"], c["spans"], c["score"], c["count"], c["w"], c["b"],
                                              c["cls"], topk_per_span=R, topk_per_seg=M, out=out)

    rp, rs = srref.span_rows(a["pairs"], a["N"], a["spans"])
    q = (tspn.ops.span_predicate_bf16(a["feats"], rp, rs, a["packed"], a["b"], a["K"]) if bf16
         else tspn.ops.span_predicate(a["feats"], rp, rs, a["w"], a["b"]))
    want = srref.compose(q, a["pairs"], a["spans"], a["score"], a["count"], a["cls"], R, M)

    def check(outs):
        t_sr.assert_equal([o.cpu().numpy() for o in outs], want)
        assert sum(w["valid"] for w in want) > 0
    return run, a, b, check


# (S, N, T, D, K, J, R, M, a pair without a proposal)
REL_F32 = [(1, 2, 1, 16, 1, 1, 1, 1, False), (2, 3, 9, 16, 145, 16, 20, 200, True), (2, 4, 9, 24, 20, 1, 5, 40, True)]
REL_BF16 = [(1, 2, 1, 16, 1, 1, 1, 1, False), (2, 3, 9, 16, 132, 16, 20, 200, True), (2, 4, 9, 32, 20, 1, 5, 40, True)]


@pytest.mark.parametrize("S,N,T,D,K,J,R,M,empty_pair", REL_F32, ids=["x".join(map(str, c[:8])) for c in REL_F32])
def test_decode_span_relations(tspn, device, S, N, T, D, K, J, R, M, empty_pair):
    """T = 1 and J = 1; J = 16 with K = 145 (three values per lane) and a pair whose count is 0 (its rows write the pad
    key: the candidate arrays are complete whatever they held)."""
    hold(tspn, f"decode_span_relations {(S, N, T, D, K, J, R, M)}",
         *case_decode_span_relations(tspn, device, False, S, N, T, D, K, J, R, M, empty_pair))


@pytest.mark.parametrize("S,N,T,D,K,J,R,M,empty_pair", REL_BF16, ids=["x".join(map(str, c[:8])) for c in REL_BF16])
def test_decode_span_relations_bf16(tspn, device, S, N, T, D, K, J, R, M, empty_pair):
    hold(tspn, f"decode_span_relations_bf16 {(S, N, T, D, K, J, R, M)}",
         *case_decode_span_relations(tspn, device, True, S, N, T, D, K, J, R, M, empty_pair))


# ------------------------------------------------------------------------------------------------ stem
def case_stem(tspn, device, NB, H, W, Cout, pool):
    """tests/test_gpu_roi_head.py::test_stem_bf16_vs_oracle (conv: 2^-8 of the range, < 1 % of the outputs off at all) and
    ::test_stem_pool_fused_bit_identical_to_conv_then_pool (pool: equal to conv + max pool bit for bit)."""
    def inputs(seed):
        return (tspn.hashrng.uniform(seed, "x", (NB, H, W, 3), -2, 2), tspn.hashrng.normal(seed, "w", (Cout, 3, 7, 7), std=0.1),
                tspn.hashrng.normal(seed, "b", (Cout,), std=0.1))

    def run(inp, helds):
        x, w, b = (t(v).to(device) for v in inp)
        fn = tspn.ops.stem_pool_bf16 if pool else tspn.ops.stem_conv_bf16
        return (fn(x, tspn.ops.pack_stem_bf16(w), b),)

    a = inputs(88)
    x, w, b = (t(v).to(device) for v in a)
    conv = tspn.ops.stem_conv_bf16(x, tspn.ops.pack_stem_bf16(w), b)          # outside the guarded runs

    def check(outs):
        if pool:
            assert torch.equal(outs[0], tspn.ops.max_pool_nhwc_bf16(conv, 3, 2, 1))
            assert wsc.same_bits(outs[0], tspn.ops.max_pool_nhwc_bf16(conv, 3, 2, 1))
            return
        ref = ro.conv2d_bf16(t(a[0]).permute(0, 3, 1, 2), t(a[1]), t(a[2]), stride=2, padding=3, relu=True).permute(0, 2, 3, 1)
        assert wsc.same_bits(outs[0], conv)
        err = (outs[0].cpu().double() - ref).abs()
        assert float(err.max()) <= 2.0 ** -8 * float(ref.abs().max()) and float((err > 0).double().mean()) < 0.01
    return run, a, inputs(89), check


@pytest.mark.parametrize("pool", [False, True], ids=["conv", "pool"])
@pytest.mark.parametrize("NB,H,W,Cout", [(1, 7, 7, 32), (2, 30, 41, 64)])
def test_stem_bf16(tspn, device, NB, H, W, Cout, pool):
    """Odd sizes: the 2x2 space-to-depth image has a padded last row and column, and a border of three pixels."""
    hold(tspn, f"stem {'pool' if pool else 'conv'} {(NB, H, W, Cout)}", *case_stem(tspn, device, NB, H, W, Cout, pool))


# ------------------------------------------------------------------------------------------------ short / no workspace
ENTRY_CASES = {
    "tspn_predicate_head_f32": lambda tspn, dev: case_predicate_head(tspn, dev, 65, 257, 145),
    "tspn_predicate_head_norm_f32": lambda tspn, dev: case_predicate_head_norm(tspn, dev, 65, 257, 145, (1, 16, 16)),
    "tspn_conv3_tc_wino63_f32": lambda tspn, dev: case_conv3_wino63(tspn, dev, 3, 7, 32, 256),
    "tspn_conv3_tc_wino63_f16x3": lambda tspn, dev: case_conv3_wino63_f16x3(tspn, dev, 128, 7, 64, 256),
    "tspn_decode_topk_f32": lambda tspn, dev: case_decode_topk(tspn, dev, 3, 8, 132, 20, 200),
    "tspn_forward_fused_f32": lambda tspn, dev: case_forward_fused(tspn, dev, 3, 5, 7, 64, "f16x3", True),
    "tspn_forward_fused_bf16": lambda tspn, dev: case_forward_fused_bf16(tspn, dev, 1, 17, 7, 16, "canonical"),
    "tspn_forward_fused_bf16_pairs": lambda tspn, dev: case_forward_fused_bf16(tspn, dev, 1, 17, 30, 16, "sparse"),
    "tspn_heads_pairlist_bf16": lambda tspn, dev: case_heads_pairlist(tspn, dev, 1, 17, 20, 32, "sparse"),
    "tspn_span_predicate_f32": lambda tspn, dev: case_span_predicate(tspn, dev, 4, 9, 40, 145),
    "tspn_decode_span_relations_f32": lambda tspn, dev: case_decode_span_relations(tspn, dev, False, 2, 4, 9, 24, 20, 1, 5, 40, True),
    "tspn_span_predicate_bf16": lambda tspn, dev: case_span_predicate_bf16(tspn, dev, 4, 9, 16, 145),
    "tspn_decode_span_relations_bf16": lambda tspn, dev: case_decode_span_relations(tspn, dev, True, 2, 4, 9, 32, 20, 1, 5, 40, True),
    "tspn_stem_conv_bf16": lambda tspn, dev: case_stem(tspn, dev, 1, 7, 7, 32, False),
    "tspn_stem_pool_bf16": lambda tspn, dev: case_stem(tspn, dev, 1, 7, 7, 32, True),
}


def test_every_row_of_the_table_has_a_refusal_case():
    import workspace_contracts
    assert set(ENTRY_CASES) == {r["entry"] for r in workspace_contracts.ROWS}


@pytest.mark.parametrize("entry", sorted(ENTRY_CASES))
def test_a_short_or_null_workspace_is_refused_untouched(tspn, device, entry):
    """A real device buffer of `need` bytes reported as need - 1: TSPN_EWORKSPACE, the sentinel-filled outputs and the
    0xFF workspace unchanged; a null workspace is refused as well.  (The span relations entries get their outputs through
    `out=` without a guard band: their sentinels are checked by the bit-equality cases above.)"""
    run, a, _, _ = ENTRY_CASES[entry](tspn, device)
    refused_untouched(tspn, entry, run, a)


def test_wrappers_with_a_workspace_argument_refuse_a_short_one(tspn, device):
    """The wrappers that take `workspace=` answer a short one themselves (ValueError), before the library is called."""
    ops = tspn.ops
    run, a, _, _ = case_conv3_wino63(tspn, device, 3, 7, 32, 256)
    x, w, b = (t(v).to(device) for v in a)
    need = tspn._abi.lib().tspn_conv3_tc_wino63_workspace_bytes(3, 7, 32)
    buf, view = wsc.guarded_ws(need, device, "ones")
    with pytest.raises(ValueError):
        ops.conv3_tc_wino63(x, ops.pack_conv3_wino63(w), b, workspace=view[:need - 1])
    torch.cuda.synchronize(device)
    wsc.assert_all_ones(view, "conv3_tc_wino63(workspace=need - 1)")
    y = ops.conv3_tc_wino63(x, ops.pack_conv3_wino63(w), b, workspace=view)        # exactly need bytes: served
    torch.cuda.synchronize(device)
    wsc.assert_guards_intact(buf, "conv3_tc_wino63(workspace=need)")
    np.testing.assert_allclose(y.cpu().numpy(), t_w63.conv_ref(*a, False), rtol=0, atol=6e-5)


# ------------------------------------------------------------------------------------------------ the model
VIDEOS = {"A": (9, 34, 64), "B": (5, 31, 64), "C": (9, 7, 64)}        # (N, T, D)
MODEL_TABLES = {"A": [[0, 1], [4, 2], [0, 1], [8, 0], [4, 2], [3, 3], [1, 0]], "B": [[4, 3], [0, 3], [3, 4], [2, 0]],
                "C": [[8, 8], [0, 7], [7, 0], [0, 7], [5, 6]]}


def _contract_model(tspn, device, path):
    over = {"RELPN.USE_PPN": True, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 128, "PREDICT.FEATURE_DIM": 128}
    if path == "direct":
        over["RELPN.DPN.CONV_ALGO"] = "direct"
    model = tspn.BaseModel(cases.baseline_cfg(**over))
    sd = tspn.synth.make_weights(0, c=128, bias_std=0.05)
    own = model.state_dict()
    model.load_state_dict({k: t(v) for k, v in sd.items() if k in own})
    model = model.eval().to(device)
    if path == "f16x3":
        model.conv_promoted = True          # what CONV_F16X3_AFTER clean guard readings switch on (D % 128 == 0 there)
    return model


def _model_need(tspn, path):
    ops, need = tspn.ops, 0
    for name, (n, tt, d) in VIDEOS.items():
        if path.startswith("bf16"):
            P = len(MODEL_TABLES[name]) if path == "bf16_pairs" else n * (n - 1)
            need = max(need, ops.fused_bf16_workspace_bytes(1, n, tt, d, A, 132, P, canonical_pairs=path == "bf16"))
        else:
            algo = tspn._abi.CONV_WINOGRAD63_F16X3 if path == "f16x3" else 0
            need = max(need, ops.fused_workspace_bytes(1, n, tt, d, A, 132, n * (n - 1), conv_algo=algo))
    return need


@pytest.mark.parametrize("path", ["direct", "wino63", "f16x3", "bf16", "bf16_pairs"])
def test_model_workspace_reused_across_videos(tspn, device, path):
    """One BaseModel in eval mode keeps one workspace per (device, stream) and scores every later video in it.  Here that
    buffer starts as 0xFF (between guard bands, exactly as large as the largest video needs) and serves A (N = 9, T = 34),
    B (N = 5, T = 31), C (N = 9, T = 7), then A, C, B: each layout finds what another layout left.  Every output of every
    call equals, bit for bit, the same video scored by a fresh model whose workspace was zero-filled."""
    need = _model_need(tspn, path)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)

    def plist(name):
        n, tt, d = VIDEOS[name]
        v = tspn.synth.make_video(400 + ord(name), n, tt, d)
        f = t(v["tracklet_feats"]).to(device)
        kw = {}
        if path.startswith("bf16"):
            f = f.to(torch.bfloat16)
        if path == "bf16_pairs":
            kw["tracklet_pairs"] = torch.tensor(MODEL_TABLES[name], dtype=torch.int64)
        return [tspn.PairList.from_tracklets(f, t(v["tracklet_boxes"]).to(device), t(v["track_cls_logits"]).to(device), **kw)]

    def score(model, name):
        _, dp, lg = model(plist(name), None)
        torch.cuda.synchronize(device)
        return dp[0].heads.clone(), lg[0].clone()

    want = {}
    for name in VIDEOS:
        fresh = _contract_model(tspn, device, path)
        zbuf, zview = wsc.guarded_ws(need, device, "zero")
        fresh._workspaces[key] = zview
        want[name] = score(fresh, name)
        wsc.assert_guards_intact(zbuf, f"fresh model, video {name}")
        assert not bool(torch.isnan(want[name][0]).any()) and not bool(torch.isnan(want[name][1]).any())
    model = _contract_model(tspn, device, path)
    buf, view = wsc.guarded_ws(need, device, "ones")
    model._workspaces[key] = view
    for k, name in enumerate("ABCACB"):
        heads, logits = score(model, name)
        assert model._workspaces[key].data_ptr() == view.data_ptr(), "the model replaced its workspace: `need` is not the largest"
        wsc.assert_guards_intact(buf, f"call {k} (video {name})")
        assert wsc.same_bits(heads, want[name][0]), f"call {k} (video {name}): the heads depend on what the workspace held"
        assert wsc.same_bits(logits, want[name][1]), f"call {k} (video {name}): the logits depend on what the workspace held"
    if path in ("wino63", "f16x3"):
        assert not model.conv_fallback


# ------------------------------------------------------------------------------------------------ the split buffer
def case_heads_pairgrid_f16x3(tspn, device, B, N, C, T, H):
    """tspn_heads_pairgrid_f16x3's `split_buf` (workspace_contracts.OTHER_SCRATCH: not a `void* workspace`, the same
    contract).  tests/test_gpu_pair_stage_f16x3_bound.py's `unit` distribution, reference and relative bound
    (tests/pairf16_reference.py).  The stale run's weights hold an Inf: it leaves a raised flag word behind."""
    ldt = (T + 3) // 4 * 4
    a = pfref.make_case(tspn.hashrng, "unit", B, N, C, T, H, seed=75)
    b = pfref.make_case(tspn.hashrng, "unit", B, N, C, T, H, seed=76)
    b[1][H // 2, C - 1] = np.inf

    def run(inp, helds):
        y, w, bias = inp
        yp = torch.full((B * N, 2 * C, ldt), float("nan"))
        yp[:, :, :T] = t(y)
        ho = sb.held((B * N * (N - 1), H, T), device)
        helds.append((*ho, None))
        return (tspn.ops.heads_pairgrid_f16x3(yp.to(device), B, N, t(w).to(device), t(bias).to(device), T=T, out=ho[1]),)

    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        chain = run(a, [])[0].cpu()                                   # outside the guarded runs
    finally:
        tspn.ops.heads_pairgrid_f16x3_set_force_exact(prev)

    def check(outs):
        got = outs[0].cpu()
        act = pfref.activations(a[0], B, N)
        err = np.abs(got.numpy().astype(np.float64) - pfref.ref64(act, a[1], a[2]))
        assert bool((err <= pfref.bound(act, a[1], a[2])).all()), "heads_pairgrid_f16x3 misses its relative bound"
        assert not wsc.same_bits(got, chain), "the MFMA path did not run"
    return run, a, b, check


@pytest.mark.parametrize("B,N,C,T,H", [(2, 9, 64, 30, 12), (1, 17, 96, 36, 5), (1, 3, 32, 4, 16)])
def test_heads_pairgrid_f16x3_split_buf(tspn, device, B, N, C, T, H):
    """One, two and three k-steps; H = 5 and 16: rows H .. 15 of the weight fragments are the pack kernel's to zero."""
    need = tspn.ops.heads_pairgrid_f16x3_split_bytes(C, H)
    assert need == 256 + C // 32 * 2048
    hold(tspn, f"heads_pairgrid_f16x3 {(B, N, C, T, H)}", *case_heads_pairgrid_f16x3(tspn, device, B, N, C, T, H))


def test_heads_pairgrid_f16x3_refuses_a_short_null_or_misaligned_split_buf(tspn, device):
    """need - 1 bytes: TSPN_EWORKSPACE; no buffer: TSPN_EINVAL; a buffer 8 bytes off a 16-byte boundary: TSPN_EINVAL.
    Each before any device work: the sentinel-filled output and the 0xFF buffer keep every byte."""
    E = tspn._abi
    B, N, C, T, H = 2, 9, 64, 30, 12
    run, a, _, _ = case_heads_pairgrid_f16x3(tspn, device, B, N, C, T, H)
    refused_untouched(tspn, "tspn_heads_pairgrid_f16x3", run, a)
    need = tspn.ops.heads_pairgrid_f16x3_split_bytes(C, H)
    buf, view = wsc.guarded_ws(need + 16, device, "ones")
    y, w, bias = a
    yp = torch.zeros((B * N, 2 * C, 32))
    yp[:, :, :T] = t(y)
    hbuf, out = sb.held((B * N * (N - 1), H, T), device)
    with pytest.raises(E.TspnError) as e:
        tspn.ops.heads_pairgrid_f16x3(yp.to(device), B, N, t(w).to(device), t(bias).to(device), T=T, split_buf=view[8:8 + need],
                                      out=out)
    assert e.value.code == E.TSPN_EINVAL, e.value
    torch.cuda.synchronize(device)
    sb.assert_untouched(hbuf, "misaligned split_buf")
    wsc.assert_all_ones(view, "misaligned split_buf")
    wsc.assert_guards_intact(buf, "misaligned split_buf")


@pytest.mark.parametrize("first,second", [("inf_weight", "clean"), ("H=12", "H=5"), ("C=96", "C=32")])
def test_heads_pairgrid_f16x3_split_buf_carries_no_state(tspn, device, first, second):
    """One caller-held buffer (0xFF at first) serves two calls: flagged weights and then clean ones (the flag word must be
    rewritten), H = 12 and then H = 5 (rows 5 .. 15 of the fragments must be zeroed again), C = 96 and then C = 32 (the
    k-steps past the first hold the other call's fragments).  The second call equals, bit for bit, the same call on a
    fresh zeroed buffer, and it ran on MFMAs."""
    B, N, T = 2, 9, 30
    shape = {"inf_weight": (64, 12), "clean": (64, 12), "H=12": (64, 12), "H=5": (64, 5), "C=96": (96, 12), "C=32": (32, 12)}

    def operands(name, seed):
        C, H = shape[name]
        y, w, b = pfref.make_case(tspn.hashrng, "unit", B, N, C, T, H, seed=seed)
        if name == "inf_weight":
            w[3, 17] = np.inf
        return y, w, b

    def call(inp, view):
        y, w, b = inp
        yp = torch.full((B * N, y.shape[1], 32), float("nan"))
        yp[:, :, :T] = t(y)
        hbuf, out = sb.held((B * N * (N - 1), w.shape[0], T), device)
        tspn.ops.heads_pairgrid_f16x3(yp.to(device), B, N, t(w).to(device), t(b).to(device), T=T, split_buf=view, out=out)
        sb.assert_written_inside_only(hbuf, out, f"{first} -> {second}")
        return out.clone()

    need = max(tspn.ops.heads_pairgrid_f16x3_split_bytes(*shape[n]) for n in (first, second))
    buf, view = wsc.guarded_ws(need, device, "ones")
    one, two = operands(first, 77), operands(second, 78)
    call(one, view)
    got = call(two, view)
    wsc.assert_guards_intact(buf, f"{first} -> {second}")
    # what the second call left: no flag, a zero header tail, and zero rows H .. 15 in every fragment (the MFMA computes
    # those rows too; no output shows them, so the buffer is the only place to see that the pack kernel wrote them)
    C_, H_ = shape[second]
    raw = view[:256 + C_ // 32 * 2048].cpu()
    hdr = raw[:256].view(torch.int32)
    assert int(hdr[0]) == 0 and bool((hdr[17:] == 0).all()), "the flag word or the header's tail was not rewritten"
    frag = raw[256:].view(C_ // 32, 2, 64, 16)           # [k-step][hi | lo][lane][16 bytes], head row = lane & 15
    assert bool((frag[:, :, torch.arange(64) % 16 >= H_] == 0).all()), "rows H .. 15 of the weight fragments are not zero"
    assert bool((frag[:, 0, torch.arange(64) % 16 < H_] != 0).any())
    zbuf, zview = wsc.guarded_ws(tspn.ops.heads_pairgrid_f16x3_split_bytes(*shape[second]), device, "zero")
    want = call(two, zview)
    wsc.assert_guards_intact(zbuf, f"{second} on a zeroed buffer")
    assert wsc.same_bits(got, want), f"{second} after {first}: the output depends on what the split buffer held"
    prev = tspn.ops.heads_pairgrid_f16x3_set_force_exact(1)
    try:
        chain = call(two, zview)
    finally:
        tspn.ops.heads_pairgrid_f16x3_set_force_exact(prev)
    assert not wsc.same_bits(got, chain), f"{second} after {first}: the MFMA path did not run"
    act = pfref.activations(two[0], B, N)
    err = np.abs(got.cpu().numpy().astype(np.float64) - pfref.ref64(act, two[1], two[2]))
    assert bool((err <= pfref.bound(act, two[1], two[2])).all())


# ------------------------------------------------------------------------------------------------ caller-zeroed scratch
def test_caller_zeroed_scratch_is_not_overrun(tspn, device):
    """det_ws of tspn_eval_greedy_match_f64 and the scratch of the stand-alone tspn_conv3_spot_check_f32 are zeroed by the
    caller (header): no "any contents" here, but their exact sizes between guard bands."""
    ops, E = tspn.ops, tspn._abi
    # one group of 4200 ground truths (above the 4096 of the register form) and a small one behind it
    rs = np.random.RandomState(5)
    groups = np.array([[0, 5, 7, 4200, 0], [5, 2, 4207, 3, 5 * 4200]], dtype=np.int64)
    ov = rs.uniform(0, 1, size=5 * 4200 + 2 * 3)
    buf, det = wsc.guarded_ws(7 + 4200 + 3, device, "zero")
    hit, match = ops.eval_greedy_match(t(ov).to(device), t(groups).to(device), 7, 0.5, 4200, det_ws=det)
    torch.cuda.synchronize(device)
    wsc.assert_guards_intact(buf, "eval_greedy_match det_ws")
    for p0, npred, gt0, ngt, off in groups:
        done = np.zeros(ngt, dtype=bool)
        for q in range(npred):
            row = np.where(done | (ov[off + q * ngt:off + (q + 1) * ngt] < 0.5), -1.0, ov[off + q * ngt:off + (q + 1) * ngt])
            best = int(row.argmax()) if row.max() >= 0.5 else -1
            if best >= 0:
                done[best] = True
            assert int(match[p0 + q]) == best and int(hit[p0 + q]) == (1 if best >= 0 else 0)
        # the flags of a group of up to 4096 ground truths stay in a register: its bytes of det_ws are not touched
        assert np.array_equal(det.cpu().numpy()[gt0:gt0 + ngt] != 0, done if ngt > 4096 else np.zeros(ngt, dtype=bool))
    # the spot check on its own scratch
    B, T, Cin, M = 3, 7, 32, 32
    x = t(tspn.hashrng.uniform(91, "x", (B, T, Cin), -1, 1)).to(device)
    w = t(tspn.hashrng.normal(91, "w", (M, Cin, 3), std=0.2)).to(device)
    y = ops.conv3_tc_wino63(x, ops.pack_conv3_wino63(w), None)
    words = ops.status_words(device)
    words[E.STATUS_CONV_ERR] = 0
    words[E.STATUS_CONV_CHECKS] = 0
    sbuf, scratch = wsc.guarded_ws(E.CONV_CHECK_SCRATCH_BYTES, device, "zero")
    p = ops._p
    E.check(E.lib().tspn_conv3_spot_check_f32(p(x), B, T, Cin, p(w), M, Cin, 0, None, 0, p(y), T, p(scratch), 64, ops._stream()))
    torch.cuda.synchronize(device)
    wsc.assert_guards_intact(sbuf, "conv3_spot_check scratch")
    assert bool((scratch[:32] == 0).all()) and 64 * 4 <= int(words[E.STATUS_CONV_CHECKS]) <= 64 * 24
    assert float(words[E.STATUS_CONV_ERR:E.STATUS_CONV_ERR + 1].view(np.float32)[0]) < 1e-4
    words[E.STATUS_CONV_ERR] = 0
    words[E.STATUS_CONV_CHECKS] = 0
