"""Every kernel variant a launcher can pick, at the edges of its tiles, against a float64 reference on the CPU.

The launchers choose among compiled variants by shape AND by pointer alignment (tests/kernel_variants.py lists
each variant, the condition that selects it and the tests that reach it).  Torch allocations are 256-byte aligned,
so the "unaligned" variants are reached here through views at a one-element storage offset (`off4`): a fast shape
paired with an unaligned pointer.  Tolerances are the suite's: 2e-5 absolute for fp32 convs and heads, 3e-5 for
bf16 operands against the rounded operands, bit-exact for gathers and means."""
import ctypes

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DPN_PRE = "relpn.duration_proposal_network.dpn_head."


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def off4(x, device):
    """A contiguous device copy of `x` whose storage starts 4 bytes past a 256-byte aligned block."""
    x = x.to(device)
    buf = torch.zeros(x.numel() + 1, dtype=x.dtype, device=device)
    buf[1:] = x.flatten()
    v = buf[1:].view(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)


# ------------------------------------------------------------------------------------------------- conv3
def conv_ref(x, w, b, relu):
    y = torch.nn.functional.conv1d(t(x).double(), t(w).double(), None if b is None else t(b).double(), padding=1)
    return (torch.relu(y) if relu else y).float().numpy()


def conv3_variant(Cin, M, packed):
    """tspn_conv3_f32's choice (tspn_conv3.hip), restated."""
    vec = M % 4 == 0 and packed.data_ptr() % 16 == 0
    if vec and Cin % 8 == 0:
        return "dma8" if Cin % 16 else "dma16"
    return "vec" if vec else "scalar"


# (variant, Cin values): one chunk and three chunks of the variant's K chunk (a partial last chunk where the
# kernel has one); "scalar" is selected by alignment alone (M % 4 == 0, packed weights at a 4-byte offset)
CONV3_VARIANTS = [("dma16", (16, 48)), ("dma8", (8, 24)), ("vec", (12, 37)), ("scalar", (16, 37))]
# (B, T): B*T < BN = 128; B*T = BN +- 1 and BN - 2 with T not dividing 128 (tiles span sequences); T in {1, 2}
CONV3_BT = [(5, 1), (3, 2), (65, 2), (43, 3), (1, 127), (18, 7)]


@pytest.mark.parametrize("variant,cins", CONV3_VARIANTS)
@pytest.mark.parametrize("B,T", CONV3_BT)
@pytest.mark.parametrize("M", [4, 132])
def test_conv3_every_variant_at_tile_edges(tspn, device, variant, cins, B, T, M):
    for Cin in cins:
        x = tspn.hashrng.uniform(401, f"x{Cin}", (B, Cin, T), -1, 1)
        w = tspn.hashrng.normal(401, f"w{Cin}", (M, Cin, 3), std=0.1)
        b = tspn.hashrng.normal(401, f"b{Cin}", (M,), std=0.1)
        packed = tspn.ops.pack_conv3(t(w).to(device))
        if variant == "scalar":
            packed = off4(packed, device)
        assert conv3_variant(Cin, M, packed) == variant
        for xd in (t(x).to(device), off4(t(x), device)):   # the DMA kernels read x 4 bytes at a time
            for relu in (False, True):
                for bias in (b, None):
                    y = tspn.ops.conv3(xd, packed, None if bias is None else t(bias).to(device), relu=relu)
                    np.testing.assert_allclose(y.cpu().numpy(), conv_ref(x, w, bias, relu), rtol=0, atol=2e-5,
                                               err_msg=f"{variant} Cin={Cin} relu={relu} bias={bias is not None}")


def test_conv3_mfma_dma_kernel_8_bias_and_tail(tspn, device):
    """Regression case for conv3_mfma_dma_kernel<8>: Cin % 16 == 8 over several 128 x 128 tiles in both
    directions (M tail, sequences across column tiles), bias and ReLU in the epilogue."""
    B, Cin, T, M = 29, 40, 9, 260
    x = tspn.hashrng.uniform(402, "x", (B, Cin, T), -1, 1)
    w = tspn.hashrng.normal(402, "w", (M, Cin, 3), std=0.1)
    b = tspn.hashrng.normal(402, "b", (M,), std=0.5)
    packed = tspn.ops.pack_conv3(t(w).to(device))
    assert conv3_variant(Cin, M, packed) == "dma8"
    for relu in (False, True):
        y = tspn.ops.conv3(t(x).to(device), packed, t(b).to(device), relu=relu)
        np.testing.assert_allclose(y.cpu().numpy(), conv_ref(x, w, b, relu), rtol=0, atol=2e-5)


def test_conv3_channels_last_refuses_unaligned(tspn, device):
    """tspn_conv3_tc_f32 stages x and the weights in 16-byte pieces: a view at a 4-byte offset is refused."""
    x = torch.zeros(2, 5, 16, device=device)
    packed = tspn.ops.pack_conv3(torch.zeros(8, 16, 3, device=device))
    for xx, pk in ((off4(x, device), packed), (x, off4(packed, device))):
        with pytest.raises(tspn._abi.TspnError) as e:
            tspn.ops.conv3_tc(xx, pk)
        assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED


# ------------------------------------------------------------------------------------------- heads_kernel
def heads_raw(tspn, mode, a, b, ia, ib, bias, wh, bh, out):
    """tspn_heads_f32 with a caller-held `out` (ops.heads allocates its own, always aligned)."""
    P, H, T = out.shape
    lda, C = a.shape[1], wh.shape[1]
    tspn._abi.check(tspn._abi.lib().tspn_heads_f32(mode, p(a), p(b), lda, p(ia), p(ib), 1, p(bias), p(wh), p(bh),
                                                   H, P, C, T, p(out), tspn.ops._stream()))
    return out


@pytest.mark.parametrize("H", [1, 12, 16])
@pytest.mark.parametrize("T", [2, 31, 32, 33, 34])
@pytest.mark.parametrize("P", [1, 3, 5, 9])
def test_heads_kernel_both_modes_vec2_and_scalar(tspn, device, P, T, H):
    """heads_kernel<mode, vec2>: P around NP = 4 pairs per wave, T around TB = 32 frames; even T selects the
    vec2 form, and a, b or out at a 4-byte offset selects the scalar form at the same shape.  Index tables
    repeat rows and include ia == ib."""
    C, R = 21, max(P // 2, 1)
    a = tspn.hashrng.uniform(410, "a", (R, C, T), -1, 1)
    b = tspn.hashrng.uniform(410, "b", (R, C, T), -1, 1)
    wh = tspn.hashrng.normal(410, "wh", (H, C), std=0.1)
    bh = tspn.hashrng.normal(410, "bh", (H,), std=0.1)
    bias = tspn.hashrng.normal(410, "bias", (C,), std=0.3)
    ia = tspn.hashrng.integers(410, "ia", (P,), 0, R)
    ib = tspn.hashrng.integers(410, "ib", (P,), 0, R)
    ib[0] = ia[0]
    wd, bhd, biasd = t(wh).to(device), t(bh).to(device), t(bias).to(device)
    iad, ibd = t(ia).to(device), t(ib).to(device)
    ref0 = (torch.einsum("hc,pct->pht", t(wh).double(), t(a).double()[ia]) + t(bh).double().view(1, -1, 1)).float()
    hh = torch.relu(t(a).double()[ia] + t(b).double()[ib] + t(bias).double().view(1, -1, 1))
    ref1 = (torch.einsum("hc,pct->pht", t(wh).double(), hh) + t(bh).double().view(1, -1, 1)).float()
    aligned = lambda v: t(v).to(device)
    unaligned = lambda v: off4(t(v), device)
    forms = [(aligned, aligned, aligned), (unaligned, aligned, aligned), (aligned, unaligned, aligned),
             (aligned, aligned, unaligned)]
    for fa, fb, fo in forms:
        out_shape = torch.zeros((P, H, T))
        out0 = heads_raw(tspn, 0, fa(a), None, iad, None, None, wd, bhd, fo(out_shape))
        np.testing.assert_allclose(out0.cpu().numpy(), ref0.numpy(), rtol=0, atol=2e-5)
        out1 = heads_raw(tspn, 1, fa(a), fb(b), iad, ibd, biasd, wd, bhd, fo(out_shape))
        np.testing.assert_allclose(out1.cpu().numpy(), ref1.numpy(), rtol=0, atol=2e-5)


# ---------------------------------------------------------------------------------------- fp32 pair grid
def pairgrid_ref(y, B, N, wh, bh):
    C = y.shape[1] // 2
    yy = t(y).double()
    pairs = torch.cat([oracle.pair_index(N) + b * N for b in range(B)])
    h = torch.relu(yy[pairs[:, 0], :C] + yy[pairs[:, 1], C:])
    return (torch.einsum("hc,pct->pht", t(wh).double(), h) + t(bh).double().view(1, -1, 1)).float().numpy()


def pairgrid_variant(C, T, y, out):
    """tspn_heads_pairgrid_f32's choice with ldt == T (tspn_heads.hip), restated."""
    if T % 4 == 0 and C % 16 == 0 and y.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0:
        return "v3"
    return "vec2" if T % 2 == 0 and y.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0 else "scalar"


@pytest.mark.parametrize("C", [16, 24, 48])
@pytest.mark.parametrize("T", [2, 32, 33, 34, 150])
@pytest.mark.parametrize("N", [2, 8, 9, 17])
def test_heads_pairgrid_every_variant(tspn, device, N, T, C):
    """heads_pairgrid3_kernel (T % 4 == 0, C % 16 == 0), heads_pairgrid_kernel<true> (even T, or C % 16 != 0)
    and <false> (odd T; and even T with y at a 4-byte offset) on the canonical pair table of two videos."""
    B, H = 2, 12
    y = tspn.hashrng.uniform(420, "y", (B * N, 2 * C, T), -1, 1)
    wh = tspn.hashrng.normal(420, "wh", (H, C), std=0.1)
    bh = tspn.hashrng.normal(420, "bh", (H,), std=0.1)
    ref = pairgrid_ref(y, B, N, wh, bh)
    seen = set()
    for yd in (t(y).to(device), off4(t(y), device)):
        out = tspn.ops.heads_pairgrid(yd, B, N, t(wh).to(device), t(bh).to(device))
        seen.add(pairgrid_variant(C, T, yd, out))
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=2e-5)
    assert "scalar" in seen


# -------------------------------------------------------------------------------------- forward_fused fp32
def fused_weights(tspn, D, A):
    sd = tspn.synth.make_weights(7, c=2 * D, a=A, k=37, bias_std=0.05)
    return {"conv_w": t(sd[DPN_PRE + "conv.weight"]), "conv_b": t(sd[DPN_PRE + "conv.bias"]),
            "dur_w": t(sd[DPN_PRE + "duration_pred.weight"]), "dur_b": t(sd[DPN_PRE + "duration_pred.bias"]),
            "rel_w": t(sd[DPN_PRE + "relness_pred.weight"]), "rel_b": t(sd[DPN_PRE + "relness_pred.bias"]),
            "cls_w": t(sd["classifier.rel_predictor.weight"]), "cls_b": t(sd["classifier.rel_predictor.bias"])}


@pytest.mark.parametrize("D,T,A,canonical,aligned", [
    (16, 30, 4, True, True),     # channels-last conv, ldy = 32 (T % 4 == 2), pairgrid4<8>
    (16, 32, 4, True, True),     # ldy = T, pairgrid4<8>
    (16, 33, 4, True, True),     # odd T: ldy = T, heads_pairgrid_kernel<false>
    (32, 150, 5, True, True),    # ldy = 152, H = 15: heads_pairgrid3_kernel
    (16, 34, 4, False, True),    # indexed pair stage, heads_kernel<1, true>
    (16, 30, 4, True, False),    # feats at an offset: transpose + conv3_mfma_dma_kernel<16>, ldy = T, pairgrid<true>
    (24, 30, 4, True, True),     # D % 16 == 8: transpose + conv3_mfma_dma_kernel<8>
    (24, 32, 4, True, True),     # D % 16 == 8, T % 4 == 0: transpose + dma<8>, heads_pairgrid4_kernel<8>
    (8, 33, 4, False, True),     # D % 16 == 8, odd T: dma<8>, heads_kernel<1, false>
    (20, 30, 4, True, True),     # D % 8 != 0: transpose + conv3_mfma_kernel<true>
])
def test_forward_fused_conv_and_pair_paths(tspn, device, D, T, A, canonical, aligned):
    """The fused fp32 pass on each of its conv paths (channels-last / transpose + direct) and pair stages
    (padded ldy or not), against the dense float64-faithful oracle; the logits go through the split-K GEMM's
    column-half form (ldw = 2D > F = D)."""
    B, N = 2, 9
    w = fused_weights(tspn, D, A)
    vids = [tspn.synth.make_video(60 + b, N, T, D) for b in range(B)]
    feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
    pairs = torch.cat([oracle.pair_index(N) + b * N for b in range(B)])
    d = lambda v: v.to(device).contiguous()
    packed = tspn.ops.pack_conv3(d(w["conv_w"]), split=D)
    hw = d(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]))
    hb = d(torch.cat([w["rel_b"], w["dur_b"]]))
    fd = d(feats) if aligned else off4(feats, device)
    heads, logits = tspn.ops.forward_fused(fd, d(pairs), B, N, packed, d(w["conv_b"]), hw, hb, d(w["cls_w"]),
                                           d(w["cls_b"]), canonical_pairs=canonical)
    for b in range(B):
        ref = oracle.forward_dense(t(vids[b]["tracklet_feats"]).double(), t(vids[b]["tracklet_boxes"]).double(),
                                   oracle.pair_index(N), {k: v.double() for k, v in w.items()})
        sl = slice(b * N * (N - 1), (b + 1) * N * (N - 1))
        np.testing.assert_allclose(heads[sl, :A].cpu().numpy(), ref["relness"].numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(heads[sl, A:].cpu().numpy(), ref["duration"].numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(logits[sl].cpu().numpy(), ref["rel_logits"].numpy(), rtol=0, atol=2e-5)


# ---------------------------------------------------------------------------------------- bf16 pair grid
def heads_bf16_ref64(y, B, N, hw, hb):
    C = y.shape[2] // 2
    out = []
    for b in range(B):
        yy = y[b * N:(b + 1) * N]
        pairs = oracle.pair_index(N)
        a = torch.relu(yy[pairs[:, 0], :, :C] + yy[pairs[:, 1], :, C:]).to(torch.bfloat16).double()
        out.append(torch.einsum("ptc,hc->pht", a, hw.double()) + hb.double().view(1, -1, 1))
    return torch.cat(out)


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("T", [1, 16, 17])
@pytest.mark.parametrize("N", [12, 13, 16, 17, 33])
def test_heads_pairgrid_bf16_small_and_big(tspn, device, N, T, C):
    """heads_pairgrid_bf16_kernel<4, 8, 2> (N <= 12) and <8, 16, SW> (N > 12), T around HP_FB = 16, B = 2;
    y at a 4-byte offset is refused."""
    B = 2
    y = t(tspn.hashrng.normal(430, "y", (B * N, T, 2 * C), std=1.0))
    hw = t(tspn.hashrng.normal(430, "hw", (12, C), std=0.1)).to(torch.bfloat16).float()
    hb = t(tspn.hashrng.normal(430, "hb", (12,), std=0.1))
    hp = tspn.ops.pack_heads_bf16(hw.to(device))
    out = tspn.ops.heads_pairgrid_bf16(y.to(device), B, N, hp, hb.to(device), 12)
    np.testing.assert_allclose(out.cpu().numpy(), heads_bf16_ref64(y, B, N, hw, hb).numpy(), rtol=0, atol=3e-5)
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn.ops.heads_pairgrid_bf16(off4(y, device), B, N, hp, hb.to(device), 12)
    assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED


# --------------------------------------------------------------------------------- gathers and means
@pytest.mark.parametrize("T", [160, 161])
def test_pair_gather_rows_form_and_32x32_form(tspn, device, T):
    """transpose_gather_rows_kernel (D % 64 == 0, T <= TG_TMAX = 160, 16-byte aligned) and transpose_gather_kernel
    (T = 161, or feats at a 4-byte offset): bit-exact.  Boxes at an offset are refused."""
    N, D = 5, 64
    f = tspn.hashrng.uniform(440, "f", (N, T, D), -1, 1)
    bx = tspn.hashrng.uniform(440, "bx", (N, T, 4), 0, 100)
    pairs = oracle.pair_index(N)
    want = np.concatenate([f[pairs[:, 0]], f[pairs[:, 1]]], axis=2).transpose(0, 2, 1)
    for fd in (t(f).to(device), off4(t(f), device)):
        got, _ = tspn.ops.pair_gather(fd, None, pairs.to(device), want_geom=False)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn.ops.pair_gather(t(f).to(device), off4(t(bx), device), pairs.to(device))
    assert e.value.code == tspn._abi.TSPN_EINVAL


@pytest.mark.parametrize("R,T,D", [(3, 7, 8), (5, 150, 64), (2, 1, 4), (4, 33, 132)])
def test_temporal_mean_td4_td_ct_by_alignment(tspn, device, R, T, D):
    """temporal_mean_td4_kernel (D % 4 == 0, 16-byte aligned) vs temporal_mean_td_kernel (the same values at a
    4-byte offset): bit for bit; temporal_mean_ct_kernel on the transposed layout, aligned or not, bit for bit."""
    x = tspn.hashrng.uniform(450, "x", (R, T, D), -1, 3)
    a = tspn.ops.temporal_mean(t(x).to(device), layout_tc=True)
    b = tspn.ops.temporal_mean(off4(t(x), device), layout_tc=True)
    assert torch.equal(a, b)
    np.testing.assert_allclose(a.cpu().numpy(), x.astype(np.float64).mean(axis=1), rtol=0, atol=2e-6)
    xc = np.ascontiguousarray(x.transpose(0, 2, 1))
    c1 = tspn.ops.temporal_mean(t(xc).to(device), layout_tc=False)
    c2 = tspn.ops.temporal_mean(off4(t(xc), device), layout_tc=False)
    assert torch.equal(c1, c2)
    np.testing.assert_allclose(c1.cpu().numpy(), x.astype(np.float64).mean(axis=1), rtol=0, atol=2e-6)


@pytest.mark.parametrize("F", [2, 64, 1001, 1030])
def test_gather_rows_v2_and_scalar_by_alignment(tspn, device, F):
    """gather_rows_kernel<float2> (even F, 8-byte aligned) and <float> (odd F, or src at a 4-byte offset): bit-exact."""
    src = tspn.hashrng.uniform(460, "src", (37, F), -1, 1)
    idx = tspn.hashrng.integers(460, "idx", (50,), 0, 37)
    for sd in (t(src).to(device), off4(t(src), device)):
        got = tspn.ops.gather_rows(sd, t(idx).to(device))
        np.testing.assert_array_equal(got.cpu().numpy(), src[idx])


# ---------------------------------------------------------------------------------------- split-K GEMM
def splits_of(P, F, K):
    """choose_splits of tspn_linear.hip, restated."""
    tiles = -(-P // 64) * -(-K // 144)
    return max(min(-(-512 // tiles), max(1, F // 64), 64), 1)


@pytest.mark.parametrize("P,F,K,splits", [
    (10944, 40, 289, 1),     # 513 tiles: one split; P*K > 2^20: the reduce loop strides; three column tiles + 1
    (5, 4500, 10, 64),       # one tile: 64 splits
    (70, 63, 17, 1),         # F < 64
    (9, 129, 144, 2),        # F = 32*4 + 1
    (9, 127, 145, 1),        # F = 32*4 - 1, two column tiles
    (3, 2047, 289, 31),      # F = 32*64 - 1
    (130, 289, 5, 4),        # K < 16, three row tiles
])
def test_predicate_head_split_k_edges(tspn, device, P, F, K, splits):
    assert splits_of(P, F, K) == splits
    x = tspn.hashrng.uniform(470, "x", (P, F), -1.0, 1.0)
    w = tspn.hashrng.normal(470, "w", (K, F), std=0.05)
    b = tspn.hashrng.normal(470, "b", (K,), std=0.1)
    xd, wd = t(x).to(device), t(w).to(device)
    raw = tspn.ops.predicate_head(xd, wd, None, apply_sigmoid=False)
    ref_raw = (t(x).double() @ t(w).double().t()).float().numpy()
    np.testing.assert_allclose(raw.cpu().numpy(), ref_raw, rtol=0, atol=2e-5)
    out = tspn.ops.predicate_head(xd, wd, t(b).to(device))
    ref = oracle.predicate_head(t(x).double(), t(w).double(), t(b).double()).float().numpy()
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=5e-6)
    # operands at a 4-byte offset: the split-K kernel reads them one float at a time
    out_u = tspn.ops.predicate_head(off4(t(x), device), off4(t(w), device), t(b).to(device))
    np.testing.assert_allclose(out_u.cpu().numpy(), ref, rtol=0, atol=5e-6)


def test_predicate_head_norm_table_over_64_slices(tspn, device):
    """linear_splitk_kernel<true> + linear_reduce_norm_kernel with 70 normalisation blocks: more than 64 slices."""
    P, K, norm = 33, 21, (3, 40, 70)
    F = norm[0] + norm[1] * norm[2] + 5
    x = tspn.hashrng.uniform(471, "x", (P, F), -1.0, 1.0)
    x[4, norm[0] + norm[1]:norm[0] + 2 * norm[1]] = 0   # a zero block: divides by 1
    w = tspn.hashrng.normal(471, "w", (K, F), std=0.05)
    b = tspn.hashrng.normal(471, "b", (K,), std=0.1)
    assert tspn._abi.lib().tspn_predicate_head_norm_workspace_bytes(P, F, K, *norm) > 64 * P * (K + 1) * 4
    ref = oracle.predicate_head(oracle.feature_preprocess(t(x).double(), *norm), t(w).double(), t(b).double())
    out = tspn.ops.predicate_head(t(x).to(device), t(w).to(device), t(b).to(device), norm=norm)
    np.testing.assert_allclose(out.cpu().numpy(), ref.float().numpy(), rtol=0, atol=5e-6)


# --------------------------------------------------------------------------------------- bf16 conv2d
@pytest.mark.parametrize("NB,H,W,Cin,Cout,k,stride,pad", [
    (2, 7, 7, 320, 128, 1, 1, 0),     # 1x1 with K = Cin > 256, Cout % 64 == 0
    (3, 9, 11, 64, 64, 3, 2, 1),      # strided 3x3, Cout % 64 == 0
])
def test_conv2d_nhwc_bf16_mi2_without_ring(tspn, device, NB, H, W, Cin, Cout, k, stride, pad):
    """conv2d_nhwc_bf16_kernel<2, false>: exact bf16 products, fp32 accumulation vs float64 on the same operands,
    one bf16 rounding of the result."""
    r16 = lambda a: t(a).to(torch.bfloat16)
    x = tspn.hashrng.uniform(480, "x", (NB, H, W, Cin), -1, 1)
    w = tspn.hashrng.normal(480, "w", (Cout, Cin, k, k), std=0.1)
    b = tspn.hashrng.normal(480, "b", (Cout,), std=0.1)
    xb, wb = r16(x), r16(w)
    ref = torch.nn.functional.conv2d(xb.double().permute(0, 3, 1, 2), wb.double(), t(b).double(),
                                     stride=stride, padding=pad).permute(0, 2, 3, 1)
    res = r16(tspn.hashrng.uniform(480, "r", tuple(ref.shape), -1, 1))
    ref = torch.relu(ref + res.double())
    frag = tspn.ops.pack_conv2d_frag_bf16(t(w).to(device))
    y = tspn.ops.conv2d_nhwc_bf16(xb.to(device), frag, (k, k), stride, pad, bias=t(b).to(device),
                                  residual=res.to(device), relu=True)
    got = y.cpu().double()
    tol = ref.abs() * 2.0 ** -8 + 3e-5
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() - tol).max())
