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


@pytest.mark.parametrize("variant,Cin", [("dma16", 32), ("dma8", 8), ("vec", 12), ("scalar", 16), ("cl", 16)])
def test_conv3_tile_map_with_a_short_last_group(tspn, device, variant, Cin):
    """The workgroup-to-tile map of the three kernels of tspn_conv3.hip (BM = BN = 128, GM = 8): M = 9 * 128 rows are two
    groups of weight panels, the second a single panel, and 5 * 43 = 215 columns are two column tiles (the second partial,
    sequences of 43 frames across the tile edge): a grid of 18 workgroups (> 8, 18 % 8 = 2).  Every output element against
    the float64 conv; a tile computed twice or not at all shows as garbage in the freshly allocated output."""
    B, T, M = 5, 43, 9 * 128
    x = tspn.hashrng.uniform(403, f"x{Cin}", (B, Cin, T), -1, 1)
    w = tspn.hashrng.normal(403, f"w{Cin}", (M, Cin, 3), std=0.1)
    b = tspn.hashrng.normal(403, f"b{Cin}", (M,), std=0.1)
    packed = tspn.ops.pack_conv3(t(w).to(device))
    if variant == "cl":
        y = tspn.ops.conv3_tc(t(x).permute(0, 2, 1).contiguous().to(device), packed, t(b).to(device), relu=True)
    else:
        if variant == "scalar":
            packed = off4(packed, device)
        assert conv3_variant(Cin, M, packed) == variant
        y = tspn.ops.conv3(t(x).to(device), packed, t(b).to(device), relu=True)
    assert tuple(y.shape) == (B, M, T)
    np.testing.assert_allclose(y.cpu().numpy(), conv_ref(x, w, b, True), rtol=0, atol=2e-5)


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
    (16, 148, 4, True, True),    # pairgrid4<8> past one round of its map: PG_T = 32 -> 5 frame blocks x 2 videos = 10 groups
                                 # (10 % 8 = 2: the last round has two groups, six XCDs' workgroups return early)
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
@pytest.mark.parametrize("B,N,T,grid", [(3, 12, 33, 36), (3, 8, 49, 12), (1, 33, 17, 18)])
def test_heads_pairgrid_bf16_grids_the_xcd_remap_does_not_divide(tspn, device, B, N, T, grid):
    """heads_pairgrid_bf16_kernel numbers its B x nfb x nsb x nsb workgroups through the XCD remap (HP_FB = 16 frames,
    8 subjects per block for N <= 12, else 16): <4, 8, 2> with 3 * 3 * 2 * 2 = 36 and 3 * 4 * 1 * 1 = 12 workgroups,
    <8, 16, SW> with 1 * 2 * 3 * 3 = 18 -- each larger than 8 and no multiple of 8.  Every element against float64."""
    sblk = 16 if N > 12 else 8
    assert B * -(-T // 16) * (-(-N // sblk)) ** 2 == grid and grid > 8 and grid % 8
    C = 32
    y = t(tspn.hashrng.normal(431, "y", (B * N, T, 2 * C), std=1.0))
    hw = t(tspn.hashrng.normal(431, "hw", (12, C), std=0.1)).to(torch.bfloat16).float()
    hb = t(tspn.hashrng.normal(431, "hb", (12,), std=0.1))
    out = tspn.ops.heads_pairgrid_bf16(y.to(device), B, N, tspn.ops.pack_heads_bf16(hw.to(device)), hb.to(device), 12)
    np.testing.assert_allclose(out.cpu().numpy(), heads_bf16_ref64(y, B, N, hw, hb).numpy(), rtol=0, atol=3e-5)


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


# ------------------------------------------------------------------- split-fp16 F(6,3) (tspn_wino63.hip overloads)
# Against float64 conv1d at the split form's tolerances of tests/test_gpu_wino63_f16x3.py: 6e-5 absolute at these
# magnitudes and 64 eps sum|x||w|.  The output is caller-held and pre-filled: no element may keep the sentinel, and
# the 32 floats in front of and behind it must keep it.
SENTINEL = np.float32(-3.0e33)
F_BM = F_BN = 256     # contraction tile (rows x sextets), GM = 4 row tiles per group, 8 XCDs: tspn_wino63.hip
F_GM = 4


def conv_tc_ref64(x, w):
    """x [B,T,Cin], w [M,Cin,3] -> (conv, sum |x||w|), float64 [B,M,T]."""
    xt, wt = t(x).double().transpose(1, 2), t(w).double()
    return (torch.nn.functional.conv1d(xt, wt, padding=1).numpy(),
            torch.nn.functional.conv1d(xt.abs(), wt.abs(), padding=1).numpy())


def held_output(shape, device, offset=0):
    """(buffer, view): a sentinel-filled buffer and a contiguous view of `shape` 32 + offset floats into it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64 + offset,), float(SENTINEL), dtype=torch.float32, device=device)
    v = buf[32 + offset:32 + offset + n].view(shape)
    assert v.data_ptr() % 8 == (4 if offset % 2 else 0)
    return buf, v


def f16x3_raw(tspn, x, pk, bias, relu, y, ws=None, ws_bytes=None, M=None):
    """tspn_conv3_tc_wino63_f16x3 on a caller-held y (and workspace); raises TspnError on a refusal."""
    B, T, Cin = x.shape
    M = tspn.ops.wino63_f16x3_dims(pk)[1] if M is None else M
    l = tspn._abi.lib()
    if ws is None:
        ws = torch.empty(max(l.tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M), 256), dtype=torch.uint8,
                         device=x.device)
    tspn._abi.check(l.tspn_conv3_tc_wino63_f16x3(p(x), B, T, Cin, p(pk), M, p(bias), 1 if relu else 0, p(y), p(ws),
                                                 ws.numel() if ws_bytes is None else ws_bytes, tspn.ops._stream()))
    return y


def check_f16x3(buf, y, ref, mag, what):
    got = y.cpu().numpy()
    n = y.numel()
    edge = torch.cat([buf[:buf.numel() - n - 32], buf[buf.numel() - 32:]]).cpu().numpy()
    assert (edge == SENTINEL).all(), f"{what}: wrote outside y"
    assert not (got == SENTINEL).any(), f"{what}: {int((got == SENTINEL).sum())} outputs never written"
    e = np.abs(got - ref)
    assert e.max() <= 6e-5, f"{what}: max error {e.max():.3g}"
    r = (e / (2.0 ** -24 * mag + 1e-300)).max()
    assert r <= 64.0, f"{what}: {r:.3g} eps sum|x||w|"


def run_f16x3_case(tspn, device, B, T, Cin, M, seed, offset=0, combos=((True, False), (False, True), (True, True), (False, False)),
                   x=None, w=None):
    x = tspn.hashrng.uniform(seed, "x", (B, T, Cin), -1, 1) if x is None else x
    w = tspn.hashrng.normal(seed, "w", (M, Cin, 3), std=0.1) if w is None else w
    b = tspn.hashrng.normal(seed, "b", (M,), std=0.1)
    ref, mag = conv_tc_ref64(x, w)
    xd, bd = t(x).to(device), t(b).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device))
    outs = []
    for with_bias, relu in combos:
        r = ref + (b.astype(np.float64)[None, :, None] if with_bias else 0.0)
        buf, y = held_output((B, M, T), device, offset)
        f16x3_raw(tspn, xd, pk, bd if with_bias else None, relu, y)
        check_f16x3(buf, y, np.maximum(r, 0.0) if relu else r, mag + (np.abs(b)[None, :, None] if with_bias else 0.0),
                    f"B={B} T={T} Cin={Cin} M={M} offset={offset} bias={with_bias} relu={relu}")
        outs.append(y)
    return outs


@pytest.mark.parametrize("M,B,T,nwg_mod8", [
    (1280, 300, 7, 7),      # 5 row tiles (a group of 4 and a group of 1) x 3 sextet tiles = 15 workgroups, scalar tail
    (1280, 520, 12, 1),     # x 5 sextet tiles = 25, vec2 stores
    (1280, 800, 7, 3),      # x 7 = 35
    (2304, 550, 12, 5),     # 9 row tiles (4 + 4 + 1) x 5 = 45
])
def test_wino63_f16x3_tile_grid_and_sextet_edges(tspn, device, M, B, T, nwg_mod8):
    """Grids the workgroup remap has to get right: tiles_m % GM != 0 with tiles_m > GM, more than 8 workgroups with
    every odd remainder against the 8 XCDs; every tile is written exactly once (sentinel, float64 reference)."""
    tiles_m, tiles_n = M // F_BM, -(-(B * -(-T // 6)) // F_BN)
    assert tiles_m % F_GM != 0 and tiles_m > F_GM and tiles_m * tiles_n > 8 and (tiles_m * tiles_n) % 8 == nwg_mod8
    run_f16x3_case(tspn, device, B, T, 32, M, 430 + nwg_mod8)


@pytest.mark.parametrize("B,T,nsext", [(85, 17, 255), (128, 12, 256), (64, 19, 256), (257, 5, 257), (128, 24, 512)])
def test_wino63_f16x3_sextet_counts_at_the_tile_edge(tspn, device, B, T, nsext):
    """Exactly 255, 256, 257 and 512 sextets: one padded column, a full tile, one column in a second tile, no padding."""
    assert B * -(-T // 6) == nsext
    run_f16x3_case(tspn, device, B, T, 32, 512, 440 + T)


@pytest.mark.parametrize("T", [1, 5, 6, 7, 12, 31, 33, 34, 150])
def test_wino63_f16x3_every_T_both_store_forms(tspn, device, T):
    """Through the C entry ldy = T, so the 8-byte stores need T % 6 == 0 and an 8-byte aligned y; a y whose base is 4-byte
    but not 8-byte aligned takes the scalar stores at the same shape and equals the aligned launch bit for bit."""
    B, Cin, M = 5, 64, 256
    aligned = run_f16x3_case(tspn, device, B, T, Cin, M, 450)
    shifted = run_f16x3_case(tspn, device, B, T, Cin, M, 450, offset=1)
    for a, s in zip(aligned, shifted):
        assert torch.equal(a, s)


@pytest.mark.parametrize("Cin,B,T,M", [(32, 50, 33, 512), (64, 50, 31, 512), (2048, 3, 33, 256)])
def test_wino63_f16x3_contraction_depths(tspn, device, Cin, B, T, M):
    """Cin = 32: two k-steps per point, the ring shorter than its prefetch depth, over several tiles; Cin = 2048: the
    headline depth (benchmark distribution, whose outputs stay below 1)."""
    if Cin == 2048:
        run_f16x3_case(tspn, device, B, T, Cin, M, 460, x=tspn.hashrng.uniform(460, "x", (B, T, Cin)),
                       w=tspn.hashrng.normal(460, "w", (M, Cin, 3), std=0.01))
    else:
        run_f16x3_case(tspn, device, B, T, Cin, M, 460)


def test_wino63_f16x3_refusals_leave_the_output_untouched(tspn, device):
    """Every refusal of the split entry points comes before any launch: y keeps its sentinel and the workspace its
    fill (the input transform would have written it)."""
    E = tspn._abi
    B, T, Cin, M = 2, 9, 32, 256
    x = t(tspn.hashrng.uniform(470, "x", (B, T, Cin), -1, 1)).to(device)
    w = t(tspn.hashrng.normal(470, "w", (M, Cin, 3), std=0.1)).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(w)
    need = E.lib().tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M)
    pk_buf = torch.zeros(pk.numel() + 8, dtype=torch.int16, device=device)
    pk_off = pk_buf[2:2 + pk.numel()].view(pk.shape)
    pk_off.copy_(pk)
    assert pk_off.data_ptr() % 16 == 4

    def refused(code, xx=x, pkk=pk, ws_off=0, ws_bytes=None, MM=None):
        buf, y = held_output((B, MM or M, T), device)
        ws_buf = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=device)
        with pytest.raises(E.TspnError) as e:
            f16x3_raw(tspn, xx, pkk, None, False, y, ws=ws_buf[ws_off:], ws_bytes=need if ws_bytes is None else ws_bytes, M=MM)
        assert e.value.code == code, (e.value.code, str(e.value))
        torch.cuda.synchronize(device)
        assert bool((buf == float(SENTINEL)).all()) and bool((ws_buf == 0x5A).all())

    refused(E.TSPN_EINVAL, xx=off4(x.cpu(), device))                   # x: 16-byte pieces
    refused(E.TSPN_EUNSUPPORTED, pkk=pk_off)                           # packed: 16-byte LDS-DMA pieces
    refused(E.TSPN_EINVAL, ws_off=16)                                  # workspace: 256-byte aligned
    refused(E.TSPN_EWORKSPACE, ws_bytes=need - 256)                    # workspace: short
    refused(E.TSPN_EUNSUPPORTED, MM=128)                               # M % 256 != 0
    # the weight pack: M % 256, split with Cin != 2 split, packed at a 4-byte offset
    out = torch.full((pk.numel() + 8,), 0x5A5A, dtype=torch.int16, device=device)
    for (m, cin, split, o, code) in ((128, 32, 0, 0, E.TSPN_EUNSUPPORTED), (256, 96, 32, 0, E.TSPN_EINVAL),
                                     (256, 32, 0, 2, E.TSPN_EINVAL)):
        wt = torch.zeros((m, cin, 3), device=device)
        with pytest.raises(E.TspnError) as e:
            E.check(E.lib().tspn_pack_conv3_wino63_f16x3(p(wt), m, cin, split, p(out[o:]), tspn.ops._stream()))
        assert e.value.code == code
        torch.cuda.synchronize(device)
        assert bool((out == 0x5A5A).all())
    # a refused call is not sticky: the same operands, aligned, run
    buf, y = held_output((B, M, T), device)
    f16x3_raw(tspn, x, pk, None, False, y)
    assert torch.equal(y, tspn.ops.conv3_tc_wino63_f16x3(x, pk))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("T", [31, 33, 34])
@pytest.mark.parametrize("D", [64, 192])
def test_forward_fused_f16x3_against_dense_oracle(tspn, device, D, T, canonical):
    """tspn_forward_fused_f32 with conv_algo = TSPN_CONV_WINOGRAD63_F16X3 at ops level (gate D % 64 == 0), 45 tracklets =
    two contraction tiles: odd T keeps ldy = T (scalar stores), T = 34 with canonical pairs pads the rows of y to 36
    frames and takes the 8-byte stores over two pad frames, which must never reach an output.  Against the dense
    float64 oracle; the outputs are pre-filled and must all be written."""
    B, N, A = 5, 9, 4
    assert B * N * -(-T // 6) > F_BN
    w = fused_weights(tspn, D, A)
    vids = [tspn.synth.make_video(70 + b, N, T, D) for b in range(B)]
    feats = torch.cat([t(v["tracklet_feats"]) for v in vids])
    pairs = torch.cat([oracle.pair_index(N) + b * N for b in range(B)])
    if not canonical:
        pairs = pairs.flip(0).contiguous()
    d = lambda v: v.to(device).contiguous()
    packed = tspn.ops.pack_conv3_wino63_f16x3(d(w["conv_w"]), split=D)
    hw = d(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]]))
    hb = d(torch.cat([w["rel_b"], w["dur_b"]]))
    P = pairs.shape[0]
    out_h = torch.full((P, 3 * A, T), float(SENTINEL), device=device)
    out_l = torch.full((P, w["cls_w"].shape[0]), float(SENTINEL), device=device)
    need = tspn.ops.fused_workspace_bytes(B, N, T, D, A, w["cls_w"].shape[0], P, conv_algo=tspn._abi.CONV_WINOGRAD63_F16X3)
    ws = torch.full((need,), 0x7F, dtype=torch.uint8, device=device)      # pad frames of y start as NaN bit patterns
    heads, logits = tspn.ops.forward_fused(d(feats), d(pairs), B, N, packed, d(w["conv_b"]), hw, hb, d(w["cls_w"]),
                                           d(w["cls_b"]), canonical_pairs=canonical, workspace=ws, out_heads=out_h,
                                           out_logits=out_l)
    assert not bool((heads == float(SENTINEL)).any()) and not bool((logits == float(SENTINEL)).any())
    refs = [oracle.forward_dense(t(v["tracklet_feats"]).double(), t(v["tracklet_boxes"]).double(), oracle.pair_index(N),
                                 {k: x.double() for k, x in w.items()}) for v in vids]
    rel = torch.cat([r["relness"] for r in refs]).numpy()
    dur = torch.cat([r["duration"] for r in refs]).numpy()
    lg = torch.cat([r["rel_logits"] for r in refs]).numpy()
    if not canonical:
        rel, dur, lg = rel[::-1], dur[::-1], lg[::-1]
    np.testing.assert_allclose(heads[:, :A].cpu().numpy(), rel, rtol=0, atol=6e-5)
    np.testing.assert_allclose(heads[:, A:].cpu().numpy(), dur, rtol=0, atol=6e-5)
    np.testing.assert_allclose(logits.cpu().numpy(), lg, rtol=0, atol=2e-5)


def test_forward_fused_f16x3_refuses_d32_before_any_launch(tspn, device):
    """D = 32 passes the fp32 F(6,3) gate but not the split form's (4D % 256): TSPN_EUNSUPPORTED, and neither the heads
    nor the logits (computed first in a pass that runs) are touched."""
    B, N, T, D, A = 1, 3, 12, 32, 4
    w = fused_weights(tspn, D, A)
    d = lambda v: v.to(device).contiguous()
    pairs = oracle.pair_index(N)
    fake = torch.zeros((8, 2 * (D // 8) + 1, 4 * D, 8), dtype=torch.int16, device=device)
    assert tspn.ops.wino63_f16x3_dims(fake) == (D, 4 * D)
    out_h = torch.full((pairs.shape[0], 3 * A, T), float(SENTINEL), device=device)
    out_l = torch.full((pairs.shape[0], w["cls_w"].shape[0]), float(SENTINEL), device=device)
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn.ops.forward_fused(d(torch.zeros(N, T, D)), d(pairs), B, N, fake, d(w["conv_b"]),
                               d(torch.cat([w["rel_w"][:, :, 0], w["dur_w"][:, :, 0]])), d(torch.cat([w["rel_b"], w["dur_b"]])),
                               d(w["cls_w"]), d(w["cls_b"]), canonical_pairs=True, out_heads=out_h, out_logits=out_l)
    assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED
    torch.cuda.synchronize(device)
    assert bool((out_h == float(SENTINEL)).all()) and bool((out_l == float(SENTINEL)).all())
