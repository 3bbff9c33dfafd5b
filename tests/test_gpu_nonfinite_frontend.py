"""Non-finite values through the frames -> features front end (DESIGN.md §2 "Non-finite values", the front-end bullet).

Inputs are finite except for planted +-Inf / NaN (either sign, a quiet and a signalling payload; +Inf also against one
zero weight), as image pixels or as elements of a feature map or a residual.  Every output is NaN, +Inf or -Inf exactly
where the float64 restatement's is (tests/frontend_nonfinite_reference.py: products and sums elementwise, torch's ReLU
and max pool), within the entry's existing bound elsewhere -- and CONFINED: wherever the reference of the planted input
equals the reference of the clean input bit for bit, the GPU output has the bits of the GPU's clean launch.  A bad
value therefore never crosses into another row, image, frame or frame chunk through a masked tap, a garbage column, an
LDS exchange buffer or a carried pool column.  The fused kernels are also held, bit for bit with NaN == NaN, to the
launch chains they replace.  Box coordinates stay finite (DESIGN.md §8 gap 11).

tests/test_frontend_nonfinite_host.py checks on the CPU that no case can pass emptily."""
import functools

import numpy as np
import pytest
import torch

import conv2d_edge_cases as ce
import frontend_nonfinite_reference as fr
from frontend_nonfinite_reference import assert_confined, assert_same_nonfinite, assert_scores_equal, t, to_bf16
from oracle import roi_head_oracle as ro
from test_gpu_frontend_edges import ROI_ATOL, ROI_SCALE, ROIS

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -8


def f32(y):
    return y.detach().cpu().float().numpy()


def finite_scale(ref):
    return float(np.abs(ref[np.isfinite(ref)]).max())


def same_with_nan(got, want, what):
    """Bit equality in which any NaN equals any NaN (assert_scores_equal of the scoring path's file)."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), what
    assert_scores_equal(f32(got), f32(want))


def check(got_p, got_c, ref_p, ref_c, atol, what):
    """Positions against the reference and the bound on the finite rest; confinement against the clean launch."""
    assert_same_nonfinite(f32(got_p), ref_p, atol, what)
    assert_confined(f32(got_p), f32(got_c), ref_p, ref_c, what)


# ================================================================================================== rule cases: conv2d
@pytest.mark.parametrize("plant", fr.PLANT_IDS)
@pytest.mark.parametrize("form", fr.CONV_FORMS)
def test_conv2d_forms_with_relu_and_residual(tspn, device, form, plant):
    """conv2d_nhwc_kernel<16>, conv2d_nhwc_frag_kernel<false> (two geometries) and <true>, the four
    conv2d_nhwc_bf16_kernel<MI, RNG>: relu = True, a residual where the entry takes one.  fp32 forms: the suite's 2e-5;
    bf16: half a bf16 ulp of the value plus 3e-5 (test_conv2d_nhwc_bf16_vs_float64)."""
    kind, g, x, xp, w, b, r, rp, ref_c, ref_p = fr.conv_case(form, plant)
    if kind == "bf16":
        assert ce.bf16_kernel(ce.Case("bf16", w.shape[1], w.shape[0], g, 3)) == (int(form[5]), form[7] == "1")
    packed = ce.pack(tspn, device, kind, w)
    bd = t(b).to(device)

    def run(xa, ra):
        if kind == "bf16":
            return tspn.ops.conv2d_nhwc_bf16(to_bf16(xa).to(device), packed, (g.KH, g.KW), g.stride, g.pad, bias=bd,
                                             residual=to_bf16(ra).to(device), relu=True)
        if kind == "cin4":
            x4 = torch.nn.functional.pad(t(xa), (0, 1)).contiguous().to(device)
            return tspn.ops.conv2d_nhwc_cin4(x4, packed, (g.KH, g.KW), g.stride, g.pad, bias=bd, relu=True)
        return tspn.ops.conv2d_nhwc(t(xa).to(device), packed, (g.KH, g.KW), g.stride, g.pad, bias=bd,
                                    residual=t(ra).to(device), relu=True)
    got_c, got_p = run(x, r), run(xp, rp)
    atol = BF16_ULP * finite_scale(ref_p) + 3e-5 if kind == "bf16" else 2e-5
    check(got_p, got_c, ref_p, ref_c, atol, f"{form} {plant}")
    if kind == "bf16":
        fin = np.isfinite(ref_p)
        assert (np.abs(f32(got_p).astype(np.float64)[fin] - ref_p[fin]) <= np.abs(ref_p[fin]) * BF16_ULP + 3e-5).all()


# ================================================================================================== rule cases: max pools
@pytest.mark.parametrize("ksp", fr.POOL_KSP, ids=lambda v: "k%ds%dp%d" % v)
@pytest.mark.parametrize("C", fr.POOL_C)
@pytest.mark.parametrize("shape", fr.POOL_MAPS, ids=lambda v: "%dx%dx%d" % v)
def test_max_pools_propagate_nan_and_keep_padding_out(tspn, device, shape, C, ksp):
    """fp32 -> fp32, fp32 -> bf16 and bf16 -> bf16 on a map of bf16 values (so the three agree bit for bit): the four NaN
    encodings, +Inf, -Inf and a window of only -Inf.  A max pool moves values: outside NaN the output is the
    reference's bit for bit."""
    k, s, p = ksp
    x, xp = fr.pool_case(shape, C, ksp)
    NB, H, W = shape
    if H + 2 * p < k or W + 2 * p < k:
        with pytest.raises(ValueError):                  # no output at this size (tests/test_gpu_frontend_edges.py)
            tspn.ops.max_pool_nhwc(t(xp).to(device), k, s, p)
        return
    ref_c, ref_p = fr.max_pool_ref(x, k, s, p), fr.max_pool_ref(xp, k, s, p)
    for what, run in (("fp32 -> fp32", lambda a: tspn.ops.max_pool_nhwc(t(a).to(device), k, s, p)),
                      ("fp32 -> bf16", lambda a: tspn.ops.max_pool_nhwc(t(a).to(device), k, s, p, out_bf16=True)),
                      ("bf16 -> bf16", lambda a: tspn.ops.max_pool_nhwc_bf16(to_bf16(a).to(device), k, s, p))):
        got_c, got_p = run(x), run(xp)
        check(got_p, got_c, ref_p, ref_c, 0.0, f"{what} {shape} C={C} {ksp}")
        assert_scores_equal(f32(got_p), ref_p.astype(np.float32))


# ================================================================================================== stem
def stem_operands(tspn, device, shape):
    x, xp, w, b, ref_c, ref_p, pool_c, pool_p = fr.stem_case(*shape)
    frag = tspn.ops.pack_stem_bf16(t(w).to(device))
    return t(x).to(device), t(xp).to(device), frag, t(b).to(device), ref_c, ref_p, pool_c, pool_p


@pytest.mark.parametrize("shape", fr.STEM_SHAPES, ids=lambda v: "%dx%dx%dx%d" % v)
def test_stem_conv_positions_and_confinement(tspn, device, shape):
    """ops.stem_conv_bf16: pixel (0, 0), the last pixel of image 0, the first of image 1, input columns 255 / 256 of a
    513-wide row.  The 7 x 7 / 2 conv runs as a 4 x 4 conv on the 2 x 2 space-to-depth image, whose eighth row and
    column of taps carry zero weights: a pixel there must not reach the output.  Bound: one bf16 ulp of the range
    (test_stem_bf16_vs_oracle)."""
    x, xp, frag, b, ref_c, ref_p, _, _ = stem_operands(tspn, device, shape)
    got_c, got_p = tspn.ops.stem_conv_bf16(x, frag, b), tspn.ops.stem_conv_bf16(xp, frag, b)
    check(got_p, got_c, ref_p, ref_c, BF16_ULP * finite_scale(ref_p), f"stem conv {shape}")


@pytest.mark.parametrize("shape", fr.STEM_POOL_SHAPES, ids=lambda v: "%dx%dx%dx%d" % v)
def test_stem_pool_equals_conv_then_pool_and_the_reference(tspn, device, shape):
    """ops.stem_pool_bf16 (accumulator-level maximum of three conv rows, the pooled column carried across the 128-column
    tile boundary) == stem_conv_bf16 + max_pool_nhwc_bf16 bit for bit with NaN == NaN, and both against the reference."""
    x, xp, frag, b, _, _, pool_c, pool_p = stem_operands(tspn, device, shape)
    got_c, got_p = tspn.ops.stem_pool_bf16(x, frag, b), tspn.ops.stem_pool_bf16(xp, frag, b)
    chain_c = tspn.ops.max_pool_nhwc_bf16(tspn.ops.stem_conv_bf16(x, frag, b), 3, 2, 1)
    chain_p = tspn.ops.max_pool_nhwc_bf16(tspn.ops.stem_conv_bf16(xp, frag, b), 3, 2, 1)
    assert torch.equal(got_c, chain_c)
    same_with_nan(got_p, chain_p, f"stem pool {shape} against conv + pool")
    atol = BF16_ULP * finite_scale(pool_p)
    check(chain_p, chain_c, pool_p, pool_c, atol, f"stem conv + pool {shape}")
    check(got_p, got_c, pool_p, pool_c, atol, f"stem pool {shape}")


# ================================================================================================== fused tails
TAIL_CASES = [(s, "one_role") for s in fr.TAIL_SHAPES] + \
    [(fr.TAIL_SHAPES[2], f) for f in ("next_frag1", "persistent0", "persistent1", "io_waves")]


@functools.lru_cache(maxsize=None)
def tail_device(device, shape):
    import tspn_mi355x as tspn
    h1, h1p, res, resp, w2, b2, w3, b3, ref_c, ref_p = fr.tail_case(*shape)
    d = lambda a: t(a).to(device)   # noqa: E731
    f2, f3 = tspn.ops.pack_conv2d_frag_bf16(d(w2)), tspn.ops.pack_conv2d_frag_bf16(d(w3))
    ops = dict(f2=f2, f3=f3, b2=d(b2), b3=d(b3))
    chain = []
    for a, r in ((h1, res), (h1p, resp)):
        ad, rd = to_bf16(a).to(device), to_bf16(r).to(device)
        h2 = tspn.ops.conv2d_nhwc_bf16(ad, f2, (3, 3), 1, 1, bias=ops["b2"], relu=True)
        chain.append((ad, rd, tspn.ops.conv2d_nhwc_bf16(h2, f3, (1, 1), 1, 0, bias=ops["b3"], residual=rd, relu=True)))
    return ops, chain, ref_c, ref_p


@pytest.mark.parametrize("shape", fr.TAIL_SHAPES, ids=lambda v: "%dx%dx%dx%d" % v)
def test_tail_two_launch_chain_against_the_reference(tspn, device, shape):
    """conv2d_nhwc_bf16 (3 x 3, linear ranges) + conv2d_nhwc_bf16 (expand, residual, ReLU) with planted values on both
    sides of a row wrap, of the image boundary and of linear pixel 128, one +Inf against a zero weight and one +Inf in
    the residual.  Bound: four bf16 ulps of the range (test_bottleneck_tail_fused_bit_identical_to_two_convs)."""
    _, chain, ref_c, ref_p = tail_device(device, shape)
    check(chain[1][2], chain[0][2], ref_p, ref_c, 4 * BF16_ULP * finite_scale(ref_p), f"tail chain {shape}")


@pytest.mark.parametrize("shape,form", TAIL_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%dx%dx%d" % v)
def test_fused_tail_forms_equal_the_chain(tspn, device, shape, form):
    """ops.bottleneck_tail_bf16 one-role at all three widths; at CM = 256 also with the next block's conv1, persistent
    (grid unlimited and one workgroup) and role-split: clean and planted launches equal the two-launch chain bit for
    bit with NaN == NaN, and the planted launch is confined like the reference."""
    ops, chain, ref_c, ref_p = tail_device(device, shape)
    kw = {"one_role": {}, "persistent0": dict(persistent=True, max_workgroups=0),
          "persistent1": dict(persistent=True, max_workgroups=1), "io_waves": dict(io_waves=True)}.get(form)
    CM = shape[0]
    got = []
    if form == "next_frag1":
        w1n = fr.r16(fr.nonzero_normal(tspn.hashrng, 1706, "w1n", (CM, 4 * CM, 1, 1), float(np.sqrt(2.0 / (4 * CM)))))
        b1n = tspn.hashrng.normal(1706, "b1n", (CM,), std=0.1)
        f1n = tspn.ops.pack_conv2d_frag_bf16(t(w1n.astype(np.float32)).to(device))
    for ad, rd, want in chain:
        if form == "next_frag1":
            out, h1n = tspn.ops.bottleneck_tail_bf16(ad, ops["f2"], ops["b2"], ops["f3"], ops["b3"], rd, next_frag1=f1n,
                                                     next_bias1=t(b1n).to(device))
            want_h = tspn.ops.conv2d_nhwc_bf16(want, f1n, (1, 1), 1, 0, bias=t(b1n).to(device), relu=True)
            same_with_nan(h1n, want_h, f"{form} {shape}: h1_next")
        else:
            out = tspn.ops.bottleneck_tail_bf16(ad, ops["f2"], ops["b2"], ops["f3"], ops["b3"], rd,
                                                out=torch.full_like(want, 777.0), **kw)
        same_with_nan(out, want, f"{form} {shape}")
        got.append(out)
    assert torch.equal(got[0], chain[0][2])
    check(got[1], got[0], ref_p, ref_c, 4 * BF16_ULP * finite_scale(ref_p), f"tail {form} {shape}")


# ================================================================================================== one-launch blocks
BLOCK_CASES = [("id", s) for s in fr.BLOCK_SHAPES] + [("proj", (64, 1, 11, 31)), ("res", (128, 1, 13, 61))]


@pytest.mark.parametrize("kind,shape", BLOCK_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%dx%dx%d" % v)
def test_one_launch_blocks_equal_their_chain_and_the_reference(tspn, device, kind, shape):
    """ops.bottleneck_block_bf16 (2 x 2 tiles of 10 x 30 and 6 x 30 with a recomputed halo, two images),
    bottleneck_block_proj_bf16 and bottleneck_block_res_bf16 (stride 2): planted values at (0, 0), on both sides of the
    tile grid's inner corner, at (H - 1, W - 1) and at the end of image 0; one +Inf whose conv1 row is -Inf everywhere
    (h1 = 0: the shortcut's infinity comes out as one).  Against conv1 (+ shortcut) + fused tail bit for bit with NaN ==
    NaN, and against the reference within four bf16 ulps of the range.  Stride 2: planted values at odd coordinates,
    which no tap reads, leave the clean launch's bits."""
    c = fr.block_case(kind, *shape)
    d = lambda a: t(a).to(device)   # noqa: E731
    b = {k: d(v) for k, v in c["b"].items()}
    f1, f2, f3 = (tspn.ops.pack_conv2d_frag_bf16(d(c[k])) for k in ("w1", "w2", "w3"))
    fs = tspn.ops.pack_conv2d_frag_bf16(d(c["ws"])) if kind == "proj" else None
    s = c["stride"]

    def run(xa, ra):
        xd = to_bf16(xa).to(device)
        h1 = tspn.ops.conv2d_nhwc_bf16(xd, f1, (1, 1), s, 0, bias=b["b1"], relu=True)
        if kind == "id":
            sc = xd
            got = tspn.ops.bottleneck_block_bf16(xd, f1, b["b1"], f2, b["b2"], f3, b["b3"])
        elif kind == "proj":
            sc = tspn.ops.conv2d_nhwc_bf16(xd, fs, (1, 1), s, 0, bias=b["bs"], relu=False)
            got = tspn.ops.bottleneck_block_proj_bf16(xd, s, f1, b["b1"], f2, b["b2"], f3, b["b3"], fs, b["bs"])
        else:
            sc = to_bf16(ra).to(device)
            got = tspn.ops.bottleneck_block_res_bf16(xd, s, f1, b["b1"], f2, b["b2"], f3, b["b3"], sc)
        return got, tspn.ops.bottleneck_tail_bf16(h1, f2, b["b2"], f3, b["b3"], sc)
    got_c, chain_c = run(c["x"], c["res"])
    got_p, chain_p = run(c["xp"], c.get("resp"))
    what = f"block {kind} {shape}"
    assert torch.equal(got_c, chain_c), what
    same_with_nan(got_p, chain_p, what + " against its chain")
    atol = 4 * BF16_ULP * finite_scale(c["ref_p"])
    check(chain_p, chain_c, c["ref_p"], c["ref_c"], atol, what + " (chain)")
    check(got_p, got_c, c["ref_p"], c["ref_c"], atol, what)
    if kind == "res":
        got_o, chain_o = run(c["xodd"], c["res"])
        assert torch.equal(got_o, got_c) and torch.equal(chain_o, chain_c), "a value at an odd coordinate was read"


# ================================================================================================== RoIAlign
@functools.lru_cache(maxsize=None)
def roi_case():
    """The in-image map and finite boxes of tests/test_gpu_frontend_edges.py (3 x 9 x 12, C = 160, bf16 values); planted:
    NaN at (0, 3, 4, 5), +Inf at (1, 2, 6, 17), -Inf at (2, 1, 1, 33), a signalling NaN at (0, 8, 11, 150).  float64
    oracle of both maps, aligned, adaptive sampling."""
    import tspn_mi355x as tspn
    C, P = 160, 7
    fm = fr.r16(tspn.hashrng.uniform(1707, "roi-map", (3, 9, 12, C), -1, 1)).astype(np.float32)
    fp = fm.copy()
    fp[0, 3, 4, 5] = fr.bf16_value("nan-")
    fp[1, 2, 6, 17] = np.inf
    fp[2, 1, 1, 33] = -np.inf
    fp[0, 8, 11, 150] = fr.bf16_value("snan+")
    with np.errstate(invalid="ignore"):
        ref_c = ro.roi_align_nhwc(fm, ROIS, P, ROI_SCALE, 0, True, dtype=np.float64).numpy()
        ref_p = ro.roi_align_nhwc(fp, ROIS, P, ROI_SCALE, 0, True, dtype=np.float64).numpy()
    return fm, fp, ref_c, ref_p


def test_roi_align_feature_values_three_instantiations(tspn, device):
    """NaN / +-Inf in the feature map only, boxes finite.  <false, false>, <false, true> and <true, true> at P = 7, C = 160:
    positions from the float64 oracle; RoIs (here: output elements) whose samples do not touch a planted pixel are
    bit-equal to the clean launch.  A bilinear weight of exactly zero on a planted pixel is Inf * 0 in the oracle as
    in the kernel.  Bounds: 2e-6 (fp32), one bf16 ulp of the value plus 2e-6 (bf16 out)."""
    P = 7
    fm, fp, ref_c, ref_p = roi_case()
    fr.check_not_empty(ref_p, ref_c, True, "roi align")
    whole = fr.untouched(ref_p, ref_c).reshape(len(ROIS), -1).all(axis=1)
    assert whole.any() and not whole.all()                      # RoIs that never touch a planted pixel exist
    rois = t(ROIS).to(device)
    forms = (("fp32", lambda a: tspn.ops.roi_align_nhwc(t(a).to(device), rois, P, ROI_SCALE, 0, True), ROI_ATOL * 2),
             ("fp32 -> bf16",
              lambda a: tspn.ops.roi_align_nhwc(t(a).to(device), rois, P, ROI_SCALE, 0, True, out_bf16=True), None),
             ("bf16", lambda a: tspn.ops.roi_align_nhwc(to_bf16(a).to(device), rois, P, ROI_SCALE, 0, True), None))
    for what, run, atol in forms:
        got_c, got_p = run(fm), run(fp)
        atol = atol if atol is not None else BF16_ULP * finite_scale(ref_p) + ROI_ATOL
        check(got_p, got_c, ref_p, ref_c, atol, f"roi align {what}")
        assert torch.equal(got_p[t(whole).to(device)], got_c[t(whole).to(device)])


# ================================================================================================== model level
def plant_frames(img):
    """One NaN pixel in frame 1 and one +Inf pixel in frame 3 (five frames, frame_chunk = 2: chunks {0, 1}, {2, 3}, {4})."""
    img = np.array(img)
    img[1, img.shape[1] // 2, img.shape[2] // 3, 1] = fr.NAN_NEG_PAY
    img[3, 5, 7, 2] = np.inf
    return img


def check_frames(got_p, got_c, ref_p, ref_c, atol, what):
    """Frames 0, 2, 4: the clean run's bits (and an unchanged oracle); frames 1, 3: the oracle's positions."""
    gp, gc = f32(got_p), f32(got_c)
    for f in (0, 2, 4):
        assert fr.same_bits(ref_p[f], ref_c[f]).all() and np.isfinite(ref_c[f]).all(), f"{what}: oracle frame {f} changed"
        np.testing.assert_array_equal(gp[f].view(np.uint32), gc[f].view(np.uint32), err_msg=f"{what}: frame {f}")
    assert np.isnan(ref_p[1]).any() and not np.isfinite(ref_p[3]).all()
    for f in (1, 3):
        assert_same_nonfinite(gp[f], ref_p[f], atol, f"{what}: frame {f}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_resnet_c4_keeps_a_bad_pixel_inside_its_frame(tspn, device, bf16):
    """ResNetC4 as test_resnet_c4_backbone_matches_oracle / ..._bf16_... build it, five frames, frame_chunk = 2."""
    from test_gpu_roi_head import _backbone_and_weights
    blocks, stem_out, res2_out, hw = ((1, 1, 2), 64, 256, (64, 96)) if bf16 else ((2, 2, 3), 16, 64, (70, 100))
    net, p = _backbone_and_weights(tspn, device, stem_out, res2_out, blocks)
    assert net.frame_chunk == 2
    img = tspn.hashrng.uniform(1708, "img", (5,) + hw + (3,), -1, 1)
    imgp = plant_frames(img)
    got_c, got_p = net(t(img).to(device), bf16=bf16), net(t(imgp).to(device), bf16=bf16)
    with np.errstate(invalid="ignore"):
        if bf16:
            ref_c, ref_p = (ro.resnet_c4_bf16(t(a), p, blocks).double().numpy() for a in (img, imgp))
        else:
            ref_c, ref_p = (ro.resnet_c4(t(a), p, blocks).double().numpy() for a in (img, imgp))
    scale = max(1.0, finite_scale(ref_c))
    check_frames(got_p, got_c, ref_p, ref_c, 6 * BF16_ULP * scale if bf16 else 5e-5 * scale, f"ResNetC4 bf16={bf16}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_res5_roi_head_keeps_a_bad_map_value_inside_its_frame(tspn, device, bf16):
    """Res5RoIHead as test_res5_roi_head_bf16_matches_oracle builds it (RoIs in chunks of 7), five frames: one NaN element
    in the map of frame 1 and one +Inf element in the map of frame 3, each under one box; features [N, T, C] of frames
    0, 2, 4 keep the clean run's bits."""
    from test_gpu_roi_head import _head_and_weights
    N, T, cin, mid, cout = 3, 5, 128, 64, 256
    head, p = _head_and_weights(tspn, device, cin, mid, cout, roi_chunk=7)
    fm = fr.r16(tspn.hashrng.uniform(1709, "fm", (T, 10, 12, cin), 0, 1)).astype(np.float32)
    fmp = fm.copy()
    fmp[1, 5, 6, 3] = fr.bf16_value("nan-pay")          # one map element each, under one tracklet's box of that frame
    fmp[3, 6, 5, 9] = np.inf
    v = tspn.synth.make_video(1709, N, T, 16)
    boxes = (v["tracklet_boxes"] * np.float32(0.15)).astype(np.float32)
    cast = (lambda a: to_bf16(a).to(device)) if bf16 else (lambda a: t(a).to(device))
    got_c, got_p = head(cast(fm), t(boxes).to(device)), head(cast(fmp), t(boxes).to(device))
    with np.errstate(invalid="ignore"):
        if bf16:
            ref_c, ref_p = (ro.res5_roi_head_bf16(t(a), t(boxes), p).double().numpy() for a in (fm, fmp))
        else:
            ref_c, ref_p = (ro.res5_roi_head(t(a), t(boxes), p, dtype=torch.float64).double().numpy() for a in (fm, fmp))
    scale = max(1.0, finite_scale(ref_c))
    tr = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))   # noqa: E731  [N, T, C] -> [T, N, C]
    check_frames(t(tr(f32(got_p))), t(tr(f32(got_c))), tr(ref_p), tr(ref_c), 4 * BF16_ULP * scale if bf16 else 2e-5 * scale,
                 f"Res5RoIHead bf16={bf16}")
