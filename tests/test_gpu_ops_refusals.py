"""The refusals of the ops wrappers that share their operand checks (ops._workspace, _out_hw, _bias_residual, _toggle,
_stem_bf16, _span_rows, _decode_span_relations, _block_operands / _block_frags_match): exception type and the whole
message, as the wrappers worded them before they shared a body, on the smallest tensors that pass ops._dev.  Every case is
refused in Python before anything is launched, or is a valid tiny call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64


def refused(exc, text, fn, *args, **kwargs):
    with pytest.raises(exc) as e:
        fn(*args, **kwargs)
    assert type(e.value) is exc and str(e.value) == text


@pytest.fixture(scope="module")
def z(device):
    return lambda *shape, dtype=F32: torch.zeros(shape, dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------- workspaces, toggles
def test_stem_wrappers(tspn, z):
    ops = tspn.ops
    img, frag, bias, short = z(1, 8, 8, 3), z(2, 16, 64, 8, dtype=BF16), z(64), z(16, dtype=torch.uint8)
    for who, fn, shape in (("stem_conv_bf16", ops.stem_conv_bf16, (1, 4, 4, 64)), ("stem_pool_bf16", ops.stem_pool_bf16, (1, 2, 2, 64))):
        refused(TypeError, "x: expected torch.float32, got torch.bfloat16", fn, img.to(BF16), frag, bias)
        refused(TypeError, "frag: expected torch.bfloat16, got torch.float32", fn, img, frag.float(), bias)
        refused(ValueError, f"{who}: x must be [NB,H,W,3] and frag = pack_stem_bf16(weight)", fn, z(1, 8, 8, 4), frag, bias)
        refused(ValueError, f"{who}: x must be [NB,H,W,3] and frag = pack_stem_bf16(weight)", fn, img, z(2, 16, 64, 4, dtype=BF16), bias)
        refused(ValueError, f"{who}: bias shape mismatch", fn, img, frag, z(32))
        refused(ValueError, f"{who}: workspace too small", fn, img, frag, bias, workspace=short)
        out = fn(img, frag, bias)                                  # zero weights, zero bias: relu(0)
        assert tuple(out.shape) == shape and out.dtype == BF16 and not out.any()


def test_workspace_refusals_that_name_both_sizes(tspn, z):
    ops, lib = tspn.ops, tspn._abi.lib()
    short = z(16, dtype=torch.uint8)
    need = lib.tspn_conv3_tc_wino63_workspace_bytes(1, 6, 32)
    refused(ValueError, f"conv3_tc_wino63: workspace too small (16 < {need})", ops.conv3_tc_wino63, z(1, 6, 32),
            z(1, 4, 8, 64, 4), workspace=short)
    need = lib.tspn_conv3_tc_wino63_f16x3_workspace_bytes(1, 6, 32, 256)
    refused(ValueError, f"conv3_tc_wino63_f16x3: workspace too small (16 < {need})", ops.conv3_tc_wino63_f16x3, z(1, 6, 32),
            z(8, 9, 256, 8, dtype=torch.int16), workspace=short)
    B, N, T, D, A, K = 1, 2, 4, 16, 1, 3
    need = ops.fused_workspace_bytes(B, N, T, D, A, K, 2)
    assert need > 16
    refused(ValueError, f"forward_fused: workspace too small (16 < {need})", ops.forward_fused, z(2, T, D), z(2, 2, dtype=I64),
            B, N, z(3, D, 4 * D), z(2 * D), z(3, 2 * D), z(3), z(K, 2 * D), z(K), workspace=short)


def test_workspace_refusals_without_sizes(tspn, z):
    ops = tspn.ops
    short = z(16, dtype=torch.uint8)
    B, N, T, D, K = 1, 2, 4, 16, 3
    args = (z(2, T, D, dtype=BF16), z(2, 2, dtype=I64), B, N, z(3, D // 8, 4 * D, 8, dtype=BF16), z(2 * D),
            z(2 * D // 8, 16, 8, dtype=BF16), z(3), z(K, 2 * D), z(K))
    refused(ValueError, "forward_fused_bf16: workspace too small", ops.forward_fused_bf16, *args, workspace=short)
    refused(ValueError, "forward_fused_bf16: workspace too small", ops.forward_fused_bf16, *args, workspace=short,
            canonical_pairs=False, check_pairs=False)
    feats, pairs, spans, packed = z(2, T, D, dtype=BF16), z(1, 2, dtype=I64), z(1, 2, dtype=I64), z(1, 1, 64, 8, dtype=BF16)
    refused(ValueError, "span_predicate_bf16: workspace too small", ops.span_predicate_bf16, feats, pairs, spans, packed, z(K),
            K, workspace=short)


def test_toggles_return_the_previous_setting(tspn, device):
    ops = tspn.ops
    for setter in (ops.wino63_set_piece_form, ops.wino63_f16x3_set_tail_split, ops.heads_pairgrid_f16x3_set_force_exact):
        before = setter(1)
        assert before in (0, 1) and setter(0) == 1 and setter(before) == 0 and setter(before) == before


# ------------------------------------------------------------------------------------------- conv2d / pools
def test_empty_outputs(tspn, z):
    ops = tspn.ops
    m16, m32 = z(1, 4, 4, 64, dtype=BF16), z(1, 4, 4, 16)
    refused(ValueError, "conv2d_nhwc: empty output", ops.conv2d_nhwc, m32, z(49, 16, 4), (7, 7))
    refused(ValueError, "conv2d_nhwc: empty output", ops.conv2d_nhwc, m32, z(1, 49, 1, 64, 8), (7, 7), stride=2, padding=1)
    refused(ValueError, "conv2d_nhwc_bf16: empty output", ops.conv2d_nhwc_bf16, m16, z(1, 1, 49, 4, 64, 8, dtype=BF16), (7, 7))
    refused(ValueError, "conv2d_nhwc_cin4: empty output", ops.conv2d_nhwc_cin4, z(1, 4, 4, 4), z(1, 13, 64, 8), (7, 7))
    refused(ValueError, "max_pool_nhwc: empty output", ops.max_pool_nhwc, m32, kernel_size=7, stride=2, padding=0)
    refused(ValueError, "max_pool_nhwc_bf16: empty output", ops.max_pool_nhwc_bf16, m16, kernel_size=7, stride=2, padding=0)
    # the smallest output that is not empty: one pixel
    assert tuple(ops.max_pool_nhwc(m32, kernel_size=4, stride=2, padding=0).shape) == (1, 1, 1, 16)
    assert tuple(ops.max_pool_nhwc_bf16(m16, kernel_size=4, stride=2, padding=0).shape) == (1, 1, 1, 64)


def test_bias_and_residual_of_the_conv_wrappers(tspn, z):
    ops = tspn.ops
    m16, m32 = z(1, 4, 4, 64, dtype=BF16), z(1, 4, 4, 16)
    w32, w16 = z(1, 16, 4), z(1, 1, 1, 4, 64, 8, dtype=BF16)               # 1x1: Cout = 4 / Cout = 32
    refused(ValueError, "conv2d_nhwc: bias shape mismatch", ops.conv2d_nhwc, m32, w32, (1, 1), bias=z(5))
    refused(ValueError, "conv2d_nhwc: residual shape mismatch", ops.conv2d_nhwc, m32, w32, (1, 1), residual=z(1, 4, 4, 8))
    refused(ValueError, "conv2d_nhwc: residual shape mismatch", ops.conv2d_nhwc, m32, w32, (1, 1), stride=2, residual=z(1, 4, 4, 4))
    refused(TypeError, "residual: expected torch.float32, got torch.bfloat16", ops.conv2d_nhwc, m32, w32, (1, 1),
            residual=z(1, 4, 4, 4, dtype=BF16))
    refused(TypeError, "bias: expected torch.float32, got torch.bfloat16", ops.conv2d_nhwc, m32, w32, (1, 1), bias=z(4, dtype=BF16))
    refused(ValueError, "conv2d_nhwc_bf16: bias shape mismatch", ops.conv2d_nhwc_bf16, m16, w16, (1, 1), bias=z(5))
    refused(ValueError, "conv2d_nhwc_bf16: residual shape mismatch", ops.conv2d_nhwc_bf16, m16, w16, (1, 1),
            residual=z(1, 4, 4, 64, dtype=BF16))
    refused(TypeError, "residual: expected torch.bfloat16, got torch.float32", ops.conv2d_nhwc_bf16, m16, w16, (1, 1),
            residual=z(1, 4, 4, 32))
    refused(TypeError, "bias: expected torch.float32, got torch.bfloat16", ops.conv2d_nhwc_bf16, m16, w16, (1, 1),
            bias=z(32, dtype=BF16))
    out = ops.conv2d_nhwc_bf16(m16, w16, (1, 1), bias=z(32), residual=z(1, 4, 4, 32, dtype=BF16), relu=True)
    assert tuple(out.shape) == (1, 4, 4, 32) and not out.any()
    out = ops.conv2d_nhwc(m32, w32, (1, 1), bias=z(4), residual=z(1, 4, 4, 4))
    assert tuple(out.shape) == (1, 4, 4, 4) and not out.any()


# ------------------------------------------------------------------------------------------- bottleneck blocks
def frags(z, CIN, CM, shortcut=False):
    shape = lambda cout, cin, taps: (cout // 32, cin // 64, taps, 4, 64, 8)
    f = [z(*shape(CM, CIN, 1), dtype=BF16), z(*shape(CM, CM, 9), dtype=BF16), z(*shape(4 * CM, CM, 1), dtype=BF16)]
    return f + [z(*shape(4 * CM, CIN, 1), dtype=BF16)] if shortcut else f


def test_bottleneck_block_wrappers(tspn, z):
    ops = tspn.ops
    m = z(1, 4, 4, 64, dtype=BF16)
    # identity block: 4 CM = 256 channels
    x, (f1, f2, f3), b, b4 = z(1, 4, 4, 256, dtype=BF16), frags(z, 256, 64), z(64), z(256)
    who, fn = "bottleneck_block_bf16", ops.bottleneck_block_bf16
    refused(TypeError, "x: expected torch.bfloat16, got torch.float32", fn, x.float(), f1, b, f2, b, f3, b4)
    refused(TypeError, "frag2: expected torch.bfloat16, got torch.float32", fn, x, f1, b, f2.float(), b, f3, b4)
    refused(TypeError, "bias3: expected torch.float32, got torch.bfloat16", fn, x, f1, b, f2, b, f3, b4.to(BF16))
    refused(ValueError, f"{who}: needs 4 x 64 or 4 x 128 channels (got 64)", fn, m, f1, b, f2, b, f3, b4)
    refused(ValueError, f"{who}: frag1 / frag2 / frag3 must be pack_conv2d_frag_bf16 of [CM,4CM,1,1] / [CM,CM,3,3] / [4CM,CM,1,1]",
            fn, x, f3, b, f2, b, f3, b4)
    refused(ValueError, f"{who}: frag1 / frag2 / frag3 must be pack_conv2d_frag_bf16 of [CM,4CM,1,1] / [CM,CM,3,3] / [4CM,CM,1,1]",
            fn, x, f1, b, f2, b, f1, b4)
    refused(ValueError, f"{who}: bias shape mismatch", fn, x, f1, b, f2, b4, f3, b4)
    refused(ValueError, f"{who}: out must be (1, 4, 4, 256), got (1, 4, 4, 64)", fn, x, f1, b, f2, b, f3, b4, out=m)
    # projection block: the [1,4,4,64] map is res2.0's input
    f1, f2, f3, fs = frags(z, 64, 64, shortcut=True)
    who, fn = "bottleneck_block_proj_bf16", ops.bottleneck_block_proj_bf16
    refused(TypeError, "frags: expected torch.bfloat16, got torch.float32", fn, m, 1, f1, b, f2, b, f3, b4, fs.float(), b4)
    refused(TypeError, "biass: expected torch.float32, got torch.bfloat16", fn, m, 1, f1, b, f2, b, f3, b4, fs, b4.to(BF16))
    refused(ValueError, f"{who}: built for (CIN, CM, stride) = (64, 64, 1), got (64, 64, 2)", fn, m, 2, f1, b, f2, b, f3, b4, fs, b4)
    refused(ValueError, f"{who}: built for (CIN, CM, stride) = (64, 64, 1), got (256, 64, 1)", fn, x, 1, f1, b, f2, b, f3, b4, fs, b4)
    text = f"{who}: fragment shapes do not match [CM,CIN,1,1] / [CM,CM,3,3] / [4CM,CM,1,1] / [4CM,CIN,1,1]"
    refused(ValueError, text, fn, m, 1, f1, b, f2, b, f3, b4, f1, b4)
    refused(ValueError, text, fn, m, 1, f3, b, f2, b, f3, b4, fs, b4)
    refused(ValueError, f"{who}: bias shape mismatch", fn, m, 1, f1, b, f2, b, f3, b4, fs, b)
    refused(ValueError, f"{who}: out must be (1, 4, 4, 256), got (1, 4, 4, 64)", fn, m, 1, f1, b, f2, b, f3, b4, fs, b4, out=m)
    # residual block: res3.0, 256 -> 128 -> 512 at stride 2
    f1, f2, f3 = frags(z, 256, 128)
    b, b4, res = z(128), z(512), z(1, 2, 2, 512, dtype=BF16)
    who, fn = "bottleneck_block_res_bf16", ops.bottleneck_block_res_bf16
    refused(TypeError, "residual: expected torch.bfloat16, got torch.float32", fn, x, 2, f1, b, f2, b, f3, b4, res.float())
    refused(TypeError, "frag1: expected torch.bfloat16, got torch.float32", fn, x, 2, f1.float(), b, f2, b, f3, b4, res)
    refused(ValueError, f"{who}: built for (CIN, CM, stride) = (256, 128, 2), got (256, 128, 1)", fn, x, 1, f1, b, f2, b, f3, b4, res)
    refused(ValueError, f"{who}: fragment shapes do not match [CM,CIN,1,1] / [CM,CM,3,3] / [4CM,CM,1,1]", fn, x, 2, f1, b, f2, b,
            f1, b4, res)
    refused(ValueError, f"{who}: bias / residual shape mismatch", fn, x, 2, f1, b, f2, b, f3, b, res)
    refused(ValueError, f"{who}: bias / residual shape mismatch", fn, x, 2, f1, b, f2, b, f3, b4, z(1, 4, 4, 512, dtype=BF16))
    refused(ValueError, f"{who}: out must be (1, 2, 2, 512), got (1, 4, 4, 64)", fn, x, 2, f1, b, f2, b, f3, b4, res, out=m)


# ------------------------------------------------------------------------------------------- span entries
S, N, P, J, T, D, K = 1, 2, 1, 1, 4, 16, 3


def span_case(tspn, z, bf16):
    """(who, fn, the nine leading arguments as a dict) of decode_span_relations / its bf16 twin on S=1 N=2 P=1 J=1 T=4 D=16 K=3."""
    a = dict(feats=z(S * N, T, D, dtype=BF16 if bf16 else F32), pairs=z(S, P, 2, dtype=I64), spans=z(S * P, J, 2, dtype=I64),
             span_scores=z(S * P, J), span_counts=z(S * P, dtype=I64))
    if bf16:
        a.update(cls_packed=z(1, 1, 64, 8, dtype=BF16), cls_b=z(K), K=K)
        return "decode_span_relations_bf16", tspn.ops.decode_span_relations_bf16, dict(a, cls_logits=z(S, N, 5))
    a.update(cls_w=z(K, 2 * D), cls_b=z(K))
    return "decode_span_relations", tspn.ops.decode_span_relations, dict(a, cls_logits=z(S, N, 5))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_decode_span_relations_wrappers(tspn, z, bf16):
    who, fn, a = span_case(tspn, z, bf16)
    call = lambda **kw: fn(**dict(a, **kw))
    other = "torch.float32" if bf16 else "torch.bfloat16"
    refused(TypeError, f"feats: expected {a['feats'].dtype}, got {other}", call, feats=a["feats"].to(F32 if bf16 else BF16))
    refused(TypeError, "span_counts: expected torch.int64, got torch.float32", call, span_counts=z(S * P))
    refused(ValueError, f"{who}: pairs must be [S,P,2] and cls_logits [S,N,num_obj]", call, pairs=z(P, 2, dtype=I64))
    refused(ValueError, f"{who}: pairs must be [S,P,2] and cls_logits [S,N,num_obj]", call, cls_logits=z(2, N, 5))
    refused(ValueError, f"{who}: feats must hold S*N = 2 tracklets [S*N,T,D], got (3, 4, 16)", call, feats=z(3, T, D, dtype=a["feats"].dtype))
    refused(ValueError, f"{who}: spans must be [S*P,J,2]", call, spans=z(J, 2, dtype=I64))
    text = f"{who}: spans [S*P,J,2], span_scores [S*P,J] and span_counts [S*P] expected for S*P = 1, J = 1"
    refused(ValueError, text, call, span_scores=z(S * P, 2))
    refused(ValueError, text, call, span_counts=z(2, dtype=I64))
    if bf16:
        text = f"{who}: cls_packed must be pack_span_cls_bf16 of a [K=3, 2D=32] weight and cls_b [K]"
        refused(ValueError, text, call, cls_packed=z(2, 1, 64, 8, dtype=BF16))
        refused(ValueError, text, call, cls_b=z(K + 1))
        refused(ValueError, "the bf16 path needs D % 16 == 0 (D=8)", call, feats=z(S * N, T, 8, dtype=BF16))
        refused(TypeError, "cls_packed: expected torch.bfloat16, got torch.float32", call, cls_packed=z(1, 1, 64, 8))
    else:
        refused(ValueError, f"{who}: cls_w must be [K,2D] and cls_b [K]", call, cls_w=z(K, D))
        refused(ValueError, f"{who}: cls_w must be [K,2D] and cls_b [K]", call, cls_b=z(K + 1))
        refused(TypeError, "cls_w: expected torch.float32, got torch.bfloat16", call, cls_w=z(K, 2 * D, dtype=BF16))
    bad = a["pairs"].clone()
    bad[0, 0, 1] = N
    refused(IndexError, f"{who}: tracklet id outside the segment", call, pairs=bad)
    out = [z(S, 3), z(S, 3, 3, dtype=I64), z(S, 3, 2, dtype=I64), z(S, 3, 2, dtype=I64), z(S, 3, dtype=I64), z(S, dtype=I64)]
    refused(ValueError, f"{who}: out must be the six result tensors", call, out=out[:5])
    refused(ValueError, f"{who}: out.scores must be (1, 3)", call, out=[z(S, 2)] + out[1:])
    refused(ValueError, f"{who}: out.valid must be (1,)", call, out=out[:5] + [z(2, dtype=I64)])
    refused(ValueError, f"{who}: out.triplets must be (1, 1, 3)", call, out=[z(S, 1)] + out[1:], topk_per_span=1)   # Mc = 1
    refused(TypeError, "out.span_rank: expected torch.int64, got torch.float32", call, out=out[:4] + [z(S, 3)] + out[5:])
    # accepted: no pairs at all -- nothing is launched and valid is written as 0
    res = call(pairs=z(S, 0, 2, dtype=I64), spans=z(0, J, 2, dtype=I64), span_scores=z(0, J), span_counts=z(0, dtype=I64))
    assert len(res) == 6 and tuple(res[0].shape) == (S, 0) and res[5].tolist() == [0]
    # and the valid tiny call: one pair with no span left by the NMS (count 0) has no candidate either
    res = call(out=out)
    assert all(r is o for r, o in zip(res, out)) and res[5].tolist() == [0]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_span_predicate_wrappers(tspn, z, bf16):
    ops = tspn.ops
    feats, pairs, spans = z(N, T, D, dtype=BF16 if bf16 else F32), z(P, 2, dtype=I64), z(P, 2, dtype=I64)
    if bf16:
        who, fn, cls = "span_predicate_bf16", ops.span_predicate_bf16, (z(1, 1, 64, 8, dtype=BF16), z(K), K)
        refused(ValueError, f"{who}: feats must be [NT,T,D]", fn, z(T, D, dtype=BF16), pairs, spans, *cls)
        refused(ValueError, f"{who}: out shape mismatch", fn, feats, pairs, spans, *cls, out=z(2, K))
    else:
        who, fn, cls = "span_predicate", ops.span_predicate, (z(K, 2 * D), z(K))
        refused(ValueError, f"{who}: shape mismatch", fn, feats, pairs, spans, z(K, D), z(K))
    refused(ValueError, f"{who}: shape mismatch", fn, feats, pairs, z(2, 2, dtype=I64), *cls)
    refused(ValueError, f"{who}: shape mismatch", fn, feats, z(P, 3, dtype=I64), spans, *cls)
    refused(IndexError, f"{who}: pair index out of range", fn, feats, pairs + N, spans, *cls)
    refused(IndexError, f"{who}: pair index out of range", fn, feats, pairs - 1, spans, *cls)
    out = fn(feats, pairs, spans, *cls)                              # zero features and weights: sigmoid(0)
    assert tuple(out.shape) == (P, K) and (out == 0.5).all()
