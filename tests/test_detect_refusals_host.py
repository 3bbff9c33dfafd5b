"""Return code and whole tspn_last_error() text of every refusal of the detector entries (csrc/detect/tspn_detect.hip).
Every refusal comes from the argument checks, before any launch: the device pointers are made-up addresses, and no
device is needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def env():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    return abi, abi.lib()


vp = ctypes.c_void_p
OK, NULL, ODD4, ODD1 = vp(0x10000), vp(0), vp(0x10004), vp(0x10001)


def offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_box_nms_refusals(env):
    A_, lib = env
    w = "tspn_box_nms_f32: "

    def nms(n=300, off=(0, 100, 100, 300), G=None, pre=128, thr=0.5, post=50, min_size=0.0, boxes=OK, scores=OK, valid=NULL,
            index=OK, count=OK, keep=NULL, scratch=OK, nbytes=1 << 30):
        arr = None if off is None else offs(*off)
        G = (len(off) - 1 if off is not None else 3) if G is None else G
        rc = lib.tspn_box_nms_f32(boxes, scores, valid, n, arr, G, pre, thr, post, min_size, index, count, keep, scratch, nbytes,
                                  None)
        return rc, lib.tspn_last_error().decode()

    # sizes first
    assert nms(n=-1) == (A_.TSPN_EINVAL, w + "bad sizes n=-1 G=3 pre_topk=128 post_topk=50")
    assert nms(G=-2) == (A_.TSPN_EINVAL, w + "bad sizes n=300 G=-2 pre_topk=128 post_topk=50")
    assert nms(pre=0) == (A_.TSPN_EINVAL, w + "bad sizes n=300 G=3 pre_topk=0 post_topk=50")
    assert nms(post=0) == (A_.TSPN_EINVAL, w + "bad sizes n=300 G=3 pre_topk=128 post_topk=0")
    # then the limits
    assert nms(pre=8193, post=8193) == (A_.TSPN_EUNSUPPORTED, w + "pre_topk=8193 > 8192")
    assert nms(pre=8192, post=8192, scratch=NULL)[0] == A_.TSPN_EWORKSPACE              # 8192 itself is served
    assert nms(post=129) == (A_.TSPN_EUNSUPPORTED, w + "post_topk=129 > pre_topk=128")
    assert nms(n=2 ** 31, off=(0, 2 ** 31)) == (A_.TSPN_EUNSUPPORTED, w + "n=2147483648 G=1 (needs n < 2^31, G < 2^24)")
    # then the groups, read on the host
    assert nms(off=None) == (A_.TSPN_EINVAL, w + "null pointer")
    bad = w + "group_off must ascend from 0 to n=300"
    assert nms(off=(0, 200, 100, 300)) == (A_.TSPN_EINVAL, bad)                         # unsorted
    assert nms(off=(1, 100, 100, 300)) == (A_.TSPN_EINVAL, bad)                         # does not start at 0
    assert nms(off=(0, 100, 100, 299)) == (A_.TSPN_EINVAL, bad)                         # does not end at n
    assert nms(off=(0, 100, 100, 301)) == (A_.TSPN_EINVAL, bad)
    # then the operands
    for name in ("scores", "index", "count"):
        assert nms(**{name: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), name
    only = w + "the selection alone (boxes == null) takes no validity array and writes no keep bytes"
    assert nms(boxes=NULL, valid=OK) == (A_.TSPN_EINVAL, only) and nms(boxes=NULL, keep=OK) == (A_.TSPN_EINVAL, only)
    assert nms(thr=float("nan")) == nms(min_size=float("nan")) == (A_.TSPN_EINVAL, w + "iou_threshold and min_size must be numbers")
    assert nms(boxes=NULL, thr=float("nan"), scratch=NULL)[0] == A_.TSPN_EWORKSPACE     # not read by the selection alone
    align = w + "boxes and scratch must be 16-byte aligned, the outputs 8-byte aligned"
    for name in ("boxes", "scratch", "index", "count"):
        assert nms(**{name: ODD4}) == (A_.TSPN_EUNSUPPORTED, align), name
    assert nms(scores=ODD1) == (A_.TSPN_EUNSUPPORTED, align)
    # the scratch last: short, or none at all
    need = lib.tspn_box_nms_scratch_bytes(offs(0, 100, 100, 300), 3, 128, 0)
    # offsets 4 x 8 -> 256, counts 3 x 4 -> 256, indices 3 x 128 x 4, boxes 3 x 128 x 16, words 3 x 128 x 2 x 8
    assert need == 256 + 256 + 1536 + 6144 + 6144
    assert nms(nbytes=need - 1) == (A_.TSPN_EWORKSPACE, w + f"scratch {need - 1} < {need} bytes")
    assert nms(nbytes=0) == (A_.TSPN_EWORKSPACE, w + f"scratch 0 < {need} bytes")
    assert nms(scratch=NULL) == (A_.TSPN_EWORKSPACE, w + f"scratch 0 < {need} bytes")
    assert lib.tspn_box_nms_scratch_bytes(offs(0, 100, 100, 300), 3, 128, 1) == 256
    assert nms(boxes=NULL, nbytes=255) == (A_.TSPN_EWORKSPACE, w + "scratch 255 < 256 bytes")
    # the order of the checks decides which error a doubly wrong call gets
    assert "bad sizes" in nms(n=-1, pre=9000)[1] and "pre_topk=9000" in nms(pre=9000, post=9001)[1]
    assert "group_off" in nms(off=(0, 200, 100, 300), scores=NULL)[1] and "null pointer" in nms(scores=NULL, scratch=NULL)[1]
    # no group: nothing to do, no pointer needed
    assert nms(n=0, off=(0,), boxes=NULL, scores=NULL, index=NULL, count=NULL, scratch=NULL, nbytes=0)[0] == A_.TSPN_OK
    # what the query answers for the shapes the entry refuses
    q = lib.tspn_box_nms_scratch_bytes
    assert q(offs(0, 100, 100, 300), 3, 8193, 0) == 0 and q(offs(0, 200, 100, 300), 3, 128, 0) == 0
    assert q(None, 3, 128, 0) == 0 and q(offs(0, 5), -1, 128, 0) == 0 and q(offs(0,), 0, 128, 0) == 0
    # the capacity is the largest group, cut at pre_topk
    assert q(offs(0, 8192), 1, 8192, 0) == 256 + 256 + 8192 * 4 + 8192 * 16 + 8192 * 128 * 8
    assert q(offs(0, 70, 100000), 2, 8192, 0) == q(offs(0, 8192, 8262), 2, 8192, 0)


def test_rpn_decode_refusals(env):
    A_, lib = env
    w = "tspn_rpn_decode_f32: "
    names = ("logits", "deltas", "cell", "sizes")
    outs = ("boxes", "out_logits", "valid")

    def dec(B=2, H=3, W=5, A=15, M=40, stride=16.0, cand=OK, **ptr):
        rc = lib.tspn_rpn_decode_f32(cand, *[ptr.get(n, OK) for n in names], B, H, W, A, M, stride,
                                     *[ptr.get(n, OK) for n in outs], None)
        return rc, lib.tspn_last_error().decode()

    assert dec(B=-1) == (A_.TSPN_EINVAL, w + "bad sizes B=-1 H=3 W=5 A=15 M=40")
    assert dec(H=0) == (A_.TSPN_EINVAL, w + "bad sizes B=2 H=0 W=5 A=15 M=40")
    assert dec(A=0)[0] == dec(W=-3)[0] == dec(M=-1)[0] == A_.TSPN_EINVAL
    assert dec(H=2 ** 20) == dec(A=1024) == dec(H=2 ** 12, W=2 ** 12, A=128) == (A_.TSPN_EUNSUPPORTED, w + "dimension too large")
    assert dec(cand=NULL) == (A_.TSPN_EINVAL, w + "without candidates M must be H*W*A=225 (got 40)")
    assert dec(stride=0.0) == dec(stride=float("nan")) == (A_.TSPN_EINVAL, w + "stride must be positive")
    for n in names + outs:
        assert dec(**{n: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    assert dec(boxes=ODD4) == (A_.TSPN_EUNSUPPORTED, w + "out_boxes must be 16-byte aligned")
    # (the other operands are read element by element: a slice such as image_sizes[1:] is served)
    nothing = {n: NULL for n in names + outs}
    assert dec(B=0, cand=NULL, M=225, **nothing)[0] == dec(M=0, **nothing)[0] == A_.TSPN_OK


def test_box_head_decode_refusals(env):
    A_, lib = env
    w = "tspn_box_head_decode_f32: "
    names = ("cls", "deltas", "proposals", "count", "sizes")
    outs = ("scores", "boxes", "valid")

    def dec(B=2, R=65, K=35, weights=(10.0, 10.0, 5.0, 5.0), thr=0.05, **ptr):
        rc = lib.tspn_box_head_decode_f32(*[ptr.get(n, OK) for n in names], B, R, K, *weights, thr,
                                          *[ptr.get(n, OK) for n in outs], None)
        return rc, lib.tspn_last_error().decode()

    assert dec(B=-1) == (A_.TSPN_EINVAL, w + "bad sizes B=-1 R=65 K=35")
    assert dec(K=0) == (A_.TSPN_EINVAL, w + "bad sizes B=2 R=65 K=0")
    assert dec(R=-1)[0] == A_.TSPN_EINVAL
    assert dec(K=2 ** 16) == dec(B=2 ** 20, R=2 ** 10, K=2) == (A_.TSPN_EUNSUPPORTED, w + "dimension too large")
    rule = w + "weights must be positive and score_thresh a number"
    assert dec(weights=(10.0, 0.0, 5.0, 5.0)) == dec(weights=(10.0, 10.0, 5.0, float("nan"))) == (A_.TSPN_EINVAL, rule)
    assert dec(thr=float("nan")) == (A_.TSPN_EINVAL, rule)
    for n in names + outs:
        assert dec(**{n: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    for n in ("proposals", "boxes"):
        assert dec(**{n: ODD4}) == (A_.TSPN_EUNSUPPORTED, w + "proposals and out_boxes must be 16-byte aligned"), n
    nothing = {n: NULL for n in names + outs}
    assert dec(B=0, **nothing)[0] == dec(R=0, **nothing)[0] == A_.TSPN_OK


def test_detections_topk_refusals(env):
    A_, lib = env
    w = "tspn_detections_topk_f32: "
    names = ("scores", "boxes", "keep")
    outs = ("out_boxes", "out_scores", "classes", "count")

    def top(B=2, K=35, R=65, D=100, **ptr):
        rc = lib.tspn_detections_topk_f32(*[ptr.get(n, OK) for n in names], B, K, R, D, *[ptr.get(n, OK) for n in outs], None)
        return rc, lib.tspn_last_error().decode()

    assert top(B=-1) == (A_.TSPN_EINVAL, w + "bad sizes B=-1 K=35 R=65 D=100")
    assert top(D=0) == (A_.TSPN_EINVAL, w + "bad sizes B=2 K=35 R=65 D=0")
    assert top(K=0)[0] == top(R=-1)[0] == A_.TSPN_EINVAL
    assert top(D=1025) == (A_.TSPN_EUNSUPPORTED, w + "D=1025 > 1024")
    assert top(K=2 ** 16, R=2 ** 15) == (A_.TSPN_EUNSUPPORTED, w + "dimension too large")
    for n in names + outs:
        assert top(**{n: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    for n in ("boxes", "out_boxes"):
        assert top(**{n: ODD4}) == (A_.TSPN_EUNSUPPORTED, w + "operands must be 16-byte aligned"), n
    assert top(B=0, **{n: NULL for n in names + outs})[0] == A_.TSPN_OK


def test_wrappers_refuse_before_the_library(env):
    import tspn_mi355x
    ops = tspn_mi355x.ops
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.box_nms(torch.zeros(4, 4), torch.zeros(4), [0, 4], 4, 0.5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rpn_proposals(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 12), torch.zeros(3, 4), 16, torch.zeros(1, 2))
    assert ops.box_nms_workspace_bytes([0, 100, 100, 300], 128) == 256 + 256 + 1536 + 6144 + 6144
    assert ops.box_nms_workspace_bytes(range(0, 4 * 50, 50), 9000) == 0
