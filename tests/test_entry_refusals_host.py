"""The refusals of the C entries whose operand checks live in shared helpers (the stem, the conv2d / max-pool family, the
bottleneck blocks, the span relation decodes), pinned without a GPU: every row is answered by the argument checks or is an
empty-batch early return, so the made-up addresses are never dereferenced and no row reaches a HIP call.  Each refusal row
states the return code and the complete tspn_last_error() text; the doubly wrong rows pin the order of the ladder."""
import ctypes

import pytest

import tspn_mi355x

A = tspn_mi355x._abi
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = A.TSPN_OK, A.TSPN_EINVAL, A.TSPN_EUNSUPPORTED, A.TSPN_EWORKSPACE
p = ctypes.c_void_p
ok, ok2, odd, null = p(0x10000), p(0x20000), p(0x10004), p(0)     # two aligned addresses, a misaligned one, null
BIG = 1 << 40                                                       # a batch no grid can hold


def _stem(name):
    def call(x=ok, NB=1, H=8, W=8, frag=ok, Cout=64, bias=ok, ws=ok, ws_bytes=1 << 30, out=ok2):
        return getattr(A.lib(), name)(x, NB, H, W, frag, Cout, bias, ws, ws_bytes, out, null)
    return call


def _conv(name):
    def call(x=ok, NB=1, H=8, W=8, Cin=64, w=ok, Cout=64, KH=3, KW=3, stride=1, pad=1, bias=ok, residual=ok, out=ok2):
        return getattr(A.lib(), name)(x, NB, H, W, Cin, w, Cout, KH, KW, stride, pad, bias, residual, 1, out, null)
    return call


def _cin4(x=ok, NB=1, H=8, W=8, frag=ok, Cout=64, KH=3, KW=3, stride=1, pad=1, bias=ok, out=ok2):
    return A.lib().tspn_conv2d_nhwc_cin4_f32(x, NB, H, W, frag, Cout, KH, KW, stride, pad, bias, 1, out, null)


def _pool_f32(x=ok, NB=1, H=8, W=8, C=64, k=3, stride=2, pad=1, out=ok2):
    return A.lib().tspn_max_pool_nhwc_f32(x, NB, H, W, C, k, stride, pad, out, 0, null)


def _pool_bf16(x=ok, NB=1, H=8, W=8, C=64, k=3, stride=2, pad=1, out=ok2):
    return A.lib().tspn_max_pool_nhwc_bf16(x, NB, H, W, C, k, stride, pad, out, null)


def _block(x=ok, NB=1, H=8, W=8, CM=64, f1=ok, b1=ok, f2=ok, b2=ok, f3=ok, b3=ok, out=ok2):
    return A.lib().tspn_bottleneck_block_bf16(x, NB, H, W, CM, f1, b1, f2, b2, f3, b3, out, null)


def _proj(x=ok, NB=1, H=8, W=8, CIN=64, stride=1, CM=64, f1=ok, b1=ok, f3=ok, fs=ok, bs=ok, out=ok2):
    return A.lib().tspn_bottleneck_block_proj_bf16(x, NB, H, W, CIN, stride, CM, f1, b1, ok, ok, f3, ok, fs, bs, out, null)


def _res(x=ok, NB=1, H=8, W=8, CIN=256, stride=2, CM=128, f1=ok, b1=ok, f3=ok, residual=ok, out=ok2):
    return A.lib().tspn_bottleneck_block_res_bf16(x, NB, H, W, CIN, stride, CM, f1, b1, ok, ok, f3, ok, residual, out, null)


def _rel(name):
    def call(feats=ok, S=1, N=3, T=5, D=16, P=6, J=2, cls=ok, K=9, R=4, M=16, out_valid=ok2, ws=ok, ws_bytes=1 << 30):
        return getattr(A.lib(), name)(feats, S, N, T, D, ok, P, ok, ok, ok, J, cls, ok, K, ok, 35, R, M,
                                      ok2, ok2, ok2, ok2, ok2, out_valid, ws, ws_bytes, null)
    return call


def _stem_rows(n):
    f = _stem(n)
    return [
        (f, dict(H=0), EINVAL, f"{n}: bad sizes"),
        (f, dict(NB=-1, Cout=48), EINVAL, f"{n}: bad sizes"),
        (f, dict(Cout=48), EUNSUPPORTED, f"{n}: Cout must be 32 or 64 (got 48)"),
        (f, dict(Cout=48, x=null), EUNSUPPORTED, f"{n}: Cout must be 32 or 64 (got 48)"),
        (f, dict(Cout=16, NB=0), EUNSUPPORTED, f"{n}: Cout must be 32 or 64 (got 16)"),
        (f, dict(NB=0, x=null, frag=null, bias=null, ws=null, ws_bytes=0, out=null), OK, n),
        (f, dict(x=null), EINVAL, f"{n}: null pointer"),
        (f, dict(ws=null, ws_bytes=0), EINVAL, f"{n}: null pointer"),
        (f, dict(out=null, H=1 << 20), EINVAL, f"{n}: null pointer"),
        (f, dict(H=1 << 20), EUNSUPPORTED, f"{n}: image too large"),
        (f, dict(NB=BIG), EUNSUPPORTED, f"{n}: image too large"),
        (f, dict(W=1 << 20, ws_bytes=0), EUNSUPPORTED, f"{n}: image too large"),
        (f, dict(ws_bytes=1791), EWORKSPACE, f"{n}: workspace 1791 < 1792 bytes"),
        (f, dict(ws_bytes=1791, frag=odd), EWORKSPACE, f"{n}: workspace 1791 < 1792 bytes"),
        (f, dict(frag=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(bias=odd, Cout=32), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(ws=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(out=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
    ]


def _conv_rows(n, rule):
    f = _conv(n)
    return [
        (f, dict(stride=0), EINVAL, f"{n}: bad sizes"),
        (f, dict(Cin=0, KH=9, KW=8), EINVAL, f"{n}: bad sizes"),
        (f, dict(KH=9, KW=8, pad=4), EUNSUPPORTED, f"{n}: at most 64 taps"),
        (f, dict(KH=9, KW=8, pad=0, x=null), EUNSUPPORTED, f"{n}: at most 64 taps"),
        (f, dict(H=2, W=2, KH=5, KW=5, pad=0), EINVAL, f"{n}: empty output"),
        (f, dict(H=8, W=1, KH=1, KW=3, pad=0, NB=0), EINVAL, f"{n}: empty output"),
        (f, dict(H=2, KH=5, pad=1, x=null, Cin=8), EINVAL, f"{n}: empty output"),
        (f, dict(NB=0, x=null, w=null, bias=null, residual=null, out=null, Cin=8), OK, n),
        (f, dict(x=null), EINVAL, f"{n}: null pointer"),
        (f, dict(w=null, Cin=8), EINVAL, f"{n}: null pointer"),
        (f, dict(out=null, bias=odd), EINVAL, f"{n}: null pointer"),
        (f, dict(Cin=8), EUNSUPPORTED, f"{n}: needs {rule} (Cin=8 Cout=64)"),
        (f, dict(Cout=30, bias=odd), EUNSUPPORTED, f"{n}: needs {rule} (Cin=64 Cout=30)"),
        (f, dict(x=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(bias=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(residual=odd, bias=null, H=1 << 20), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(H=1 << 20), EUNSUPPORTED, f"{n}: dimension too large"),
        (f, dict(Cout=1 << 24, NB=BIG, bias=null, residual=null), EUNSUPPORTED, f"{n}: dimension too large"),
        (f, dict(NB=BIG), EUNSUPPORTED, f"{n}: grid too large"),
    ]


def _cin4_rows():
    n, f = "tspn_conv2d_nhwc_cin4_f32", _cin4
    return [
        (f, dict(stride=0), EINVAL, f"{n}: bad sizes"),
        (f, dict(pad=-1, Cout=48), EINVAL, f"{n}: bad sizes"),
        (f, dict(Cout=48), EUNSUPPORTED, f"{n}: needs at most 64 taps and Cout % 32 == 0"),
        (f, dict(KH=9, KW=8, pad=4, x=null), EUNSUPPORTED, f"{n}: needs at most 64 taps and Cout % 32 == 0"),
        (f, dict(H=2, W=2, KH=5, KW=5, pad=0), EINVAL, f"{n}: empty output"),
        (f, dict(W=1, KW=7, pad=2, NB=0), EINVAL, f"{n}: empty output"),
        (f, dict(NB=0, x=null, frag=null, bias=null, out=null), OK, n),
        (f, dict(x=null), EINVAL, f"{n}: null pointer"),
        (f, dict(out=null, frag=odd), EINVAL, f"{n}: null pointer"),
        (f, dict(frag=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(bias=odd, H=1 << 20), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(H=1 << 20, bias=null), EUNSUPPORTED, f"{n}: problem too large"),
        (f, dict(NB=BIG), EUNSUPPORTED, f"{n}: problem too large"),
    ]


def _pool_rows(n, f, c_bad, c_rule):
    return [
        (f, dict(pad=2), EINVAL, f"{n}: bad sizes"),
        (f, dict(C=0, x=null), EINVAL, f"{n}: bad sizes"),
        (f, dict(H=1, W=1, k=5, pad=1), EINVAL, f"{n}: empty output"),
        (f, dict(W=2, k=5, pad=1, x=null, NB=0), EINVAL, f"{n}: empty output"),
        (f, dict(NB=0, x=null, out=null, C=c_bad), OK, n),
        (f, dict(x=null), EINVAL, f"{n}: null pointer"),
        (f, dict(out=null, C=c_bad), EINVAL, f"{n}: null pointer"),
        (f, dict(C=c_bad), EUNSUPPORTED, f"{n}: needs {c_rule} and 16-byte aligned tensors"),
        (f, dict(x=odd), EUNSUPPORTED, f"{n}: needs {c_rule} and 16-byte aligned tensors"),
        (f, dict(out=odd), EUNSUPPORTED, f"{n}: needs {c_rule} and 16-byte aligned tensors"),
    ]


def _block_rows():
    n, f = "tspn_bottleneck_block_bf16", _block
    rows = [
        (f, dict(H=0), EINVAL, f"{n}: bad sizes"),
        (f, dict(W=0, CM=96), EINVAL, f"{n}: bad sizes"),
        (f, dict(CM=96), EUNSUPPORTED, f"{n}: bottleneck channels must be 64 or 128 (got 96)"),
        (f, dict(CM=256, x=null, NB=0), EUNSUPPORTED, f"{n}: bottleneck channels must be 64 or 128 (got 256)"),
        (f, dict(NB=0, x=null, f1=null, b1=null, f2=null, b2=null, f3=null, b3=null, out=null), OK, n),
        (f, dict(x=null), EINVAL, f"{n}: null pointer"),
        (f, dict(b3=null, out=ok), EINVAL, f"{n}: null pointer"),
        (f, dict(out=ok), EINVAL, f"{n}: the block cannot run in place (tiles read their neighbours' pixels)"),
        (f, dict(out=ok, b1=odd, CM=128), EINVAL, f"{n}: the block cannot run in place (tiles read their neighbours' pixels)"),
        (f, dict(b1=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(out=odd, H=1 << 12, W=1 << 12, CM=128), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
        (f, dict(H=1 << 12, W=1 << 12, CM=128), EUNSUPPORTED, f"{n}: one image's map must stay below 2 GB"),
        (f, dict(H=1 << 12, W=1 << 12, NB=BIG), EUNSUPPORTED, f"{n}: one image's map must stay below 2 GB"),
        (f, dict(NB=BIG), EUNSUPPORTED, f"{n}: grid too large"),
        (f, dict(NB=BIG, CM=128), EUNSUPPORTED, f"{n}: grid too large"),
    ]
    for n, f, built, bad, got in (
            ("tspn_bottleneck_block_proj_bf16", _proj, "res2 (64 -> 64 -> 256, stride 1)", dict(CIN=128), "CIN=128 CM=64 stride=1"),
            ("tspn_bottleneck_block_res_bf16", _res, "res3 (256 -> 128 -> 512, stride 2)", dict(stride=1), "CIN=256 CM=128 stride=1")):
        refusal = f"{n}: built for the first block of {built}; got {got}"
        rows += [
            (f, dict(H=0), EINVAL, f"{n}: bad sizes"),
            (f, dict(NB=-1, **bad), EINVAL, f"{n}: bad sizes"),
            (f, bad, EUNSUPPORTED, refusal),
            (f, dict(x=null, NB=0, **bad), EUNSUPPORTED, refusal),
            (f, dict(NB=0, x=null, f1=null, b1=null, f3=null, out=null), OK, n),
            (f, dict(x=null), EINVAL, f"{n}: null pointer"),
            (f, dict(f3=null, b1=odd), EINVAL, f"{n}: null pointer"),
            (f, dict(b1=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
            (f, dict(out=odd, H=1 << 13, W=1 << 13), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned"),
            (f, dict(H=1 << 13, W=1 << 13), EUNSUPPORTED, f"{n}: one image's maps must stay below 2 GB"),
            (f, dict(H=1 << 13, W=1 << 13, NB=BIG), EUNSUPPORTED, f"{n}: one image's maps must stay below 2 GB"),
            (f, dict(NB=BIG), EUNSUPPORTED, f"{n}: grid too large"),
        ]
    n = "tspn_bottleneck_block_proj_bf16"
    rows += [(_proj, dict(fs=null), EINVAL, f"{n}: null pointer"),
             (_proj, dict(bs=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned")]
    n = "tspn_bottleneck_block_res_bf16"
    rows += [(_res, dict(residual=null, out=null), EINVAL, f"{n}: null pointer"),
             (_res, dict(residual=ok2), EINVAL, f"{n}: out must not alias the residual"),
             (_res, dict(residual=ok2, b1=odd), EINVAL, f"{n}: out must not alias the residual"),
             (_res, dict(residual=odd), EUNSUPPORTED, f"{n}: operands must be 16-byte aligned")]
    return rows


def _rel_rows(n, bf16):
    f = _rel(n)
    sizes = "S=1 N=3 T={T} D={D} P=6 J=2 K={K} NO=35"
    rows = [
        (f, dict(T=0), EINVAL, f"{n}: bad sizes " + sizes.format(T=0, D=16, K=9)),
        (f, dict(T=0, K=257, D=24), EINVAL, f"{n}: bad sizes " + sizes.format(T=0, D=24, K=257)),
        (f, dict(K=257), EUNSUPPORTED, f"{n}: K=257 > 256"),
        (f, dict(K=257, M=1025, J=17), EUNSUPPORTED, f"{n}: K=257 > 256"),
        (f, dict(M=1025), EUNSUPPORTED, f"{n}: topk_per_seg=1025 > 1024"),
        (f, dict(M=1025, J=17, feats=null), EUNSUPPORTED, f"{n}: topk_per_seg=1025 > 1024"),
        (f, dict(J=17), EUNSUPPORTED, f"{n}: spans_per_pair J=17 > 16"),
        (f, dict(J=17, S=0, feats=null), EUNSUPPORTED, f"{n}: spans_per_pair J=17 > 16"),
        (f, dict(P=1 << 24, J=16, R=8, K=8), EUNSUPPORTED, f"{n}: P*J*topk_per_span = 2147483648 candidates per segment"),
        (f, dict(P=1 << 24, J=16, R=9, K=8, N=0), EUNSUPPORTED, f"{n}: P*J*topk_per_span = 2147483648 candidates per segment"),
        (f, dict(S=0, feats=null, cls=null, out_valid=null, ws=null, ws_bytes=0), OK, n),
        (f, dict(P=0, N=0, feats=null, cls=null, out_valid=null, ws=null, ws_bytes=0), OK, n),
        (f, dict(N=0), EINVAL, f"{n}: pairs without tracklets"),
        (f, dict(N=0, feats=null, ws_bytes=0), EINVAL, f"{n}: pairs without tracklets"),
        (f, dict(feats=null), EINVAL, f"{n}: null pointer"),
        (f, dict(cls=null), EINVAL, f"{n}: null pointer"),
        (f, dict(out_valid=null, ws_bytes=0), EINVAL, f"{n}: null pointer"),
    ]
    if bf16:
        big = dict(S=1 << 20, N=1 << 20)
        rows += [
            (f, dict(D=24), EUNSUPPORTED, f"{n}: needs D % 16 == 0 (D=24)"),
            (f, dict(D=8, K=257), EUNSUPPORTED, f"{n}: needs D % 16 == 0 (D=8)"),
            (f, dict(D=40, S=0), EUNSUPPORTED, f"{n}: needs D % 16 == 0 (D=40)"),
            (f, big, EUNSUPPORTED, f"{n}: problem too large"),
            (f, dict(feats=null, **big), EUNSUPPORTED, f"{n}: problem too large"),
            (f, dict(feats=odd), EUNSUPPORTED, f"{n}: unaligned pointer (feats and cls_packed need 16 bytes)"),
            (f, dict(cls=odd, ws_bytes=0), EUNSUPPORTED, f"{n}: unaligned pointer (feats and cls_packed need 16 bytes)"),
            (f, dict(ws_bytes=4351), EWORKSPACE, f"{n}: workspace 4351 < 4352 bytes"),
            (f, dict(ws=null), EWORKSPACE, f"{n}: workspace 1073741824 < 4352 bytes"),
            (f, dict(ws=p(0x10010), ws_bytes=16), EWORKSPACE, f"{n}: workspace 16 < 4352 bytes"),
            (f, dict(ws=p(0x10010)), EUNSUPPORTED, f"{n}: unaligned pointer (the workspace needs 256 bytes)"),
        ]
    else:
        rows += [
            (f, dict(D=24, ws_bytes=0), EWORKSPACE, f"{n}: workspace 0 < 6144 bytes"),      # no D rule on the fp32 entry
            (f, dict(ws_bytes=6143), EWORKSPACE, f"{n}: workspace 6143 < 6144 bytes"),
            (f, dict(ws=null), EWORKSPACE, f"{n}: workspace 1073741824 < 6144 bytes"),
            (f, dict(ws_bytes=6143, S=1 << 13, N=1, P=1 << 20, J=1, R=1), EWORKSPACE,
             f"{n}: workspace 6143 < 103092191232 bytes"),
            (f, dict(ws_bytes=1 << 62, S=1 << 13, N=1, P=1 << 20, J=1, R=1), EUNSUPPORTED, f"{n}: grid too large"),
        ]
    return rows


ROWS = (_stem_rows("tspn_stem_conv_bf16") + _stem_rows("tspn_stem_pool_bf16") +
        _conv_rows("tspn_conv2d_nhwc_f32", "Cin % 16 == 0 and Cout % 4 == 0") +
        _conv_rows("tspn_conv2d_nhwc_frag_f32", "Cin % 16 == 0 and Cout % 32 == 0") +
        _conv_rows("tspn_conv2d_nhwc_bf16", "Cin % 64 == 0 and Cout % 32 == 0") + _cin4_rows() +
        _pool_rows("tspn_max_pool_nhwc_f32", _pool_f32, 6, "C % 4 == 0") +
        _pool_rows("tspn_max_pool_nhwc_bf16", _pool_bf16, 12, "C % 8 == 0") + _block_rows() +
        _rel_rows("tspn_decode_span_relations_f32", False) + _rel_rows("tspn_decode_span_relations_bf16", True) + [
    # what only one of the twins has
    (_conv("tspn_conv2d_nhwc_bf16"), dict(H=1 << 15, W=1 << 15), EUNSUPPORTED,
     "tspn_conv2d_nhwc_bf16: the images one 128-pixel tile spans must stay below 2 GB (H=32768 W=32768 Cin=64)"),
    (_conv("tspn_conv2d_nhwc_bf16"), dict(H=1 << 15, W=1 << 15, NB=BIG), EUNSUPPORTED,
     "tspn_conv2d_nhwc_bf16: the images one 128-pixel tile spans must stay below 2 GB (H=32768 W=32768 Cin=64)"),
    (_conv("tspn_conv2d_nhwc_f32"), dict(Cout=36, bias=null, residual=null, NB=BIG), EUNSUPPORTED,
     "tspn_conv2d_nhwc_f32: grid too large"),                       # Cout % 4 is enough for the fp32 entry alone
])


def _entry(text):
    return text.split(":")[0]


@pytest.mark.parametrize("entry", sorted({_entry(r[3]) for r in ROWS}))
def test_refusals_are_answered_without_a_device(entry):
    lib = A.lib()
    for call, kwargs, code, text in ROWS:
        if _entry(text) != entry:
            continue
        rc = call(**kwargs)
        assert rc == code, (kwargs, rc, lib.tspn_last_error().decode())
        if code != OK:             # (an accepted call leaves the last error alone; its row carries the entry's name only)
            assert lib.tspn_last_error().decode() == text, kwargs


def test_the_table_pins_every_entry_s_order_and_its_empty_batch():
    """Per entry: at least two doubly wrong calls (two or more arguments off their defaults, refused) and the empty batch
    with null operands."""
    entries = {_entry(r[3]) for r in ROWS}
    assert len(entries) == 13, sorted(entries)
    for entry in entries:
        rows = [r for r in ROWS if _entry(r[3]) == entry]
        assert sum(1 for _, kw, code, _ in rows if code != OK and len(kw) >= 2) >= 2, entry
        assert any(code == OK and null in kw.values() for _, kw, code, _ in rows), entry
