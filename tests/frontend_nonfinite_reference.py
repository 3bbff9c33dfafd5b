"""Float64 references and planted inputs of tests/test_gpu_nonfinite_frontend.py (DESIGN.md §2 "Non-finite values", the
front-end bullet), kept apart from it so that tests/test_frontend_nonfinite_host.py can check the references, and the
conditions that keep a case from passing emptily, without a card.

conv2d_ref multiplies and sums elementwise (no BLAS, no library conv): Inf * 0 = NaN holds in it by construction, like
conv_ref of tests/test_gpu_nonfinite.py.  The ReLU is relu64 of that file (NaN stays NaN, relu(-Inf) = 0), the pool is a
NaN-propagating maximum over the window's in-image positions, and conv2d_bf16_ref has the rounding points of
oracle.roi_head_oracle.conv2d_bf16: x, w and the residual are bf16 values, the sum and the fp32 bias are added in
float64, act(...) is rounded to bf16 once.  Everything is channels-last."""
import functools

import numpy as np
import torch

from test_gpu_nonfinite import (NAN_NEG, NAN_NEG_PAY, NAN_PAY, NAN_POS, NANS, assert_same_nonfinite,  # noqa: F401
                                assert_scores_equal, relu64)

INF = np.float32(np.inf)
# (name, value, is an infinity) of the planted values; "inf0" is +Inf meeting one zero weight
PLANTS = [("nan+", NAN_POS, False), ("nan-", NAN_NEG, False), ("snan+", NAN_PAY, False), ("nan-pay", NAN_NEG_PAY, False),
          ("+inf", INF, True), ("-inf", -INF, True), ("inf0", INF, True)]
PLANT_IDS = [p[0] for p in PLANTS]
# the same encodings as bf16 bit patterns (a signalling fp32 payload below bit 16 would be lost by truncation)
BF16_BITS = {"nan+": 0x7fc0, "nan-": 0xffc0, "snan+": 0x7f81, "nan-pay": 0xffeb, "+inf": 0x7f80, "-inf": 0xff80,
             "inf0": 0x7f80}


def t(a):
    return torch.from_numpy(np.array(a))


def r16(a):
    """array -> the same values rounded to bf16 (through fp32, as the oracle's _r16), as float64."""
    with np.errstate(invalid="ignore"):                 # (numpy warns when a cast meets a signalling NaN)
        return t(np.asarray(a, np.float64)).float().to(torch.bfloat16).double().numpy()


def bf16_value(name):
    """The planted bf16 encoding `name` as a float32 scalar (NaN payload kept)."""
    return np.array([BF16_BITS[name] << 16], dtype=np.uint32).view(np.float32)[0]


def to_bf16(a):
    """float32 array whose values are bf16 values -> torch bf16 tensor with the SAME bits (NaN payloads kept)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = (a.view(np.uint32) >> 16).astype(np.uint16)
    assert ((a.view(np.uint32) & 0xffff) == 0).all(), "not bf16 values"
    return torch.from_numpy(hi.view(np.int16).copy()).view(torch.bfloat16).reshape(a.shape)


def out_dim(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv2d_ref(x, w, bias=None, stride=1, pad=0, residual=None, relu=False):
    """x [NB,H,W,Cin], w [Cout,Cin,KH,KW] -> float64 [NB,OH,OW,Cout] = act(conv + bias + residual): every product is
    formed and summed elementwise over (tap, channel); zero padding; relu64."""
    with np.errstate(invalid="ignore"):
        x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    NB, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = out_dim(H, KH, stride, pad), out_dim(W, KW, stride, pad)
    xp = np.zeros((NB, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((NB * OH * OW, Cout))
    step = max(1, (1 << 22) // (Cin * Cout))            # pixels per slab: 32 MB of products at a time
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(KH):
            for b in range(KW):
                xs = xp[:, a:a + stride * (OH - 1) + 1:stride, b:b + stride * (OW - 1) + 1:stride].reshape(-1, Cin)
                wt = w[:, :, a, b]                      # [Cout, Cin]
                for i in range(0, xs.shape[0], step):
                    y[i:i + step] += (xs[i:i + step, None, :] * wt[None]).sum(axis=2)
        y = y.reshape(NB, OH, OW, Cout)
        if bias is not None:
            y = y + np.asarray(bias, np.float64)
        if residual is not None:
            y = y + np.asarray(residual, np.float64)
    return relu64(y) if relu else y


def conv2d_bf16_ref(x, w, bias=None, stride=1, pad=0, residual=None, relu=False):
    """conv2d_ref at the rounding points of roi_head_oracle.conv2d_bf16; returns float64 holding bf16 values."""
    y = conv2d_ref(r16(x), r16(w), None if bias is None else np.asarray(bias, np.float32), stride, pad,
                   None if residual is None else r16(residual), relu)
    return r16(y)


def max_pool_ref(x, k, stride, pad):
    """torch's max_pool2d on [NB,H,W,C]: a NaN in the window gives NaN, padding positions do not take part (-inf)."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x, np.float64)
    NB, H, W, C = x.shape
    OH, OW = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
    xp = np.full((NB, H + 2 * pad, W + 2 * pad, C), -np.inf)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.full((NB, OH, OW, C), -np.inf)
    for a in range(k):
        for b in range(k):
            y = np.maximum(y, xp[:, a:a + stride * (OH - 1) + 1:stride, b:b + stride * (OW - 1) + 1:stride])   # NaN wins
    return y


def same_bits(a, b):
    """Elementwise: float64 arrays a, b hold the same value bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def untouched(ref_planted, ref_clean):
    """Where the reference of the planted input is bit-equal to the reference of the clean input and finite: the
    outputs whose receptive field holds no planted value."""
    return same_bits(ref_planted, ref_clean) & np.isfinite(ref_clean)


def check_not_empty(ref_planted, ref_clean, inf_planted, what, share=0.5):
    """The conditions that keep an op-level case from passing emptily (reference alone, no card)."""
    assert np.isfinite(ref_clean).all(), f"{what}: the clean reference is not finite"
    assert np.isnan(ref_planted).any(), f"{what}: no NaN in the planted reference"
    if inf_planted:
        assert np.isinf(ref_planted).any(), f"{what}: an infinity was planted, none came out"
    keep = float(untouched(ref_planted, ref_clean).mean())
    assert keep >= share, f"{what}: only {keep:.1%} of the outputs stay finite and unchanged"


def assert_confined(got_planted, got_clean, ref_planted, ref_clean, what):
    """Confinement: outputs whose reference did not change have, on the GPU, the bits of the clean launch."""
    keep = untouched(ref_planted, ref_clean)
    gp, gc = np.asarray(got_planted, np.float32), np.asarray(got_clean, np.float32)
    bad = np.argwhere((gp.view(np.uint32) != gc.view(np.uint32)) & keep)
    assert bad.size == 0, f"{what}: {len(bad)} outputs outside every planted value's receptive field changed, first " \
                          f"{bad[:5].tolist()} ({gp[tuple(bad[0])]} for {gc[tuple(bad[0])]})"


def nonzero_normal(rng, seed, tag, shape, std):
    """Normal weights with no zero among them, as test_an_infinity_reaches_exactly_the_windows_that_hold_it draws them
    (a weight drawn as exactly zero becomes 0.125): Inf * w is an infinity wherever the case did not plant a zero."""
    w = rng.normal(seed, tag, shape, std=std)
    return np.where(w == 0, np.float32(0.125), w).astype(np.float32)


def hashrng():
    import tspn_mi355x
    return tspn_mi355x.hashrng


# ------------------------------------------------------------------------------------------------ op-level cases
def plant(x, sites, name, value, bf16):
    """A copy of x with `value` at every site (an index tuple).  bf16: x holds bf16 values, the planted encoding is
    the bf16 one of BF16_BITS."""
    x = np.array(x, dtype=np.float32)
    v = bf16_value(name) if bf16 else value
    for s in sites:
        x[s] = v
    return x


@functools.lru_cache(maxsize=None)
def conv_case(form, plant_name):
    """(g, x, xp, w, b, r, ref_clean, ref_planted) of the conv2d rule case of `form`: generic, frag, frag_res
    (residual epilogue), bf16 <MI, RNG> as bf16-1-0 .. bf16-2-1, cin4.  One geometry of tests/conv2d_edge_cases.py each;
    relu = True, a residual where the entry has one.  The planted value sits in x (first image, the centre pixel, channel
    1) and in the residual (last image, last pixel, channel 2; none for cin4); pixel (1, 1) of the last image holds +Inf
    beside a planted NaN and a NaN beside a planted infinity, so that every case has both.  inf0: w[0, 1] = 0 at every tap."""
    import conv2d_edge_cases as ce
    geoms = {"generic": ("generic", 16, 4, ce.Geom(3, 3, 1, 1, 5, 4)), "frag": ("frag", 16, 32, ce.Geom(3, 1, 2, 1, 6, 7)),
             "frag_res": ("frag", 16, 32, ce.Geom(3, 3, 1, 1, 5, 4)),
             "bf16-1-0": ("bf16", 64, 32, ce.Geom(3, 1, 2, 1, 6, 7)), "bf16-1-1": ("bf16", 64, 32, ce.Geom(3, 3, 1, 1, 5, 4)),
             "bf16-2-0": ("bf16", 64, 64, ce.Geom(2, 3, 1, 1, 5, 4)), "bf16-2-1": ("bf16", 64, 64, ce.Geom(3, 3, 1, 1, 5, 4)),
             "cin4": ("cin4", 3, 32, ce.Geom(7, 7, 2, 3, 9, 10))}
    kind, cin, cout, g = geoms[form]
    nb = 3
    rng = hashrng()
    bf = kind == "bf16"
    oh, ow = ce.out_hw(g)
    x = rng.uniform(1701, "x" + form, (nb, g.H, g.W, cin), -1, 1)
    w = nonzero_normal(rng, 1701, "w" + form, (cout, cin, g.KH, g.KW), 0.1)
    b = rng.normal(1701, "b" + form, (cout,), std=0.1)
    r = None if kind == "cin4" else rng.uniform(1701, "r" + form, (nb, oh, ow, cout), -1, 1)
    if bf:
        x, w, r = (r16(a).astype(np.float32) for a in (x, w, r))
    if plant_name == "inf0":
        w[0, 1] = 0.0
    value, is_inf = dict((n, (v, i)) for n, v, i in PLANTS)[plant_name]
    other = ("nan-", NAN_NEG) if is_inf else ("+inf", INF)      # every case holds a NaN and an infinity
    xp = plant(x, [(0, g.H // 2, g.W // 2, 1)], plant_name, value, bf)
    xp = plant(xp, [(nb - 1, 1, 1, 2)], other[0], other[1], bf)        # (1, 1): read at every stride used here
    rp = None if r is None else plant(r, [(nb - 1, oh - 1, ow - 1, 2)], plant_name, value, bf)
    fn = conv2d_bf16_ref if bf else conv2d_ref
    ref_c = fn(x, w, b, g.stride, g.pad, r, True)
    ref_p = fn(xp, w, b, g.stride, g.pad, rp, True)
    return kind, g, x, xp, w, b, r, rp, ref_c, ref_p


CONV_FORMS = ["generic", "frag", "frag_res", "bf16-1-0", "bf16-1-1", "bf16-2-0", "bf16-2-1", "cin4"]

POOL_MAPS = [(1, 1, 1), (1, 1, 2), (2, 5, 7)]              # (NB, H, W): one pixel, two pixels, 5 x 7
POOL_C = [64, 72]
POOL_KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (1, 1, 0)]     # tests/test_gpu_frontend_edges.py


@functools.lru_cache(maxsize=None)
def pool_case(shape, C, ksp):
    """(x, xp): a finite map of bf16 values and the same map with the four NaN encodings, +Inf, -Inf and an all -Inf
    window planted in different channels (one-pixel and two-pixel maps hold them all in pixel 0).  Channel 0 .. 7 of
    every pixel of the last image's window at (0, 0) are -Inf: its maximum is -Inf."""
    NB, H, W = shape
    rng = hashrng()
    x = r16(rng.uniform(1702, f"pool{shape}{C}", (NB, H, W, C), -1, 1)).astype(np.float32)
    x[..., :C // 2] -= np.float32(1.5)                     # negative-only channels: padding must not win as 0
    x = r16(x).astype(np.float32)
    xp = x.copy()
    h, w_ = H // 2, W // 2
    for i, (name, _, _) in enumerate(PLANTS[:6]):
        xp[0, h, w_, 8 + 5 * i] = bf16_value(name)
    xp[NB - 1, :, :, 0:4] = -np.inf
    return x, xp


def stem_sites(NB, H, W):
    s = [(0, 0, 0, 0), (0, H - 1, W - 1, 2)]
    if NB > 1:
        s.append((1, 0, 0, 1))
    if W == 513:
        s += [(0, 0, 255, 0), (0, 1, 256, 1)]
    return s


STEM_SHAPES = [(2, 30, 41, 64), (1, 7, 7, 32), (1, 2, 513, 64)]
# The pooled map of a 7 x 7 image is 2 x 2 and every element of it sees pixel (0, 0): the fused stem + pool runs on a
# 15 x 15 image instead (pooled 4 x 4, 11 of 16 pixels unchanged), so that "half of the outputs unchanged" holds.
STEM_POOL_SHAPES = [(2, 30, 41, 64), (1, 15, 15, 32), (1, 2, 513, 64)]


@functools.lru_cache(maxsize=None)
def stem_case(NB, H, W, Cout):
    """(x, xp, w, b, ref conv clean, ref conv planted, ref pool clean, ref pool planted).  Planted pixels: (0, 0), the
    last pixel of image 0, the first of image 1 and, at W = 513, input columns 255 / 256 (conv columns 127 / 128: the
    128-column tile boundary and the pooled column carried across it); the values rotate through PLANTS, and weight
    [0, ch] of the first +Inf's channel is zero at every tap (Inf * 0)."""
    rng = hashrng()
    x = rng.uniform(1703, f"stem{(NB, H, W)}", (NB, H, W, 3), -2, 2)
    w = nonzero_normal(rng, 1703, f"stemw{Cout}", (Cout, 3, 7, 7), 0.1)
    b = rng.normal(1703, f"stemb{Cout}", (Cout,), std=0.1)
    xp = x.copy()
    order = [PLANTS[4], PLANTS[0], PLANTS[5], PLANTS[2], PLANTS[3], PLANTS[1]]       # +Inf first: its channel meets the zero weight
    sites = stem_sites(NB, H, W)
    for i, s in enumerate(sites):
        xp[s] = order[i % len(order)][1]
    w[0, sites[0][3]] = 0.0
    ref_c = conv2d_bf16_ref(x, w, b, 2, 3, None, True)
    ref_p = conv2d_bf16_ref(xp, w, b, 2, 3, None, True)
    return x, xp, w, b, ref_c, ref_p, max_pool_ref(ref_c, 3, 2, 1), max_pool_ref(ref_p, 3, 2, 1)


def spread_values(n):
    """n planted bf16 values: the NaN encodings, +Inf and -Inf in turn (names of BF16_BITS)."""
    names = ["+inf", "nan+", "-inf", "snan+", "nan-", "nan-pay"]
    return [names[i % len(names)] for i in range(n)]


TAIL_SHAPES = [(64, 3, 7, 61), (128, 2, 9, 13), (256, 3, 7, 11)]


def tail_sites(NB, H, W):
    """Pixels (nb, h, w) of h1 that hold a planted value: both ends of a row wrap in the middle of image 0, the last
    pixel of image 0 and the first of image 1, linear pixels 127 and 128 (the edge of the first 128-pixel tile)."""
    r = H // 2
    lin = lambda n: (n // (H * W), (n % (H * W)) // W, n % W)   # noqa: E731
    return [(0, r, W - 1), (0, r + 1, 0), (0, H - 1, W - 1), (1, 0, 0), lin(127), lin(128)]


@functools.lru_cache(maxsize=None)
def tail_case(CM, NB, H, W):
    """Operands of a fused tail (bf16 values as float32) and the references of its two-launch chain:
    (h1, h1p, res, resp, w2, b2, w3, b3, ref_clean, ref_planted).  Every planted pixel of h1 holds its value in channel
    1 + site index; w2[0, 1] = 0 at every tap, where the first site's +Inf sits (Inf * 0).  The residual holds one +Inf."""
    rng = hashrng()
    tag = f"tail{(CM, NB, H, W)}"
    h1 = r16(rng.uniform(1704, "h1" + tag, (NB, H, W, CM), 0, 1)).astype(np.float32)
    res = r16(rng.uniform(1704, "res" + tag, (NB, H, W, 4 * CM), -1, 1)).astype(np.float32)
    w2 = r16(nonzero_normal(rng, 1704, "w2" + tag, (CM, CM, 3, 3), float(np.sqrt(2.0 / (9 * CM))))).astype(np.float32)
    w3 = r16(nonzero_normal(rng, 1704, "w3" + tag, (4 * CM, CM, 1, 1), float(np.sqrt(2.0 / CM)))).astype(np.float32)
    assert (w2 != 0).all() and (w3 != 0).all()
    w2[0, 1] = 0.0
    b2 = rng.normal(1704, "b2" + tag, (CM,), std=0.1)
    b3 = rng.normal(1704, "b3" + tag, (4 * CM,), std=0.1)
    h1p, resp = h1.copy(), res.copy()
    sites = tail_sites(NB, H, W)
    for i, (s, name) in enumerate(zip(sites, spread_values(len(sites)))):
        h1p[s + (1 + i,)] = bf16_value(name)
    resp[NB - 1, 1, 2, 5] = np.inf                      # away from every planted pixel's 3 x 3 neighbourhood? checked by the host test
    refs = []
    for a, r in ((h1, res), (h1p, resp)):
        h2 = conv2d_bf16_ref(a, w2, b2, 1, 1, None, True)
        refs.append(conv2d_bf16_ref(h2, w3, b3, 1, 0, r, True))
    return h1, h1p, res, resp, w2, b2, w3, b3, refs[0], refs[1]


BLOCK_SHAPES = [(64, 1, 11, 31), (128, 1, 7, 31), (64, 2, 9, 13)]


def block_sites(CM, NB, H, W):
    """(0, 0), both sides of the tile grid's inner corner (tiles of 10 x 30 at CM = 64, 6 x 30 at 128; on a map inside
    one tile: the map's centre), (H - 1, W - 1) of the last image, the last pixel of image 0."""
    TR, TW = (10, 30) if CM == 64 else (6, 30)
    inner = [(0, TR - 1, TW - 1), (0, TR, TW)] if (H > TR and W > TW) else [(0, H // 2, W // 2)]
    return [(0, 0, 0)] + inner + [(NB - 1, H - 1, W - 1), (0, H - 1, W - 1)]


NEG_CH = 40      # input channel whose conv1 weights are all negative (the only weights that are not as drawn, beside the zero)


def _block_weights(rng, tag, CIN, CM, proj):
    w1 = r16(nonzero_normal(rng, 1705, "w1" + tag, (CM, CIN, 1, 1), float(np.sqrt(2.0 / CIN)))).astype(np.float32)
    w2 = r16(nonzero_normal(rng, 1705, "w2" + tag, (CM, CM, 3, 3), float(np.sqrt(2.0 / (9 * CM))))).astype(np.float32)
    w3 = r16(nonzero_normal(rng, 1705, "w3" + tag, (4 * CM, CM, 1, 1), float(np.sqrt(2.0 / CM)))).astype(np.float32)
    ws = r16(nonzero_normal(rng, 1705, "ws" + tag, (4 * CM, CIN, 1, 1), float(np.sqrt(1.0 / CIN)))).astype(np.float32) if proj else None
    b = {n: rng.normal(1705, n + tag, (c,), std=0.1) for n, c in (("b1", CM), ("b2", CM), ("b3", 4 * CM), ("bs", 4 * CM))}
    assert all((w != 0).all() for w in (w1, w2, w3))
    w1[0, 1] = 0.0                                      # meets the +Inf of the first site: Inf * 0
    w1[:, NEG_CH] = -np.abs(w1[:, NEG_CH])              # a +Inf in this channel is -Inf in all of conv1: h1 = relu(-Inf) = 0
    return w1, w2, w3, ws, b


def _block_ref(x, res, w1, w2, w3, ws, b, stride):
    h1 = conv2d_bf16_ref(x, w1, b["b1"], stride, 0, None, True)
    h2 = conv2d_bf16_ref(h1, w2, b["b2"], 1, 1, None, True)
    sc = res if ws is None else conv2d_bf16_ref(x, ws, b["bs"], stride, 0, None, False)
    return conv2d_bf16_ref(h2, w3, b["b3"], 1, 0, sc, True)


@functools.lru_cache(maxsize=None)
def block_case(kind, CM, NB, H, W):
    """kind 'id' (bottleneck_block_bf16: x [NB,H,W,4CM] is its own residual), 'proj' (CIN = 64, stride 1, projection
    shortcut inside), 'res' (CIN = 256, CM = 128, stride 2, a separate residual with one +Inf; planted values also sit at odd
    coordinates, which no tap reads, in `xodd`).  Returns a dict of operands and references."""
    rng = hashrng()
    tag = f"block{(kind, CM, NB, H, W)}"
    CIN, stride = {"id": (4 * CM, 1), "proj": (64, 1), "res": (256, 2)}[kind]
    x = r16(rng.uniform(1705, "x" + tag, (NB, H, W, CIN), -1, 1)).astype(np.float32)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = r16(rng.uniform(1705, "r" + tag, (NB, OH, OW, 4 * CM), -1, 1)).astype(np.float32) if kind == "res" else None
    w1, w2, w3, ws, b = _block_weights(rng, tag, CIN, CM, kind == "proj")
    sites = [(n, h * stride, w * stride) for n, h, w in block_sites(CM, NB, OH, OW)]
    sites = list(dict.fromkeys(sites))
    xp = x.copy()
    for i, (s, name) in enumerate(zip(sites, spread_values(len(sites)))):
        xp[s + (1 + i,)] = bf16_value(name)
    # an infinity that comes out as one: +Inf in NEG_CH leaves h1 finite (0), so the shortcut's +Inf (identity) or
    # +-Inf (projection) is not met by a NaN of the main path
    quiet = (0, (OH // 2) * stride, min(4, OW - 1) * stride)
    assert quiet not in sites
    xp[quiet + (NEG_CH,)] = np.inf
    out = dict(x=x, xp=xp, res=res, w1=w1, w2=w2, w3=w3, ws=ws, b=b, stride=stride)
    if kind == "res":
        out["resp"] = res.copy()
        out["resp"][0, OH - 2, 1, 7] = np.inf
        out["xodd"] = x.copy()
        out["xodd"][0, 1, 3, :] = bf16_value("nan+")
        out["xodd"][0, 2, 5, 9] = bf16_value("+inf")     # an even row, an odd column
    rp = out.get("resp", xp if kind == "id" else None)
    out["ref_c"] = _block_ref(x, x if kind == "id" else res, w1, w2, w3, ws, b, stride)
    out["ref_p"] = _block_ref(xp, rp, w1, w2, w3, ws, b, stride)
    return out
