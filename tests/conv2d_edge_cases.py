"""The case table, operands and float64 reference of tests/test_gpu_conv2d_edges.py, kept apart from it so that
tests/test_conv2d_edge_cases_host.py can check the references themselves without a card.

A case = (form, Cin, Cout, geometry, NB).  Forms: `generic` (pack_conv2d + conv2d_nhwc), `frag` (pack_conv2d_frag +
conv2d_nhwc), `cin4` (pack_conv2d_frag_cin4 + conv2d_nhwc_cin4), `bf16` (pack_conv2d_frag_bf16 + conv2d_nhwc_bf16).
The reference is always torch.nn.functional.conv2d in float64 on the CPU on the same operands (rounded to bf16 first
for the bf16 form)."""
import collections
import functools

import numpy as np
import torch

from sentinel_buffers import p

Geom = collections.namedtuple("Geom", "KH KW stride pad H W")
Case = collections.namedtuple("Case", "form cin cout g nb")

# ------------------------------------------------------------------------------------------------ geometries
G_KH_NE_KW = [Geom(1, 3, 1, 0, 6, 7), Geom(3, 1, 2, 1, 6, 7), Geom(2, 3, 1, 1, 5, 4)]   # KH != KW, an even extent, padding where the kernel is 1 wide
G_TAPS = [Geom(7, 7, 2, 3, 9, 10), Geom(8, 8, 1, 4, 9, 10)]                              # 49 and 64 taps: tap bit 63
G_STRIDE = [Geom(3, 3, 3, 2, 5, 5), Geom(1, 1, 3, 0, 7, 8), Geom(3, 3, 2, 0, 4, 6)]      # stride 3; unread rows and columns
G_PADDING = [Geom(3, 3, 1, 2, 2, 2), Geom(1, 1, 1, 1, 3, 3), Geom(5, 5, 1, 2, 2, 3)]     # windows wholly in the padding; kernel larger than the map
G_RNG = [Geom(3, 3, 1, 1, h, w) for h, w in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2))]    # the linear-range form's row wrap
G_FOUR_TAPS = [Geom(2, 2, 1, 0, 3, 3)]                                                   # 4 taps: one whole chunk of the stem form
GEOMS = G_KH_NE_KW + G_TAPS + G_STRIDE + G_PADDING + G_RNG + G_FOUR_TAPS
NB = 3
NB_MANY = 70        # 1x1 and 2x2 maps: 70 / 280 / 1120 output pixels, a 128-pixel tile spans 8 to 128 images, the last tile is partial
G_MANY = [Geom(3, 3, 1, 1, 1, 1), Geom(3, 3, 1, 1, 2, 2), Geom(3, 3, 1, 2, 2, 2)]

# geometries of every channel pair beyond the smallest: one linear-range (3x3 / 1 / 1) and one not; 1x1 for the bf16
# launcher's `mi = 1` rule (Cout % 64 == 0 and KH * KW == 1 and Cin <= 256)
WIDE_RNG = (Geom(3, 3, 1, 1, 2, 2), NB_MANY)
WIDE_TAPS = (Geom(3, 1, 2, 1, 6, 7), NB)
WIDE_1X1 = (Geom(1, 1, 3, 0, 7, 8), NB)

# channel pairs; [0] of every list runs every geometry.  bf16 has two "smallest" pairs: Cout = 32 takes the 32-row kernels
# <1, *>, Cout = 64 the 64-row kernels <2, *>, and both are to meet every geometry.
CHANNELS = {
    "generic": [(16, 4)] + [(ci, co) for ci in (16, 48) for co in (4, 36, 32, 160) if (ci, co) != (16, 4)],
    "frag": [(16, 32)] + [(ci, co) for ci in (16, 48) for co in (32, 160) if (ci, co) != (16, 32)],
    "cin4": [(1, 32)] + [(ci, co) for ci in (1, 3, 4) for co in (32, 96) if (ci, co) != (1, 32)],
    "bf16": [(64, 32), (64, 64)] + [(ci, co) for ci in (64, 128) for co in (32, 64, 96, 320) if (ci, co) not in ((64, 32), (64, 64))],
}
EVERY_GEOMETRY = {"generic": 1, "frag": 1, "cin4": 1, "bf16": 2}
FORMS = tuple(CHANNELS)


def is_rng(g):
    return (g.KH, g.KW, g.stride, g.pad) == (3, 3, 1, 1)


def out_hw(g):
    return (g.H + 2 * g.pad - g.KH) // g.stride + 1, (g.W + 2 * g.pad - g.KW) // g.stride + 1


def bf16_kernel(case):
    """The template arguments tspn_conv2d_nhwc_bf16 picks for a case (its rule restated)."""
    mi = 2 if case.cout % 64 == 0 and not (case.g.KH * case.g.KW == 1 and case.cin <= 256) else 1
    return mi, is_rng(case.g)


def all_cases():
    out = []
    for form in FORMS:
        for i, (ci, co) in enumerate(CHANNELS[form]):
            if i < EVERY_GEOMETRY[form]:
                out += [Case(form, ci, co, g, NB) for g in GEOMS] + [Case(form, ci, co, g, NB_MANY) for g in G_MANY]
            else:
                wide = [WIDE_RNG, WIDE_TAPS] + ([WIDE_1X1] if form == "bf16" and co % 64 == 0 else [])
                out += [Case(form, ci, co, g, nb) for g, nb in wide]
    return out


def case_id(c):
    g = c.g
    return f"{c.form}-{c.cin}to{c.cout}-k{g.KH}x{g.KW}s{g.stride}p{g.pad}-{g.H}x{g.W}-nb{c.nb}"


CASES = all_cases()

# ------------------------------------------------------------------------------------------------ operands
EXACT_TAPS = 48         # non-zero weights per output channel of the exact operands
EXACT_LIMIT = 256       # every |value| of an exact case stays below it: integers up to 256 are bf16 values


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _hashrng():
    import tspn_mi355x
    return tspn_mi355x.hashrng


@functools.lru_cache(maxsize=None)
def exact_operands(cin, cout, g, nb):
    """(x, w, bias, residual) as float32 arrays of small integers: x in [-2, 2]; every output channel has +-1 at 48 of
    its Cin KH KW weights (all of them when there are fewer) and 0 elsewhere; bias and residual in [-3, 3].  A partial
    sum is an integer of magnitude <= 96 and the result one of magnitude <= 102: exact in fp32 and in bf16, in any
    order of summation."""
    rng = _hashrng()
    tag = f"{cin}-{cout}-{tuple(g)}-{nb}"
    oh, ow = out_hw(g)
    x = rng.integers(1601, "x" + tag, (nb, g.H, g.W, cin), -2, 3).astype(np.float32)
    k = cin * g.KH * g.KW
    rank = np.argsort(np.argsort(rng.uniform(1601, "wpos" + tag, (cout, k)), axis=1), axis=1)
    sign = np.where(rng.uniform(1601, "wsgn" + tag, (cout, k)) < 0.5, -1.0, 1.0)
    w = (np.where(rank < EXACT_TAPS, sign, 0.0)).astype(np.float32).reshape(cout, cin, g.KH, g.KW)
    assert int((w != 0).sum(axis=(1, 2, 3)).max()) == min(EXACT_TAPS, k)
    b = rng.integers(1601, "b" + tag, (cout,), -3, 4).astype(np.float32)
    r = rng.integers(1601, "r" + tag, (nb, oh, ow, cout), -3, 4).astype(np.float32)
    return _ro(x, w, b, r)


@functools.lru_cache(maxsize=None)
def real_operands(cin, cout, g, nb):
    """(x, w, bias, residual) as the suite's conv tests draw them: x and residual uniform in [-1, 1), weights and bias
    normal with std 0.1."""
    rng = _hashrng()
    tag = f"{cin}-{cout}-{tuple(g)}-{nb}"
    oh, ow = out_hw(g)
    x = rng.uniform(1602, "x" + tag, (nb, g.H, g.W, cin), -1, 1)
    w = rng.normal(1602, "w" + tag, (cout, cin, g.KH, g.KW), std=0.1)
    b = rng.normal(1602, "b" + tag, (cout,), std=0.1)
    r = rng.uniform(1602, "r" + tag, (nb, oh, ow, cout), -1, 1)
    return _ro(x, w, b, r)


def t(a):
    return torch.from_numpy(np.array(a))        # a copy: the cached operands are read-only


def r16(a):
    """float32 array -> the same values rounded to bf16, as a float32 array."""
    return t(a).to(torch.bfloat16).float().numpy()


def operands(case, kind):
    """The operands of a case as its form sees them: rounded to bf16 for the bf16 form (bias stays fp32), no residual
    for the stem form."""
    x, w, b, r = (exact_operands if kind == "exact" else real_operands)(case.cin, case.cout, case.g, case.nb)
    if case.form == "bf16":
        x, w, r = r16(x), r16(w), r16(r)
    if case.form == "cin4":
        r = None
    return x, w, b, r


def reference(x, w, g, bias=None, residual=None, relu=False, dtype=torch.float64):
    """act(conv2d(x) + bias + residual) on channels-last arrays by torch.nn.functional.conv2d on the CPU."""
    y = torch.nn.functional.conv2d(t(x).to(dtype).permute(0, 3, 1, 2), t(w).to(dtype),
                                   None if bias is None else t(bias).to(dtype), stride=g.stride, padding=g.pad)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + t(residual).to(dtype)
    return (torch.relu(y) if relu else y).contiguous()


# ------------------------------------------------------------------------------------------------ the four forms
def pack(tspn, device, form, w):
    wd = t(w).to(device)
    return {"generic": tspn.ops.pack_conv2d, "frag": tspn.ops.pack_conv2d_frag, "cin4": tspn.ops.pack_conv2d_frag_cin4,
            "bf16": tspn.ops.pack_conv2d_frag_bf16}[form](wd)


def device_x(device, form, x):
    """x as the form's entry takes it: bf16 for the bf16 form, zero-padded to 4 channels for the stem form."""
    xt = t(x)
    if form == "bf16":
        xt = xt.to(torch.bfloat16)
    if form == "cin4":
        xt = torch.nn.functional.pad(xt, (0, 4 - xt.shape[-1])).contiguous()
    return xt.to(device)


def run(tspn, device, form, x, w, g, bias=None, residual=None, relu=False):
    """The form's wrapper on the given operands; returns the device tensor (fp32, bf16 for the bf16 form)."""
    packed = pack(tspn, device, form, w)
    xd = device_x(device, form, x)
    bd = None if bias is None else t(bias).to(device)
    if form == "cin4":
        assert residual is None
        return tspn.ops.conv2d_nhwc_cin4(xd, packed, (g.KH, g.KW), g.stride, g.pad, bias=bd, relu=relu)
    rd = None if residual is None else t(residual).to(device)
    if form == "bf16":
        rd = None if rd is None else rd.to(torch.bfloat16)
        return tspn.ops.conv2d_nhwc_bf16(xd, packed, (g.KH, g.KW), g.stride, g.pad, bias=bd, residual=rd, relu=relu)
    return tspn.ops.conv2d_nhwc(xd, packed, (g.KH, g.KW), g.stride, g.pad, bias=bd, residual=rd, relu=relu)


def run_raw(tspn, form, xd, nb, g, cin, packed, cout, bias, residual, relu, out):
    """The form's C entry on caller-held device tensors; returns the status code."""
    l, s = tspn._abi.lib(), tspn.ops._stream()
    if form == "cin4":
        return l.tspn_conv2d_nhwc_cin4_f32(p(xd), nb, g.H, g.W, p(packed), cout, g.KH, g.KW, g.stride, g.pad, p(bias),
                                           1 if relu else 0, p(out), s)
    fn = {"generic": l.tspn_conv2d_nhwc_f32, "frag": l.tspn_conv2d_nhwc_frag_f32, "bf16": l.tspn_conv2d_nhwc_bf16}[form]
    return fn(p(xd), nb, g.H, g.W, cin, p(packed), cout, g.KH, g.KW, g.stride, g.pad, p(bias), p(residual),
              1 if relu else 0, p(out), s)
