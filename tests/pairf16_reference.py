"""Host-side model of the split-fp16 pair stage (csrc/pairf16/tspn_heads_pair_f16x3.hip), plain numpy: the float64
reference, the error budget the MFMA path is held to, the split itself, an emulation of the kernel's arithmetic, and the
input generators of tests/test_gpu_pair_stage_f16x3_bound.py (host side: tests/test_pairf16_reference_host.py).

The stage computes  out[p, h, t] = b_h + sum_c w_hc a_pct,  a = relu(fl32(u + v))  per canonical pair p = (s, o).  The
kernel and the fp32 chain both form exactly this fp32 `a`, so every reference here starts from `activations()` and the
rounding of the add is charged to nobody.

The budget.  With u = 2^-24 (half an fp32 ulp, relative) and S = |b_h| + sum_c |w_hc| a_c:

    |got - ref64| <= K u S + 2^-35 (wmax_h sum_c a_c + sum_c |w_hc|),        K = 20 + C / 32.

K, term by term, each in units of u |w a| summed over c (hence u S):
  12  the split.  x is carried as xh + 2^-11 xl with xh = f16(x), xl = f16(2^11 (x - xh)); fp16 rounds to relative
      2^-11, so |x - xh| <= 2^-11 |x| and |x - xh - 2^-11 xl| <= 2^-22 |x| = 4 u |x|.  The product w a is replaced by
      wh ah + 2^-11 (wh al + wl ah): the dropped 2^-22 wl al is at most 2^-22 |w a| = 4 u |w a|, the rounding of wl
      costs 4 u |w a|, the rounding of al 4 u |w a| (second-order terms are below 2^-33 |w a|).
   3  the MFMA's own sum inside a k-step of 32 channels: "worst |MFMA - float64| = 3.0 u * sum|x||w| per step", measured
      by the probe recorded in profiles/r7/README.md on v_mfma_f32_32x32x16_f16.  ASSUMPTION: the 16x16x32 form this
      kernel uses sums alike; nothing here measures it separately.  (acc_lo's steps add 2^-11 of this: nothing.)
 C/32 the fp32 accumulator across the C / 32 k-steps: one rounding of a partial sum <= S per step.
   2  the epilogue: the fma acc_hi + 2^-11 acc_lo rounds once, the bias add once (the division by the power-of-two
      scale is exact).
  12 + 3 + 2 = 17, rounded up to 20.
The second term is an absolute floor, not a relative one: fp16's subnormal spacing is 2^-24, so below 2^-14 a lo piece
rounds to 2^-25 absolute, i.e. 2^-36 of the activation's unit per activation (times |w_hc|, summed: 2^-36 sum_c |w_hc|)
and 2^-36 of the head's scale per weight (the scale puts wmax_h in [0.5, 1): at most 2^-35 wmax_h, times a_c, summed).
Both are written with 2^-35.

The fp32 chain (the fallback of a tile, `set_force_exact(1)`) is held to its own worst case: C fma roundings and the
bias add, (C + 2) u S."""
import numpy as np

U = 2.0 ** -24
LO = 2.0 ** 11
CK = 32                       # channels per k-step (PF_CK)
Q_EXTREMES = (-90, -40, -1, 0, 7, 40, 90)      # per-head scales of the exact cases: the extremes that are not flagged
KINDS = ("unit", "tiny_a", "heads_2k", "hot_weight", "near_limit", "wide_a")


def pair_table(B, N):
    """[B*N*(N-1), 2] global tracklet ids of the canonical table: per video, s-major, o != s."""
    s, o = np.divmod(np.arange(N * N), N)
    loc = np.stack([s, o], 1)[s != o]
    return np.concatenate([loc + b * N for b in range(B)])


def activations(y, B, N):
    """y fp32 [B*N, 2C, T] -> a fp32 [P, C, T] = relu(fl32(u + v)) per canonical pair."""
    y = np.asarray(y, dtype=np.float32)
    C = y.shape[1] // 2
    p = pair_table(B, N)
    x = y[p[:, 0], :C] + y[p[:, 1], C:]                       # one fp32 add, as the kernel's
    return np.maximum(x, np.float32(0.0))


def ref64(a, w, b=None):
    """float64 [P, H, T]: b_h + sum_c w_hc a_c."""
    r = np.einsum("hc,pct->pht", np.asarray(w, np.float64), np.asarray(a, np.float64))
    return r if b is None else r + np.asarray(b, np.float64)[None, :, None]


def S(a, w, b=None):
    """float64 [P, H, T]: |b_h| + sum_c |w_hc| a_c."""
    return ref64(a, np.abs(np.asarray(w, np.float64)), None if b is None else np.abs(np.asarray(b, np.float64)))


def K_of(C):
    return 20 + C / 32


def bound(a, w, b=None):
    """The MFMA path's budget (module docstring), float64 [P, H, T]."""
    w64, a64 = np.abs(np.asarray(w, np.float64)), np.asarray(a, np.float64)
    floor = w64.max(1)[None, :, None] * a64.sum(1)[:, None, :] + w64.sum(1)[None, :, None]
    return K_of(w64.shape[1]) * U * S(a, w, b) + 2.0 ** -35 * floor


def chain_bound(a, w, b=None):
    """The fp32 chain's worst case: (C + 2) u S."""
    return (np.asarray(w).shape[1] + 2) * U * S(a, w, b)


def split(x):
    """fp32 -> (hi, lo) fp16: hi = f16(x), lo = f16((x - hi) * 2^11); the residual and its scaling are exact in fp32."""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(LO)).astype(np.float16)
    return hi, lo


def head_scale(w):
    """Per head, as pairf16_scale_kernel: max|w| = f 2^e with f in [0.5, 1) -> (inverse scale 2^e as fp32 [H], flagged)
    with flagged = some weight non-finite, or a head's max|w| below 2^-100, or e > 100.  A flagged head's scale is 1."""
    w = np.asarray(w, dtype=np.float32)
    mx = np.abs(w).max(1)
    finite = np.isfinite(w).all(1)
    with np.errstate(invalid="ignore"):
        _, e = np.frexp(np.where(finite, mx, np.float32(1.0)))
        bad = ~finite | ~(mx >= np.float32(2.0 ** -100)) | (e > 100)
    inv = np.where(bad, np.float32(1.0), np.ldexp(np.float32(1.0), np.where(bad, 0, e))).astype(np.float32)
    return inv, bool(bad.any())


def split_weights(w):
    """(wh, wl fp16 [H, C], inverse scales fp32 [H]) of unflagged weights, as pairf16_pack_kernel."""
    inv, flagged = head_scale(w)
    assert not flagged
    ws = np.asarray(w, np.float32) * (np.float32(1.0) / inv)[:, None]      # a power of two: exact
    return split(ws) + (inv,)


def emulate(a, w, b=None, drop_wl_ah=False, lo_inv=2.0 ** -11):
    """The kernel's arithmetic as far as it is specified: the two splits, float64 inside a 32-channel k-step (an MFMA is
    at least as good as 3 u per step, see the budget), ONE fp32 rounding of each accumulator per MFMA, the epilogue's
    fma, scale and bias add in fp32.  `drop_wl_ah` and `lo_inv` plant the two defects the budget must catch."""
    a = np.asarray(a, np.float32)
    wh, wl, inv = split_weights(w)
    ah, al = split(a)
    wh, wl, ah, al = (x.astype(np.float64) for x in (wh, wl, ah, al))
    P, C, T = a.shape
    H = wh.shape[0]
    acc_hi, acc_lo = np.zeros((P, H, T), np.float32), np.zeros((P, H, T), np.float32)
    for k in range(0, C, CK):
        c = slice(k, k + CK)
        acc_hi = (acc_hi + np.einsum("hc,pct->pht", wh[:, c], ah[:, c])).astype(np.float32)
        acc_lo = (acc_lo + np.einsum("hc,pct->pht", wh[:, c], al[:, c])).astype(np.float32)
        if not drop_wl_ah:
            acc_lo = (acc_lo + np.einsum("hc,pct->pht", wl[:, c], ah[:, c])).astype(np.float32)
    v = (acc_lo.astype(np.float64) * lo_inv + acc_hi).astype(np.float32) * inv[None, :, None]
    return v + (np.float32(0.0) if b is None else np.asarray(b, np.float32)[None, :, None])


# ------------------------------------------------------------------------------------------------ the six distributions
def make_case(rng, kind, B, N, C, T, H=12, seed=71):
    """(y fp32 [B*N, 2C, T], w fp32 [H, C], b fp32 [H]) of distribution `kind`; rng = the package's hashrng module."""
    assert kind in KINDS, kind
    y = rng.uniform(seed, "y", (B * N, 2 * C, T), -1, 1)
    w = rng.normal(seed, "wh", (H, C), std=0.1)
    b = rng.normal(seed, "bh", (H,), std=0.1)
    if kind == "tiny_a":                     # ah is mostly an fp16 subnormal
        y = y * np.float32(2.0 ** -18)
    elif kind == "heads_2k":                 # head h at 2^(8 (h - 6)): the per-head scale from 2^-48 to 2^40
        f = np.ldexp(np.float32(1.0), 8 * (np.arange(H) - 6)).astype(np.float32)
        w, b = w * f[:, None], b * f
    elif kind == "hot_weight":               # one weight at 1.0 above a floor of 2^-20: the others' wh are fp16 subnormals
        w = w * np.float32(2.0 ** -20)
        w[:, 7] = 1.0
        y[:, 7, 1::2] = -4.0                 # u + v < 0 on every other frame: the hot channel is off there
    elif kind == "near_limit":               # inside the MFMA range (|u|, |v| <= 2^14): the MFMA path must run
        y = rng.uniform(seed, "yl", y.shape, -16000, 16000)
    elif kind == "wide_a":                   # 34 binades of activations in one sum
        mag = np.exp2(rng.uniform(seed, "ye", y.shape, -20, 14).astype(np.float64)).astype(np.float32)
        assert float(mag.max()) < 16384.0
        y = np.where(rng.uniform(seed, "ys", y.shape) < 0.5, -mag, mag).astype(np.float32)
    return np.ascontiguousarray(y, np.float32), np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)


# ------------------------------------------------------------------------------------------------ the exact cases
def _units(x):
    """The largest power of two that divides every nonzero element of the float64 array x (1.0 if there is none)."""
    nz = x[x != 0]
    if nz.size == 0:
        return 1.0
    m, e = np.frexp(nz)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = mi & -mi
    return float(2.0 ** int((e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)).min()))


def exact_case(rng, which, C, N=9, T=32, H=12, seed=72):
    """Inputs on which the split-fp16 path must return float32(ref64) bit for bit (with no bias): wl al = 0 everywhere,
    the addends of acc_hi and of acc_lo are integer multiples of one unit each, and sum |addend| < 2^24 units per
    accumulator, so every summation order is exact and the epilogue's one fma rounds once.
      A  a in {0} u [32, 64) in multiples of 2^-16 (22 bits), weights k 2^-6 2^q_h with |k| <= 63;
      B  a in {0 .. 7}, weights +-k 2^-22 2^q_h with k in [2^21, 2^22) (22 bits);
      C  a in {0} u [2^-17, 2^-16) in multiples of 2^-35 (ah and al are fp16 subnormals), weights as in A.
    About 30 % of the (object, channel, frame) entries drive u + v negative.  Returns (y, w, stats); check_exact_case()
    asserts the preconditions in integers."""
    ku = rng.integers(seed, which + "u", (N, C, T), 0, 1 << 30)
    kv = rng.integers(seed, which + "v", (N, C, T), 0, 1 << 30)
    dead = rng.uniform(seed, which + "d", (N, C, T)) < 0.3
    if which == "B":
        unit, u, v, off = 1.0, 3 + ku % 3, kv % 5 - 2, -16                 # u + v in [1, 7]
    else:
        L = (1 << 21) if which == "A" else (1 << 18)                       # a in [L, 2L) units
        unit = 2.0 ** -16 if which == "A" else 2.0 ** -35
        u, v, off = L + L // 4 + ku % (L // 4), kv % (L // 2) - L // 4, -4 * L      # u + v in [L, 1.75 L)
    v = np.where(dead, off, v)
    y64 = np.concatenate([u, v], 1).astype(np.float64) * unit
    y = y64.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), y64) and int(np.abs(np.concatenate([u, v], 1)).max()) < (1 << 24)
    q = np.array([Q_EXTREMES[h % len(Q_EXTREMES)] for h in range(H)])
    sign = np.where(rng.uniform(seed, which + "s", (H, C)) < 0.5, -1.0, 1.0)
    if which == "B":
        k = (1 << 21) + rng.integers(seed, which + "k", (H, C), 0, 1 << 21)
        w64 = sign * k * 2.0 ** -22
    else:
        k = rng.integers(seed, which + "k", (H, C), 0, 64)
        k[np.arange(H), np.arange(H) % C] = 32 + k[np.arange(H), np.arange(H) % C] % 32     # one |k| >= 32 per head
        w64 = sign * k * 2.0 ** -6
    w64 = np.ldexp(w64, q[:, None])
    w = w64.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), w64)
    return y, w, q


def check_exact_case(y, w, q, B=1):
    """The preconditions of an exact case, in integers.  Returns (a, units in acc_hi, units in acc_lo): the largest
    sum |addend| of either accumulator in its unit."""
    N = y.shape[0] // B
    a = activations(y, B, N)
    # u + v was exact: the fp32 sum equals the float64 sum
    p, C = pair_table(B, N), y.shape[1] // 2
    x64 = y.astype(np.float64)[p[:, 0], :C] + y.astype(np.float64)[p[:, 1], C:]
    assert np.array_equal(a.astype(np.float64), np.maximum(x64, 0.0)), "u + v is not exact in fp32"
    frac = float((x64 < 0).mean())
    assert 0.2 < frac < 0.4, frac
    wh, wl, inv = split_weights(w)
    assert np.array_equal(inv, np.ldexp(np.float32(1.0), q).astype(np.float32)), "the head scale is not 2^q_h"
    ah, al = split(a)
    wh, wl, ah, al = (x.astype(np.float64) for x in (wh, wl, ah, al))
    ws = w.astype(np.float64) / inv.astype(np.float64)[:, None]
    assert np.array_equal(wh + wl / LO, ws), "wh + 2^-11 wl does not carry the weight"
    assert np.array_equal(ah + al / LO, a.astype(np.float64)), "ah + 2^-11 al does not carry the activation"
    assert not wl.any() or not al.any(), "wl al is not zero"
    totals = []
    for terms in ([(wh, ah)], [(wh, al), (wl, ah)]):                 # the addends of acc_hi, of acc_lo
        terms = [(x, z) for x, z in terms if x.any() and z.any()]
        unit = min([_units(x) * _units(z) for x, z in terms], default=1.0)       # the accumulator's unit
        tot = np.zeros((a.shape[0], w.shape[0], a.shape[2]), np.int64)
        for x, z in terms:
            xi, zi = np.abs(x) / _units(x), np.abs(z) / _units(z)
            assert np.array_equal(xi, np.round(xi)) and np.array_equal(zi, np.round(zi))
            per = int(round(_units(x) * _units(z) / unit))                       # this product's unit in the accumulator's
            tot += np.einsum("hc,pct->pht", xi.astype(np.int64), zi.astype(np.int64)) * per
        assert int(tot.max()) < (1 << 24), f"{int(tot.max())} units in one accumulator"
        totals.append(int(tot.max()))
    r = ref64(a, w)
    assert bool(((r == 0) | (np.abs(r) >= 2.0 ** -126)).all()), "an output is an fp32 subnormal"
    return a, totals[0], totals[1]
