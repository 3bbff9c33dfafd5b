"""Host-side model of the bf16 scoring path (csrc/tspn_bf16.hip, csrc/tspn_heads_pair_bf16.h,
csrc/pairlist/tspn_pairlist_bf16.hip), plain numpy: bf16 rounding by integer arithmetic, float64 references with the
header's rounding points, the error budget the kernels are held to, fp32 emulations of three summation orders, the eight
input kinds and the exact-case generators of tests/test_gpu_bf16_bound.py (host side: tests/test_bf16_reference_host.py).

The arithmetic (include/tspn_mi355x.h): operands are bf16, a product of two bf16 values has 16 significant bits and is exact
in fp32, accumulation is fp32, outputs are fp32.  There is ONE round-to-nearest-even to bf16 at each of
    pair stage   a = bf16(relu(fl32(U[s] + V[o])))       the fp32 add is one correctly rounded operation, formed here in
                                                         numpy float32 exactly as the kernel forms it: charged to nobody
    dense heads  a = bf16(relu(y))
    mean         out = bf16(fl32(sum_t x_t / T))
so every reference below starts from the SAME bf16 operands as the kernel and differs from it by fp32 summation alone.

The budget.  u = 2^-24 (half an fp32 ulp, relative).  The ONLY assumption: every addition the hardware performs on an fp32
partial sum errs by at most one fp32 ulp of that partial sum, i.e. 2 u |partial| -- twice what a correctly rounded adder
needs, which also covers an adder that truncates.  Nothing is assumed about the order in which an MFMA adds the k products
of one step.  Every partial sum of a contraction is bounded by S = |b| + sum |w| |a| (the same sum with absolute values),
so each addition costs at most 2 u S (second-order terms: (1 + 2u)^n - 1 - 2 n u < 1e-9 n^2, nothing at n <= 300).  For a
contraction of depth Kd in MFMA steps of k:
    k       additions inside one step, whatever their order (a tree or a chain of k products has k - 1 of them, one more
            for folding the step's sum into the accumulator if the hardware does that separately);  charged ONCE, not once
            per step, because the addends of step j are bounded by S_j = sum over that step's channels and sum_j S_j = S
    Kd / k  one accumulator update per step, each on a partial sum <= S
    2       the bias add of the epilogue, and one spare
    |got - ref64|  <=  2 (k + Kd / k + 2) u S.
Which instruction, which k (read from the sources):
    conv3_bf16_big_kernel        v_mfma_f32_32x32x16_bf16, k = 16; one MFMA per tap and 16-channel chunk: Kd = 3 Cin, Kd / k =
                                 3 Cin / 16 accumulator updates (the ring of tspn_bf16.hip; 192 at Cin = 1024)
    heads_pairgrid_bf16_kernel   v_mfma_f32_16x16x32_bf16, k = 32 (HP_KC), Kd = C, one accumulator per (s, o) slot pair
    heads_pairlist_bf16_kernel   the same tile (tspn_heads_pair_bf16.h): the same bits
    heads_dense_bf16_kernel      v_mfma_f32_16x16x32_bf16, k = 32, Kd = C, one accumulator per wave
At C = 32 this is 70 u S (the absolute 3e-5 of tests/test_gpu_bf16.py is about 300 u S there), at C = 2048 196 u S = 1.2e-5 S;
a dropped or doubled channel is about S / 2048 = 5e-4 S.  Nothing in the budget is measured.

The floor.  SUBNORMAL_FLOOR is the absolute error per activation that the contract allows below the normal range; it is 0:
the kernels keep bf16 subnormals (v_cvt_pk_bf16_f32 and both MFMAs), which the `subnormal` kind checks on every entry.

The mean.  temporal_mean_bf16_kernel forms four strided fp32 partial sums (frames t = j mod 4: ceil(T / 4) - 1 additions each,
the first on zero is exact), adds them pairwise (two levels), divides by (float)T (one rounding; T is exact) and rounds to
bf16.  Before the last rounding the value is within e = 2 (ceil(T / 4) + 3) u sum_t |x_t| / T of the float64 mean m (the
partials' additions, two levels of the tree, the division, one spare; each at most 2 u of a partial sum <= sum |x|).  Rounding
is monotone, so the output lies in the closed interval [bf16(fl32(m - e)), bf16(fl32(m + e))]: an interval, not a tolerance.

The kinds (make_pair_case / make_conv_case / make_mean_case), all deterministic through hashrng:
    unit         the distribution of tests/test_gpu_bf16.py: activations N(0, 1) (conv: U(-1, 1)), weights N(0, 0.1^2)
    large        activations 2^13 times that, weights 2^-13 times
    tiny         activations 2^-100 times, weights 2^90 times (outputs around 2^-10)
    hot_channel  one channel per k-step 2^12 times the others
    cancelling   activations 1 + 2^-4 U(-1, 1) against weights of alternating sign in pairs of equal magnitude: |ref| << S
    wide         per-channel powers of two, 2^-20 .. 2^20, on the activations and (independently) on the weights
    relu_edge    v = -u (1 + 2^-10 U(-1, 1)): half the activations vanish, the others are ten or more binades below |u| (a
                 pair-stage kind; the dense form reads the same fl32(u + v))
    subnormal    activations N(0, 1) 2^-129: fp32 subnormals, hence bf16 subnormals of one to four bits; weights 2^100 times

The exact cases (exact_pair_case / exact_conv_case / exact_mean_case).  Operands are small integers times ONE power of two per
tensor, a = m_a 2^qa, w = m_w 2^qw, the bias an integer in the unit 2^(qa + qw); the generator asserts
sum_c |m_w| m_a + |bias| < 2^24 in that unit.  Then every partial sum of every summation order is an integer below 2^24
units, hence exact in fp32, and the output must equal float32(ref64) bit for bit.  (qa, qw) runs over Q_PAIRS: the extremes
bf16 carries with the output finite and normal.  Three kinds per rounding point:
    plain   |m| <= 15 everywhere: no rounding happens anywhere
    ties    u + v (dense: y) is an odd 9-bit integer 257 .. 511 times 2^qa: exact in fp32, exactly halfway between two bf16
            values; n mod 4 = 1 rounds down and n mod 4 = 3 up, and both are present: ties-to-even alone decides the result
    zeros   u = -v (a = +0), u + v = -1 unit (the ReLU's 0), -0.0 inputs, and a head of all-zero weights whose output is
            exactly its bias; the other channels are plain
The conv has no rounding point: plain and zeros only.  The mean: T in {1, 2, 4, 8} on 8-bit integers times 2^q (the sum is
exact, the division by a power of two is exact, and the sum of T such integers is a tie for half / a quarter / an eighth of
the draws), and T = 3 with the exact integer sum s, whose reference is bf16(fl32(s / 3)): the double rounding the kernel
performs.

What the two planted defects of the host test cannot show, and why.  Truncation at the rounding point is a one-sided error
of up to 2^-8 |a| per activation, 2^-9 S on average -- some fifty times the budget at C = 2048, a thousand at C = 32 -- and
leaves the budget on every kind (on `cancelling` the one-sided errors meet weights of alternating sign and partly cancel: 18
budgets at C = 2048).  A dropped channel is |w a_c|: about S / C on every kind whose channels are alike.  On `hot_channel`
a COLD channel is 2^-12 / 64 of S at C = 2048, below the budget by construction, and on `wide` a channel's share is
whatever powers of two were drawn: the budget is relative to S, and what is invisible relative to S is invisible.  The host
test therefore drops the last k-step's hot channel on `hot_channel` and its largest share on `wide`, and asserts nothing
for the conv's `wide`, whose last channel is taken as it comes; on `relu_edge` half the elements have a_c = 0 and the other
half show it."""
import numpy as np

U = 2.0 ** -24
SUBNORMAL_FLOOR = 0.0          # absolute error allowed per activation below the normal range (module docstring)
K_PAIR, K_CONV = 32, 16        # the MFMA's k: v_mfma_f32_16x16x32_bf16 (pair stages, dense heads), v_mfma_f32_32x32x16_bf16 (conv)
KINDS = ("unit", "large", "tiny", "hot_channel", "cancelling", "wide", "relu_edge", "subnormal")
CONV_KINDS = ("unit", "large", "tiny", "hot_channel", "cancelling", "wide", "subnormal")
MEAN_KINDS = ("unit", "large", "tiny", "wide", "cancelling")
EXACT_KINDS = ("plain", "ties", "zeros")
# (qa, qw): output unit 2^(qa + qw), outputs below 2^24 units: finite and normal for |qa + qw| <= 100
Q_PAIRS = ((0, 0), (-1, 7), (7, -1), (-100, 100), (100, -100), (100, 0), (0, 100), (-100, 0), (0, -100))
Q_MEAN = (-100, -1, 0, 7, 100)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def rne_bf16(x):
    """fp32 -> the nearest bf16 value, ties to even, as fp32.  Integer arithmetic on the bit pattern: adding 0x7FFF plus the
    lowest kept bit carries into the kept half exactly when the dropped half is above a half, or is a half and the kept
    half is odd; the carry runs through the exponent, so the largest finite values go to Inf and subnormals round like
    everything else.  NaN stays NaN (quiet, payload's upper bits kept)."""
    b = bits(x).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, (b.astype(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r)
    return r.view(np.float32).reshape(np.shape(x))


def trunc_bf16(x):
    """The planted defect: the low half dropped (round toward zero)."""
    return (bits(x) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(x))


def relu32(x):
    """max(x, +0) in fp32; -0 -> +0."""
    x = np.asarray(x, np.float32)
    return np.where(x > 0, x, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ operands
def pair_table(B, N):
    """[B*N*(N-1), 2] global tracklet ids of the canonical table: per video, s-major, o != s."""
    s, o = np.divmod(np.arange(N * N), N)
    loc = np.stack([s, o], 1)[s != o]
    return np.concatenate([loc + b * N for b in range(B)])


def pair_activations(y, table, rnd=rne_bf16):
    """y fp32 [B*N, T, 2C], table [P, 2] global ids -> a fp32 [P, T, C] holding bf16 values: rnd(relu(fl32(u + v)))."""
    y = np.asarray(y, np.float32)
    C = y.shape[2] // 2
    table = np.asarray(table)
    return rnd(relu32(y[table[:, 0], :, :C] + y[table[:, 1], :, C:]))          # ONE fp32 add, as the kernel's


def dense_activations(y, rnd=rne_bf16):
    """y fp32 [P, T, C] -> rnd(relu(y))."""
    return rnd(relu32(y))


# ------------------------------------------------------------------------------------------------ references and budgets
def heads_ref64(a, w, b=None):
    """float64 [P, H, T]: b_h + sum_c w_hc a_ptc for a [P, T, C], w [H, C] (bf16 values)."""
    r = np.einsum("hc,ptc->pht", np.asarray(w, np.float64), np.asarray(a, np.float64))
    return r if b is None else r + np.asarray(b, np.float64)[None, :, None]


def heads_S(a, w, b=None):
    return heads_ref64(np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(w, np.float64)),
                       None if b is None else np.abs(np.asarray(b, np.float64)))


def conv_ref64(x, w, b=None):
    """float64 [B, T, M]: b_m + sum_{c,k} w[m, c, k] x[t + k - 1, c], zero outside [0, T); x [B, T, Cin], w [M, Cin, 3]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T = x.shape[1]
    xp = np.pad(x, ((0, 0), (1, 1), (0, 0)))
    r = sum(np.einsum("btc,mc->btm", xp[:, k:k + T], w[:, :, k]) for k in range(3))
    return r if b is None else r + np.asarray(b, np.float64)[None, None, :]


def conv_S(x, w, b=None):
    return conv_ref64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                      None if b is None else np.abs(np.asarray(b, np.float64)))


def K_of(Kd, k):
    """The budget in units of u S: 2 (k + Kd / k + 2)."""
    return 2.0 * (k + Kd / k + 2)


def heads_budget(a, w, b=None):
    """float64 [P, H, T]: 2 (32 + C / 32 + 2) u S (+ the subnormal floor, 0 unless SUBNORMAL_FLOOR is set)."""
    w64 = np.abs(np.asarray(w, np.float64))
    return K_of(w64.shape[1], K_PAIR) * U * heads_S(a, w, b) + SUBNORMAL_FLOOR * w64.sum(1)[None, :, None]


def conv_budget(x, w, b=None):
    """float64 [B, T, M]: 2 (16 + 3 Cin / 16 + 2) u S."""
    w64 = np.abs(np.asarray(w, np.float64))
    return K_of(3 * w64.shape[1], K_CONV) * U * conv_S(x, w, b) + SUBNORMAL_FLOOR * w64.sum((1, 2))[None, None, :]


def mean_interval(x):
    """x [R, T, D] bf16 values -> (lo, hi) fp32 [R, D]: the closed interval of the module docstring."""
    x64 = np.asarray(x, np.float64)
    T = x64.shape[1]
    m = x64.sum(1) / T
    e = 2.0 * (-(-T // 4) + 3) * U * np.abs(x64).sum(1) / T
    return rne_bf16((m - e).astype(np.float32)), rne_bf16((m + e).astype(np.float32))


# ------------------------------------------------------------------------------------------------ fp32 emulations
def contract_emulate(a, w, b=None, order="blocks", k=K_PAIR, drop=None):
    """fp32 emulation of out[r, h] = b_h + sum_j w[h, j] a[r, j] for a [R, Kd], w [H, Kd] (bf16 values: the products are
    formed in float64 and are exact).  order: "sequential" one product at a time into one fp32 accumulator; "pairwise" a
    balanced tree of fp32 additions; "blocks" float64 inside a block of k, one fp32 rounding per block into the
    accumulator (an MFMA whose inner sum is exact).  The bias is added last, in fp32.  `drop`: index of a channel left
    out (the planted defect)."""
    a64, w64 = np.asarray(a, np.float64), np.asarray(w, np.float64)
    if drop is not None:
        keep = np.arange(a64.shape[1]) != drop
        a64, w64 = a64[:, keep], w64[:, keep]
    R, Kd = a64.shape
    H = w64.shape[0]
    if order == "sequential":
        acc = np.zeros((R, H), np.float32)
        for j in range(Kd):
            acc = (acc + a64[:, j, None] * w64[None, :, j]).astype(np.float32)
    elif order == "blocks":
        acc = np.zeros((R, H), np.float32)
        for j in range(0, Kd, k):
            acc = (acc + a64[:, j:j + k] @ w64[:, j:j + k].T).astype(np.float32)
    elif order == "pairwise":
        p = (a64[:, None, :] * w64[None, :, :]).astype(np.float32)              # exact
        assert np.array_equal(p.astype(np.float64), a64[:, None, :] * w64[None, :, :])
        while p.shape[2] > 1:
            if p.shape[2] % 2:
                p = np.concatenate([p, np.zeros(p.shape[:2] + (1,), np.float32)], 2)
            p = p[:, :, 0::2] + p[:, :, 1::2]                                    # fp32 adds
        acc = p[:, :, 0]
    else:
        raise ValueError(order)
    return acc if b is None else acc + np.asarray(b, np.float32)[None, :]


def heads_emulate(a, w, b=None, **kw):
    """contract_emulate on a [P, T, C] -> [P, H, T]."""
    P, T, C = a.shape
    return contract_emulate(np.reshape(a, (P * T, C)), w, b, **kw).reshape(P, T, -1).transpose(0, 2, 1)


def conv_emulate(x, w, b=None, **kw):
    """contract_emulate on the im2col of x [B, T, Cin] in the kernel's order (16-channel chunk, tap, channel) -> [B, T, M]."""
    x = np.asarray(x, np.float32)
    B, T, Cin = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (0, 0)))
    cols = np.stack([xp[:, k:k + T] for k in range(3)], 2)                       # [B, T, 3, Cin]
    cols = cols.reshape(B, T, 3, Cin // K_CONV, K_CONV).transpose(0, 1, 3, 2, 4).reshape(B * T, 3 * Cin)
    wm = np.asarray(w, np.float32).transpose(0, 2, 1)                            # [M, 3, Cin]
    wm = wm.reshape(-1, 3, Cin // K_CONV, K_CONV).transpose(0, 2, 1, 3).reshape(-1, 3 * Cin)
    return contract_emulate(cols, wm, b, k=K_CONV, **kw).reshape(B, T, -1)


def mean_emulate(x):
    """The kernel's order in fp32: partial j sums frames j, j + 4, ..; (p0 + p1) + (p2 + p3); / (float)T; one rounding to bf16."""
    x = np.asarray(x, np.float32)
    T = x.shape[1]
    part = []
    for j in range(4):
        acc = np.zeros((x.shape[0], x.shape[2]), np.float32)
        for t in range(j, T, 4):
            acc = acc + x[:, t]
        part.append(acc)
    return rne_bf16(((part[0] + part[1]) + (part[2] + part[3])) / np.float32(T))


# ------------------------------------------------------------------------------------------------ the kinds
def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e, np.int32)).astype(np.float32)


def hot_index(n, k):
    """One channel in every block of k: block j's hot channel."""
    j = np.arange(n // k)
    return j * k + (7 * j + 5) % k


def make_pair_case(rng, kind, B, N, C, T, H=12, seed=171):
    """(y fp32 [B*N, T, 2C], w fp32 [H, C] holding bf16 values, b fp32 [H]) of `kind`; rng = the package's hashrng."""
    assert kind in KINDS, kind
    y = rng.normal(seed, "y", (B * N, T, 2 * C), std=1.0)
    w = rng.normal(seed, "hw", (H, C), std=0.1)
    b = rng.normal(seed, "hb", (H,), std=0.1)
    if kind == "large":
        y, w = y * np.float32(2.0 ** 13), w * np.float32(2.0 ** -13)
    elif kind == "tiny":
        y, w, b = y * np.float32(2.0 ** -100), w * np.float32(2.0 ** 90), b * np.float32(2.0 ** -10)
    elif kind == "hot_channel":
        hot = hot_index(C, K_PAIR)
        y[:, :, hot] *= np.float32(4096.0)
        y[:, :, C + hot] *= np.float32(4096.0)
    elif kind == "cancelling":
        y = (1.0 + rng.uniform(seed, "yc", y.shape, -1, 1) * np.float32(2.0 ** -4)).astype(np.float32)
        mag = np.abs(rng.normal(seed, "wc", (H, C // 2), std=0.1)) + np.float32(0.05)
        w = np.stack([mag, -mag], 2).reshape(H, C)
        b = b * np.float32(2.0 ** -6)
    elif kind == "wide":
        ea = rng.integers(seed, "ea", (C,), -20, 21)
        ew = rng.integers(seed, "ew", (C,), -20, 21)
        y = y * np.concatenate([_pow2(ea), _pow2(ea)])
        w = w * _pow2(ew)
    elif kind == "relu_edge":
        u = y[:, :, :C]
        # every object's V half is (minus) ONE shared row, so that every pair (s, o) sits on the edge: u_s + v_o = -u_s d_o
        base = y[:1, :, :C]
        d = rng.uniform(seed, "yd", (B * N, T, C), -1, 1) * np.float32(2.0 ** -10)
        y = np.concatenate([np.broadcast_to(base, u.shape) * (1 + rng.uniform(seed, "ys", u.shape, -1, 1) * np.float32(2.0 ** -10)),
                            -base * (1 + d)], 2).astype(np.float32)
    elif kind == "subnormal":
        y, w, b = y * np.float32(2.0 ** -129), w * np.float32(2.0 ** 100), b * np.float32(2.0 ** -30)
        assert float(np.abs(y).max()) < 2.0 ** -127 and bool((y != 0).any())
    w = rne_bf16(np.ascontiguousarray(w, np.float32))
    return np.ascontiguousarray(y, np.float32), w, np.ascontiguousarray(b, np.float32)


def make_dense_case(rng, kind, P, C, T, H=12, seed=172):
    """(y fp32 [P, T, C], w, b): the fl32(u + v) of a pair case's first P (s, s) sums -- the same values the pair stage's
    rounding point sees, `relu_edge` included."""
    y2, w, b = make_pair_case(rng, kind, 1, P, C, T, H, seed)
    return np.ascontiguousarray(y2[:, :, :C] + y2[:, :, C:], np.float32), w, b


def make_conv_case(rng, kind, B, T, Cin, M, seed=173):
    """(x fp32 [B, T, Cin] and w fp32 [M, Cin, 3] holding bf16 values, b fp32 [M]) of `kind`."""
    assert kind in CONV_KINDS, kind
    x = rng.uniform(seed, "x", (B, T, Cin), -1, 1)
    w = rng.normal(seed, "w", (M, Cin, 3), std=0.1)
    b = rng.normal(seed, "b", (M,), std=0.1)
    if kind == "large":
        x, w = x * np.float32(2.0 ** 13), w * np.float32(2.0 ** -13)
    elif kind == "tiny":
        x, w, b = x * np.float32(2.0 ** -100), w * np.float32(2.0 ** 90), b * np.float32(2.0 ** -10)
    elif kind == "hot_channel":
        x[:, :, hot_index(Cin, K_CONV)] *= np.float32(4096.0)
    elif kind == "cancelling":
        x = (1.0 + rng.uniform(seed, "xc", x.shape, -1, 1) * np.float32(2.0 ** -4)).astype(np.float32)
        mag = np.abs(rng.normal(seed, "wc", (M, Cin // 2, 3), std=0.1)) + np.float32(0.05)
        w = np.stack([mag, -mag], 2).reshape(M, Cin, 3)
        b = b * np.float32(2.0 ** -6)
    elif kind == "wide":
        x = x * _pow2(rng.integers(seed, "ea", (Cin,), -20, 21))
        w = w * _pow2(rng.integers(seed, "ew", (Cin,), -20, 21))[None, :, None]
    elif kind == "subnormal":
        x, w, b = x * np.float32(2.0 ** -128), w * np.float32(2.0 ** 100), b * np.float32(2.0 ** -30)
    x, w = rne_bf16(np.ascontiguousarray(x, np.float32)), rne_bf16(np.ascontiguousarray(w, np.float32))
    if kind == "subnormal":
        assert float(np.abs(x).max()) < 2.0 ** -126 and bool((x != 0).any())
    return x, w, np.ascontiguousarray(b, np.float32)


def make_mean_case(rng, kind, R, T, D, seed=174):
    """x fp32 [R, T, D] holding bf16 values."""
    assert kind in MEAN_KINDS, kind
    x = rng.uniform(seed, "x", (R, T, D))
    if kind == "large":
        x = x * np.float32(2.0 ** 13)
    elif kind == "tiny":
        x = x * np.float32(2.0 ** -100)
    elif kind == "wide":
        x = x * _pow2(rng.integers(seed, "e", (R, T, D), -20, 21))
    elif kind == "cancelling":          # signed, nearly equal magnitudes, alternating over the frames: |mean| << mean |x|
        x = (1.0 + x * np.float32(2.0 ** -4)) * np.where(np.arange(T) % 2, -1.0, 1.0)[None, :, None]
    return rne_bf16(np.ascontiguousarray(x, np.float32))


# ------------------------------------------------------------------------------------------------ the exact cases
def _exact_weights(rng, seed, tag, shape, mmax, qw, zero_row=True):
    m = rng.integers(seed, tag, shape, -mmax, mmax + 1)
    if zero_row:
        m[shape[0] // 2] = 0                                 # a head of all-zero weights: its output is exactly its bias
    w = np.ldexp(m.astype(np.float64), qw).astype(np.float32)
    assert np.array_equal(rne_bf16(w), w)
    return m, w


def _exact_bias(rng, seed, n, q):
    mb = rng.integers(seed, "mb", (n,), -1000, 1001)
    mb[mb == 0] = 3
    return mb, np.ldexp(mb.astype(np.float64), q).astype(np.float32)


def _exact_uv(rng, which, shape, seed):
    """Integers (u, v) of `shape`, in units of 2^qa, for the rounding point's three kinds."""
    ku = rng.integers(seed, which + "u", shape, 0, 1 << 20)
    kv = rng.integers(seed, which + "v", shape, 0, 1 << 20)
    if which == "plain":
        return ku % 16 - 7, kv % 16 - 8                                          # u + v in [-15, 15]
    if which == "ties":
        n = 289 + 2 * (ku % 96)                                                  # odd, 289 .. 479
        n = np.where((ku >> 8) % 5 == 0, -n, n)                                  # a fifth negative: the ReLU's 0
        return n, 2 * (kv % 33) - 32                                             # even, -32 .. 32: |u_s + v_o| odd in 257 .. 511
    assert which == "zeros"
    u, v = ku % 16 - 7, kv % 16 - 8
    sel = (ku >> 8) % 8
    v = np.where(sel == 0, -u, v)                                                # u = -v: +0
    v = np.where(sel == 1, -u - 1, v)                                            # one unit below zero
    u = np.where(sel == 2, 0, u).astype(np.float64)
    v = np.where(sel == 2, 0, v).astype(np.float64)
    u[sel == 2] = -0.0                                                           # -0.0 + -0.0 = -0.0 -> relu -> +0
    v[sel == 2] = -0.0
    u[(sel == 3) & (v == 0)] = -0.0
    return u, v


def _to_f32(m, q):
    x64 = np.ldexp(np.asarray(m, np.float64), q)
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    return x


def _assert_units(ma, mw, mb, einsum):
    tot = np.einsum(einsum, np.abs(mw).astype(np.int64), np.abs(ma).astype(np.int64))
    top = int(tot.max()) + int(np.abs(mb).max())
    assert top < (1 << 24), f"{top} units in one output"
    return top


def exact_pair_case(rng, which, B, N, C, T, qa, qw, H=12, seed=175):
    """(y [B*N, T, 2C], w [H, C], b [H], units): the output of the pair stage on ANY pair (s, o), s = o included, must
    equal float32(heads_ref64) bit for bit (module docstring).  units = the largest sum of |addend| of any output."""
    assert which in EXACT_KINDS
    u, v = _exact_uv(rng, which, (B * N, T, C), seed)
    y = np.concatenate([_to_f32(u, qa), _to_f32(v, qa)], 2)
    mw, w = _exact_weights(rng, seed, "mw", (H, C), 7 if which == "ties" else 15, qw)
    mb, b = _exact_bias(rng, seed, H, qa + qw)
    full = np.stack(np.divmod(np.arange(B * N * N), N), 1)                        # every (s, o) of every video, (s, s) too
    full = np.stack([full[:, 0] // N * N + full[:, 0] % N, full[:, 0] // N * N + full[:, 1]], 1)
    a = pair_activations(y, full)
    ma = np.ldexp(a.astype(np.float64), -qa)
    assert np.array_equal(ma, np.round(ma)) and float(ma.max()) <= (512 if which == "ties" else 15)
    x64 = y.astype(np.float64)[full[:, 0], :, :C] + y.astype(np.float64)[full[:, 1], :, C:]
    s32 = y[full[:, 0], :, :C] + y[full[:, 1], :, C:]
    assert np.array_equal(s32.astype(np.float64), x64), "u + v is not exact in fp32"
    if which == "ties":
        n = np.ldexp(x64, -qa)
        pos = n > 0
        assert bool((np.abs(n) % 2 == 1).all()) and float(np.abs(n).min()) >= 257 and float(np.abs(n).max()) <= 511
        assert bool((n[pos] % 4 == 1).any()) and bool((n[pos] % 4 == 3).any()) and bool((~pos).any())
        assert bool((ma[pos] != n[pos]).all()) and bool((ma[pos] % 4 == 0).all()), "a tie did not go to the even neighbour"
        assert bool((np.abs(trunc_bf16(s32)[pos] - a[pos]) > 0).any())
    if which == "zeros":
        assert bool((x64 == 0).any()) and bool((np.ldexp(x64, -qa) == -1).any()) and bool(np.signbit(y[y == 0]).any())
    units = _assert_units(ma, mw, mb, "hc,ptc->pht")
    return y, w, b, units


def exact_dense_case(rng, which, P, C, T, qa, qw, H=12, seed=176):
    """(y [P, T, C], w, b, units) for the dense heads: y is what u + v is in exact_pair_case."""
    u, v = _exact_uv(rng, which, (P, T, C), seed)
    y = (_to_f32(u, qa) + _to_f32(v, qa)).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), np.ldexp(np.asarray(u, np.float64) + np.asarray(v, np.float64), qa))
    mw, w = _exact_weights(rng, seed, "mw", (H, C), 7 if which == "ties" else 15, qw)
    mb, b = _exact_bias(rng, seed, H, qa + qw)
    ma = np.ldexp(dense_activations(y).astype(np.float64), -qa)
    assert np.array_equal(ma, np.round(ma))
    return y, w, b, _assert_units(ma, mw, mb, "hc,ptc->pht")


def exact_conv_case(rng, which, B, T, Cin, M, qa, qw, seed=177):
    """(x [B, T, Cin], w [M, Cin, 3], b [M], units), which in ("plain", "zeros"): |m| <= 15; `zeros` has a quarter of x at
    +-0.0 and an output channel of all-zero weights."""
    assert which in ("plain", "zeros")
    mx = rng.integers(seed, which + "x", (B, T, Cin), -15, 16).astype(np.float64)
    if which == "zeros":
        sel = rng.integers(seed, "sel", (B, T, Cin), 0, 8)
        mx[sel == 0] = 0.0
        mx[sel == 1] = -0.0
    x = _to_f32(mx, qa)
    assert np.array_equal(rne_bf16(x), x)
    mw, w = _exact_weights(rng, seed, "mw", (M, Cin, 3), 15, qw, zero_row=(which == "zeros"))
    mb, b = _exact_bias(rng, seed, M, qa + qw)
    units = int(conv_ref64(np.abs(mx), np.abs(mw).astype(np.float64)).max()) + int(np.abs(mb).max())
    assert units < (1 << 24), units
    return x, w, b, units


def exact_mean_case(rng, R, T, D, q, seed=178):
    """(x [R, T, D], want [R, D]).  T in {1, 2, 4, 8}: 8-bit integers 128 .. 255 (a third negative) times 2^q; the sum and the
    division by T are exact, so want = bf16(sum / T), ties included.  T = 3: the same integers; the sum s is exact and
    want = bf16(fl32(s / 3)), the kernel's own double rounding (s / 3 in float64 is never within 2^-29 of an fp32 tie: its
    binary expansion is periodic, so rounding it once more to fp32 is the correctly rounded fp32 quotient)."""
    assert T in (1, 2, 3, 4, 8)
    m = 128 + rng.integers(seed, f"m{T}", (R, T, D), 0, 128)
    m = np.where(rng.integers(seed, f"s{T}", (R, T, D), 0, 3) == 0, -m, m)
    x = _to_f32(m, q)
    assert np.array_equal(rne_bf16(x), x)
    s = m.sum(1).astype(np.float64)
    if T == 3:
        quot = (s / 3.0).astype(np.float32)
        assert np.array_equal(quot, (s.astype(np.float32) / np.float32(3.0)))
    else:
        quot = (s / T).astype(np.float32)
        assert np.array_equal(quot.astype(np.float64), s / T)
    want = rne_bf16(quot * _pow2(q)) + np.float32(0.0)                           # the scaling is exact; a zero mean is +0
    return x, want
