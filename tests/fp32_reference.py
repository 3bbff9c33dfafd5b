"""Host-side model of the fp32 scorer kernels (csrc/tspn_conv3.hip, tspn_heads.hip, tspn_linear.hip, tspn_pairs.hip), plain
numpy: float64 references, the error budget the kernels are held to, fp32 emulations of three summation orders with five
plantable defects, the eight input kinds and the exact-case generators of tests/test_gpu_fp32_bound.py (host side:
tests/test_fp32_reference_host.py).  Modelled on tests/bf16_reference.py, whose assumption it keeps.

The arithmetic.  Operands, accumulators and outputs are fp32.  Unlike bf16 operands, fp32 operands have products that are NOT
exact in fp32: w a has up to 48 significant bits.  Whether the hardware rounds a product before it adds it (unfused) or adds
it unrounded (fused) is charged either way: one rounding of every product is u |w a|, in total u S, and the budget carries
that term explicitly.  The sources: the MFMA kernels leave it to v_mfma_f32_*_f32, whose inner arithmetic is not specified;
the build passes -ffp-contract=off, so every `a * b + c` written in C++ is UNFUSED (the reduce kernels have none: they only
add); heads_pairgrid4_kernel, which the fused pass runs at H = 12, is written in v_pk_fma_f32: FUSED.  The emulators do both.

The budget.  u = 2^-24.  The ONLY assumption (bf16_reference.py's): every addition the hardware performs on an fp32 partial
sum errs by at most 2 u |partial|.  Nothing is assumed about the order inside an MFMA step.  With S = |b| + sum |w| |a|, a
contraction of depth Kd in MFMA steps of k costs k additions inside a step (charged once: the addends of step j are bounded
by S_j and sum_j S_j = S), Kd / k accumulator updates, `extra` further additions, and the products' roundings:
    |got - ref64|  <=  (2 (k + Kd / k + extra) + 1) u S          (K_of)
Per kernel (read from the sources):
    tspn_conv3_f32, tspn_conv3_tc_f32   conv3_mfma_kernel<VEC_A> ("vec" / "scalar"), conv3_mfma_dma_kernel<16 | 8> ("dma16" /
        "dma8"), conv3_mfma_cl_kernel: v_mfma_f32_32x32x2_f32, k = 2, ONE accumulator per output over the whole depth Kd = 3 Cin,
        walked one chunk of 16 (dma8: 8) channels x 3 taps at a time: Kd / k = 3 Cin / 2 updates.  extra = 2: the bias add of
        the epilogue and one spare.  The ReLU is monotone and 1-Lipschitz: the same budget after it.
    tspn_heads_f32 (heads_kernel<mode, vec2>), tspn_heads_pairgrid_f32 (heads_pairgrid_kernel<vec2>, heads_pairgrid3_kernel)
        v_mfma_f32_16x16x4_f32, k = 4, one accumulator per (pair, head, frame), Kd = C.  extra = 2 (the head bias, one spare).
        The activation is formed BEFORE the contraction by correctly rounded fp32 adds -- mode 1: relu((a + b) + bias) in
        that order, pair grid: relu(u + v) -- which heads_act / pairgrid_act form in numpy float32 exactly as the kernel
        does: charged to nobody, so a flip of the ReLU at a rounding boundary cannot happen between kernel and reference.
    tspn_predicate_head_f32   linear_splitk_kernel<false>: v_mfma_f32_16x16x4_f32, k = 4; the depth F is cut into `splits`
        slices of kps = ceil(ceil(F / splits) / 32) * 32 (choose_splits, restated as splits_of); slice z's accumulator takes
        kps / 4 updates on partial sums <= S_z and sum_z S_z = S, so Kd / k = kps / 4; linear_reduce_kernel then adds the
        `splits` slabs in order into one fp32 sum (partial sums <= S) and the bias: extra = splits + 2 (bias, one spare).
    tspn_predicate_head_norm_f32   linear_splitk_kernel<true> + linear_reduce_norm_kernel over the slices of split_table
        (build_split_table restated; a slice never straddles a normalisation block).  Per block the slices' partial dot
        products are added, their sum |x| are added to the block's L1 norm, and the block's sum is divided by it; then the
        blocks are added, then the bias.  extra = n + 2 + (steps + 5 + n + 1) where n = the table's slices (one addition per
        slice into the block sum or the row sum, bounded together by n), and the last bracket is the relative error, in units
        of 2 u, of sum / L1: a slice's sum |x| is `steps` = longest slice / 32 sequential additions per thread and 5 shuffle
        levels of non-negative terms, at most n slice norms are added, and the division rounds once.  S is taken on the
        NORMALISED operand: S = |b| + sum_blocks (sum |x| |w|) / L1 + the unnormalised columns' sum |x| |w|.
    tspn_temporal_mean_f32 / tspn_temporal_sum_f32   temporal_mean_td_kernel and temporal_mean_td4_kernel add the T frames
        in order into one fp32 sum (T - 1 additions; the first, on +0, is exact); temporal_mean_ct_kernel gives lane l the
        frames l, l + 64, .. and adds the 64 lane sums by a 6-level shuffle tree, in which an addition of a lane that holds
        no frame adds 0 and is exact: any tree over T frames has T - 1 additions that can err, and no frame passes more.
        Each errs by at most 2 u sum |x|: the sum lies within e_s = 2 (T - 1) u sum |x| of the float64 sum s (at T = 1 it IS
        the frame).  The mean divides ONCE by (float)T (T is exact; HIP's fp32 division is correctly rounded) and rounding
        is monotone, so  fl32((s - e_s) / T) <= mean <= fl32((s + e_s) / T)  and  fl32(s - e_s) <= sum <= fl32(s + e_s):
        intervals, not tolerances (mean_interval, sum_interval).
At Cin = 8 the conv's budget is 33 u S (the suite's absolute 2e-5 is about 350 u S there), at Cin = 2048 6153 u S = 3.7e-4
S; the heads at C = 21: 23.5 u S.  Nothing in a budget is measured.

The floor.  SUBNORMAL_FLOOR is the absolute error per term that the contract allows when an operand is an fp32 subnormal;
its candidate value was the smallest normal, 2^-126, times the other operand's magnitude, i.e. the error of a hardware that
reads a subnormal operand as zero.  Whether v_mfma_f32_32x32x2_f32 and v_mfma_f32_16x16x4_f32 do that is not documented, so
the `subnormal` kind measures it: tests/test_gpu_fp32_bound.py prints the worst error in units of the budget and of that
flush error.  The GPU run decided it: on gfx950 both MFMAs and the fp32 adds in front of them KEEP subnormals -- every entry
stays within 0.14 of the floor-less budget on `subnormal`, where a flush would be 1.7e3 to 6.9e5 budgets -- so the floor is 0,
and include/tspn_mi355x.h and DESIGN.md 3 say so.

The kinds (make_conv_case / make_heads_case / make_linear_case / make_mean_case), all deterministic through hashrng:
    unit         the suite's distribution: activations U(-1, 1), weights N(0, 0.1^2) (linear: 0.05^2)
    large        activations 2^13 times that, weights 2^-13 times
    tiny         activations 2^-100 times, weights 2^90 times (outputs around 2^-10)
    hot_channel  one channel in every 16 is 2^12 times the others
    cancelling   activations 1 + 2^-4 U(-1, 1) against weights of alternating sign in pairs of equal magnitude: |ref| << S
    wide         per-channel powers of two, 2^-20 .. 2^20, on the activations and (independently) on the weights
    relu_edge    (modes with a ReLU in front of the contraction: heads mode 1, pair grid)  b = -a (1 + 2^-10 U(-1, 1)): half
                 the activations vanish, the others are ten or more binades below |a|
    subnormal    activations U(-1, 1) 2^-127 (heads: 2^-129, so that a + b + bias is subnormal too): fp32 subnormals; weights
                 2^100 times, bias 2^-30 times

The exact cases (exact_conv_case / exact_heads_case / exact_linear_case / exact_norm_case / exact_mean_case).  Operands are
small integers times ONE power of two per tensor, a = m_a 2^qa, w = m_w 2^qw, the bias an integer in the unit 2^(qa + qw);
the generator asserts sum |m_w| |m_a| + |bias| < 2^24 units.  Then every product and every partial sum of every order is an
integer below 2^24 units: exact in fp32, and the output must equal float32(ref64) bit for bit.  (qa, qw) runs over Q_PAIRS.
    plain   |m| <= 15, and ONE channel (the last) whose activations are odd 24-bit integers (2^23 - 2^20 .. 2^23) against weights
            in {-1, 0, 1} (the conv: on the centre tap only): an MFMA path that kept fewer than 24 operand bits would not
            return these bits
    zeros   a quarter of the activations are +0 / -0; where there is a ReLU in front, u + v is exactly 0 and exactly -1 unit;
            one all-zero weight row whose output is exactly its bias, and (four rows or more) two more all-zero rows whose
            biases are 0 and -1 unit: a conv output of exactly 0 and of exactly -1 unit under the epilogue's ReLU
The sign of a zero output: DESIGN.md 2 freezes none for these entries, and what an MFMA returns for (+0) + (-0 x w) is not
specified, so -0 is folded onto +0 on both sides (fold_zero) before the bits are compared.
Mean and sum are exact for EVERY T: integer frames |m| < 2^16 times 2^q, T <= 150: the frame sum is an integer below 2^24
units, exact in any order; the sum's reference is s, the mean's float32(float32(s) / float32(T)), the one division.
Block-L1: every normalisation block of every row has integer entries (unit 2^qa) whose L1 norm is made 2^NORM_P units by
growing one entry; one block of one row is all zero (divides by 1); the columns outside the blocks are integers in the unit
2^-NORM_P, so that every slice sum, every slice norm, every quotient and the reduce run in ONE unit, 2^(qw - NORM_P).
The fp32 F(6,3) form has no exact case (its transform entries are not dyadic) and keeps tests/test_gpu_wino63.py.

The planted defects of the host test (contract_emulate / conv_emulate arguments), and what cannot show them:
    drop        a dropped channel: |w a_c|, about S / Kd on kinds whose channels are alike.  On `hot_channel` a cold channel
                is 2^-12 of a hot one and on `wide` a channel's share is whatever was drawn: the host test drops the hot
                channel / the largest share there.  At Cin = 2048 the share S / 6144 = 1.6e-4 S is BELOW the conv's budget
                3.7e-4 S: the full-depth conv sees a dropped channel on the exact cases and on `hot_channel` only.
    double      a doubled tap (counted twice): as a dropped one.
    leak        the -1 / +1 taps read across a sequence boundary: changes the first and last frame of every sequence but the
                outermost; about S / 3 there on every kind.
    trunc19     one 16-channel chunk of the activations cut to 19 mantissa bits (xf32-like): at most 2^-19 = 32 u of that
                chunk's share of S with signs that mix, against budgets of 23.5 u S and more: at or below the budget on
                every kind with normal operands (the host test prints the ratio and asserts nothing about it), so no
                budget can be relied on to show it.  It is the `plain` exact case's 24-bit channel that shows it.
    bias_shift  bias[m + 1] for bias[m]: about |b| = 0.1 against S of a few units on `unit`, `large`, `cancelling`, `relu_edge`
                and, up to 48 channels, `hot_channel`; on `wide` |b| can be far below S, at Cin = 2048 the conv's budget (3.7e-4
                S, S in the hundreds) is |b| itself, and 128 hot channels put S in the ten thousands: asserted on the exact
                cases, and on the kinds named first at the depths where 0.1 stands above the budget.
"""
import numpy as np

U = 2.0 ** -24
SMALLEST_NORMAL = 2.0 ** -126
SUBNORMAL_FLOOR = 0.0           # the kernels keep fp32 subnormals (module docstring): no absolute floor
K_CONV, K_HEADS, K_LIN = 2, 4, 4   # v_mfma_f32_32x32x2_f32; v_mfma_f32_16x16x4_f32 (heads, pair grid, split-K GEMM)
CHUNK = 16                      # channels per staged chunk (conv, pair grid); the hot channel's period
KINDS = ("unit", "large", "tiny", "hot_channel", "cancelling", "wide", "relu_edge", "subnormal")
PLAIN_KINDS = tuple(k for k in KINDS if k != "relu_edge")
MEAN_KINDS = ("unit", "large", "tiny", "wide", "cancelling")
EXACT_KINDS = ("plain", "zeros")
Q_PAIRS = ((0, 0), (-1, 7), (7, -1), (-100, 100), (100, -100), (100, 0), (0, 100), (-100, 0), (0, -100))
Q_MEAN = (-100, -1, 0, 7, 100)
NORM_P = 13                     # every block's L1 norm is 2^13 units in exact_norm_case


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def fold_zero(x):
    """-0 -> +0 (module docstring: the sign of a zero output)."""
    return np.asarray(x, np.float32) + np.float32(0.0)


def relu32(x):
    x = np.asarray(x, np.float32)
    return np.where(x > 0, x, np.float32(0.0)).astype(np.float32)


def trunc19(x):
    """The planted defect: 19 explicit mantissa bits kept, the low four dropped."""
    return (bits(x) & np.uint32(0xFFFFFFF0)).view(np.float32).reshape(np.shape(x))


def K_of(Kd, k, extra=2):
    """The budget in units of u S: 2 (k + Kd / k + extra) + 1."""
    return 2.0 * (k + Kd / k + extra) + 1.0


# ------------------------------------------------------------------------------------------------ conv
def conv_cols(x, leak=False):
    """x [B, T, Cin] -> [B * T, 3 * Cin] in (tap, channel) order, zero outside [0, T); `leak`: the planted defect, the +-1 taps
    read the neighbouring sequence's frame (flat columns, zero only outside the whole batch)."""
    x = np.asarray(x)
    B, T, Cin = x.shape
    if leak:
        flat = np.pad(x.reshape(B * T, Cin), ((1, 1), (0, 0)))
        return np.concatenate([flat[k:k + B * T] for k in range(3)], 1)
    xp = np.pad(x, ((0, 0), (1, 1), (0, 0)))
    return np.concatenate([xp[:, k:k + T] for k in range(3)], 2).reshape(B * T, 3 * Cin)


def conv_wmat(w):
    """w [M, Cin, 3] -> [M, 3 * Cin] in (tap, channel) order."""
    w = np.asarray(w)
    return w.transpose(0, 2, 1).reshape(w.shape[0], -1)


def _from_cols(r, B, T):
    return r.reshape(B, T, -1).transpose(0, 2, 1)


def conv_ref64(x, w, b=None, relu=False):
    """float64 [B, M, T]: (relu of) b_m + sum_{c,k} w[m, c, k] x[b, t + k - 1, c]; x [B, T, Cin], w [M, Cin, 3]."""
    B, T, _ = np.shape(x)
    r = conv_cols(np.asarray(x, np.float64)) @ conv_wmat(np.asarray(w, np.float64)).T
    if b is not None:
        r = r + np.asarray(b, np.float64)[None, :]
    return _from_cols(np.maximum(r, 0.0) if relu else r, B, T)


def conv_S(x, w, b=None):
    return conv_ref64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                      None if b is None else np.abs(np.asarray(b, np.float64)))


def conv_budget(x, w, b=None):
    """float64 [B, M, T]: (2 (2 + 3 Cin / 2 + 2) + 1) u S (+ the subnormal floor times sum |w|, 0 unless it is set)."""
    w64 = np.abs(np.asarray(w, np.float64))
    return K_of(3 * w64.shape[1], K_CONV) * U * conv_S(x, w, b) + SUBNORMAL_FLOOR * w64.sum((1, 2))[None, :, None]


# ------------------------------------------------------------------------------------------------ heads, pair grid
def heads_act(mode, a, ia, b=None, ib=None, bias=None):
    """fp32 [P, C, T], the activation heads_kernel<mode> forms: mode 0 a[ia]; mode 1 relu((a[ia] + b[ib]) + bias[c]), two
    correctly rounded fp32 adds in the kernel's order (the bias add is skipped without a bias)."""
    a = np.asarray(a, np.float32)
    if mode == 0:
        return a[ia]
    h = a[ia] + np.asarray(b, np.float32)[ib]
    if bias is not None:
        h = h + np.asarray(bias, np.float32)[None, :, None]
    return relu32(h)


def pair_table(B, N):
    """[B*N*(N-1), 2] global tracklet ids of the canonical table: per video, s-major, o != s."""
    s, o = np.divmod(np.arange(N * N), N)
    loc = np.stack([s, o], 1)[s != o]
    return np.concatenate([loc + b * N for b in range(B)])


def pairgrid_act(y, B, N):
    """y fp32 [B*N, 2C, T] -> fp32 [P, C, T]: relu(u_s + v_o), one fp32 add, on the canonical table."""
    y = np.asarray(y, np.float32)
    C = y.shape[1] // 2
    tab = pair_table(B, N)
    return relu32(y[tab[:, 0], :C] + y[tab[:, 1], C:])


def heads_ref64(h, w, bh=None):
    """float64 [P, H, T]: bh_o + sum_c w[o, c] h[p, c, t]."""
    r = np.einsum("hc,pct->pht", np.asarray(w, np.float64), np.asarray(h, np.float64))
    return r if bh is None else r + np.asarray(bh, np.float64)[None, :, None]


def heads_S(h, w, bh=None):
    return heads_ref64(np.abs(np.asarray(h, np.float64)), np.abs(np.asarray(w, np.float64)),
                       None if bh is None else np.abs(np.asarray(bh, np.float64)))


def heads_budget(h, w, bh=None):
    """float64 [P, H, T]: (2 (4 + C / 4 + 2) + 1) u S."""
    w64 = np.abs(np.asarray(w, np.float64))
    return K_of(w64.shape[1], K_HEADS) * U * heads_S(h, w, bh) + SUBNORMAL_FLOOR * w64.sum(1)[None, :, None]


# ------------------------------------------------------------------------------------------------ split-K GEMM
def splits_of(P, F, K):
    """choose_splits of tspn_linear.hip, restated (as in tests/test_gpu_kernel_variants.py)."""
    tiles = -(-P // 64) * -(-K // 144)
    return max(min(-(-512 // tiles), max(1, F // 64), 64), 1)


def kps_of(F, splits):
    return -(-(-(-F // splits)) // 32) * 32


def linear_ref64(x, w, b=None):
    r = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    return r if b is None else r + np.asarray(b, np.float64)[None, :]


def linear_S(x, w, b=None):
    return linear_ref64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                        None if b is None else np.abs(np.asarray(b, np.float64)))


def linear_K(F, splits):
    return K_of(kps_of(F, splits), K_LIN, extra=splits + 2)


def linear_budget(x, w, b=None, splits=None):
    """float64 [P, K]: (2 (4 + kps / 4 + splits + 2) + 1) u S; splits = splits_of(P, F, K) unless given (a host test on a few
    rows of a larger problem)."""
    P, F = np.shape(x)
    w64 = np.abs(np.asarray(w, np.float64))
    splits = splits_of(P, F, w64.shape[0]) if splits is None else splits
    return linear_K(F, splits) * U * linear_S(x, w, b) + SUBNORMAL_FLOOR * w64.sum(1)[None, :]


def split_table(P, F, K, first, block, nblocks):
    """build_split_table of tspn_linear.hip, restated: [(kbeg, kend, block id or -1)]."""
    cd = lambda a, b: -(-a // b)    # noqa: E731
    tiles = cd(P, 64) * cd(K, 144)
    target = min(max(cd(512, tiles), 1), 64)
    length = max(cd(cd(F, target), 32) * 32, 64)
    tab = []

    def add(lo, hi, blk):
        if hi <= lo:
            return
        pieces = cd(hi - lo, length)
        step = cd(cd(hi - lo, pieces), 32) * 32
        for k in range(lo, hi, step):
            tab.append((k, min(k + step, hi), blk))

    add(0, first, -1)
    for bl in range(nblocks):
        add(first + bl * block, first + (bl + 1) * block, bl)
    add(first + nblocks * block, F, -1)
    assert len(tab) <= 128
    return tab


def block_l1(x, first, block, nblocks):
    """float64 [P, F]: the divisor of every column under oracle.feature_preprocess's rules (1 outside the blocks and for an
    all-zero block)."""
    x64 = np.asarray(x, np.float64)
    d = np.ones_like(x64)
    for k in range(nblocks):
        lo = first + k * block
        l1 = np.abs(x64[:, lo:lo + block]).sum(1, keepdims=True)
        d[:, lo:lo + block] = np.where(l1 == 0, 1.0, l1)
    return d


def norm_ref64(x, w, b, first, block, nblocks):
    return linear_ref64(np.asarray(x, np.float64) / block_l1(x, first, block, nblocks), w, b)


def norm_S(x, w, b, first, block, nblocks):
    return linear_S(np.asarray(x, np.float64) / block_l1(x, first, block, nblocks), w, b)


def norm_K(P, F, K, first, block, nblocks):
    tab = split_table(P, F, K, first, block, nblocks)
    n = len(tab)
    longest = max(e - s for s, e, _ in tab)
    steps = -(-longest // 32)
    return K_of(-(-longest // 32) * 32, K_LIN, extra=n + 2 + (steps + 5 + n + 1))


def norm_budget(x, w, b, first, block, nblocks):
    P, F = np.shape(x)
    return norm_K(P, F, np.shape(w)[0], first, block, nblocks) * U * norm_S(x, w, b, first, block, nblocks)


# ------------------------------------------------------------------------------------------------ mean, sum
def _interval(x):
    x64 = np.asarray(x, np.float64)
    T = x64.shape[1]
    s = x64.sum(1)
    e = 2.0 * (T - 1) * U * np.abs(x64).sum(1)
    return s - e, s + e, T


def sum_interval(x):
    """x [R, T, D] -> (lo, hi) fp32 [R, D]: fl32(s - e_s) <= sum <= fl32(s + e_s), e_s = 2 (T - 1) u sum |x| (module docstring)."""
    lo, hi, _ = _interval(x)
    return lo.astype(np.float32), hi.astype(np.float32)


def mean_interval(x):
    """x [R, T, D] -> (lo, hi) fp32 [R, D]: fl32((s -+ e_s) / T)."""
    lo, hi, T = _interval(x)
    return (lo / T).astype(np.float32), (hi / T).astype(np.float32)


def mean_emulate(x, form="td", mean=True):
    """fp32 emulation: "td" the frames in order (temporal_mean_td_kernel, td4); "ct" 64 strided lane sums and the shuffle tree
    acc += shfl_down(acc, off), off = 32 .. 1 (lane 0's value: lanes past the wave read their own value, which lane 0 never
    receives); "pairwise" a balanced tree.  One division by float32(T)."""
    x = np.asarray(x, np.float32)
    R, T, D = x.shape
    if form == "td":
        acc = np.zeros((R, D), np.float32)
        for t in range(T):
            acc = acc + x[:, t]
    elif form == "ct":
        lanes = np.zeros((64, R, D), np.float32)
        for t in range(T):
            lanes[t % 64] = lanes[t % 64] + x[:, t]
        off = 32
        while off:
            nxt = lanes.copy()
            nxt[:64 - off] = lanes[:64 - off] + lanes[off:]
            lanes = nxt
            off //= 2
        acc = lanes[0]
    else:
        p = [x[:, t] for t in range(T)]
        while len(p) > 1:
            p = [p[i] + p[i + 1] if i + 1 < len(p) else p[i] for i in range(0, len(p), 2)]
        acc = p[0] + np.float32(0.0)
    return acc / np.float32(T) if mean else acc


# ------------------------------------------------------------------------------------------------ fp32 emulations
ORDERS = ("sequential", "blocks", "pairwise")


def contract_emulate(a, w, b=None, order="blocks", k=2, fused=False, drop=None, double=None, trunc_chunk=None, bias_shift=False,
                     chunk=CHUNK):
    """fp32 emulation of out[r, h] = b_h + sum_j w[h, j] a[r, j] for a [R, Kd], w [H, Kd], both fp32.
    order: "sequential" one product at a time into one fp32 accumulator; "blocks" the k products of a step summed in float64,
    one fp32 rounding per step into the accumulator (k-blocked as the kernel, an MFMA whose inner sum is exact); "pairwise" a
    balanced tree of fp32 additions.  fused = False rounds every product to fp32 first (-ffp-contract=off, an MFMA that rounds
    its products); fused = True adds the unrounded product (v_pk_fma_f32; in "pairwise" the leaves are necessarily rounded).
    The bias is added last, in fp32.  Planted defects: `drop` a column left out, `double` a column counted twice,
    `trunc_chunk` the columns [chunk * i, chunk * i + chunk) of a cut to 19 mantissa bits, `bias_shift` b rolled by one."""
    a32, w32 = np.asarray(a, np.float32), np.asarray(w, np.float32)
    if trunc_chunk is not None:
        a32 = a32.copy()
        sl = slice(trunc_chunk * chunk, (trunc_chunk + 1) * chunk)
        a32[:, sl] = trunc19(a32[:, sl])
    idx = np.arange(a32.shape[1])
    if drop is not None:
        idx = idx[idx != drop]
    if double is not None:
        idx = np.sort(np.concatenate([idx, [double]]))
    a64, w64 = a32[:, idx].astype(np.float64), w32[:, idx].astype(np.float64)
    R, Kd = a64.shape
    H = w64.shape[0]
    rnd = (lambda p: p) if fused else (lambda p: p.astype(np.float32).astype(np.float64))
    with np.errstate(under="ignore"):
        if order == "sequential":
            acc = np.zeros((R, H), np.float32)
            for j in range(Kd):
                acc = (acc + rnd(a64[:, j, None] * w64[None, :, j])).astype(np.float32)
        elif order == "blocks":
            acc = np.zeros((R, H), np.float32)
            for j in range(0, Kd, k):
                acc = (acc + rnd(a64[:, None, j:j + k] * w64[None, :, j:j + k]).sum(2)).astype(np.float32)
        elif order == "pairwise":
            p = (a64[:, None, :] * w64[None, :, :]).astype(np.float32)
            while p.shape[2] > 1:
                if p.shape[2] % 2:
                    p = np.concatenate([p, np.zeros(p.shape[:2] + (1,), np.float32)], 2)
                p = p[:, :, 0::2] + p[:, :, 1::2]
            acc = p[:, :, 0]
        else:
            raise ValueError(order)
    if b is None:
        return acc
    b32 = np.asarray(b, np.float32)
    return acc + (np.roll(b32, -1) if bias_shift else b32)[None, :]


def conv_emulate(x, w, b=None, relu=False, leak=False, **kw):
    """contract_emulate on the im2col of x [B, T, Cin] in the kernel's order (16-channel chunk, then channel pair, then tap:
    one MFMA = two channels of one tap) -> [B, M, T].  drop / double name a column of THIS order; trunc_chunk a 16-channel
    chunk (all three taps of it)."""
    x = np.asarray(x, np.float32)
    B, T, Cin = x.shape
    cols = conv_cols(x, leak=leak).reshape(B * T, 3, Cin)
    wm = np.asarray(w, np.float32).transpose(0, 2, 1)                              # [M, 3, Cin]
    if Cin % 2 == 0:        # (pair, tap, 2): the kernel's MFMA steps
        cols = cols.reshape(B * T, 3, Cin // 2, 2).transpose(0, 2, 1, 3).reshape(B * T, 3 * Cin)
        wm = wm.reshape(-1, 3, Cin // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 3 * Cin)
        kw.setdefault("chunk", 3 * CHUNK)
    else:                   # odd Cin: (channel, tap); the kernel pads the last pair with a zero channel
        cols = cols.transpose(0, 2, 1).reshape(B * T, 3 * Cin)
        wm = wm.transpose(0, 2, 1).reshape(-1, 3 * Cin)
        kw.setdefault("chunk", 3 * CHUNK)
    r = contract_emulate(cols, wm, b, k=K_CONV, **kw)
    return _from_cols(relu32(r) if relu else r, B, T)


def conv_col(Cin, c, tap):
    """The column of channel c, tap `tap` in conv_emulate's order."""
    return (c // 2) * 6 + tap * 2 + c % 2 if Cin % 2 == 0 else c * 3 + tap


def heads_emulate(h, w, bh=None, **kw):
    """contract_emulate on h [P, C, T] -> [P, H, T]."""
    P, C, T = h.shape
    r = contract_emulate(np.asarray(h).transpose(0, 2, 1).reshape(P * T, C), w, bh, k=K_HEADS, **kw)
    return r.reshape(P, T, -1).transpose(0, 2, 1)


def linear_emulate(x, w, b=None, splits=1, order="blocks", fused=False, **kw):
    """The split-K GEMM: `splits` slices of kps columns each summed by contract_emulate, then added in order, then the bias."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    F = x.shape[1]
    kps = kps_of(F, splits)
    s = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for z in range(splits):
        sl = slice(z * kps, min((z + 1) * kps, F))
        if sl.start < F:
            s = s + contract_emulate(x[:, sl], w[:, sl], None, order=order, k=K_LIN, fused=fused, **kw)
    return s if b is None else s + np.asarray(b, np.float32)[None, :]


def norm_emulate(x, w, b, first, block, nblocks, order="blocks", fused=False):
    """linear_splitk_kernel<true> + linear_reduce_norm_kernel in fp32: per slice a partial product and sum |x| (fp32, in
    order), per block acc / (l1 == 0 ? 1 : l1), the blocks added in table order, then the bias."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    P, F = x.shape
    tab = split_table(P, F, w.shape[0], first, block, nblocks)
    s = np.zeros((P, w.shape[0]), np.float32)
    z = 0
    while z < len(tab):
        blk = tab[z][2]
        acc = np.zeros_like(s)
        l1 = np.zeros((P, 1), np.float32)
        while z < len(tab) and tab[z][2] == blk:
            sl = slice(tab[z][0], tab[z][1])
            acc = acc + contract_emulate(x[:, sl], w[:, sl], None, order=order, k=K_LIN, fused=fused)
            if blk >= 0:
                part = np.zeros((P, 1), np.float32)
                for j in range(sl.start, sl.stop):
                    part = part + np.abs(x[:, j:j + 1])
                l1 = l1 + part
            z += 1
        if blk >= 0:
            acc = acc / np.where(l1 == 0, np.float32(1.0), l1)
        s = s + acc
    return s if b is None else s + np.asarray(b, np.float32)[None, :]


# ------------------------------------------------------------------------------------------------ the kinds
def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e, np.int32)).astype(np.float32)


def hot_index(n, k=CHUNK):
    """One channel in every full block of k: block j's hot channel (none if n < k: then channel n - 1)."""
    if n < k:
        return np.array([n - 1])
    j = np.arange(n // k)
    return j * k + (7 * j + 5) % k


def _shape_kind(rng, seed, kind, a, w, b, caxis, std):
    """Applies `kind` to activations a (channel axis `caxis`), weights w [rows, C, ...] and bias b."""
    C = a.shape[caxis]
    cshape = [1] * a.ndim
    cshape[caxis] = C
    wshape = [1] * w.ndim
    wshape[1] = C
    if kind == "large":
        a, w = a * np.float32(2.0 ** 13), w * np.float32(2.0 ** -13)
    elif kind == "tiny":
        a, w, b = a * np.float32(2.0 ** -100), w * np.float32(2.0 ** 90), b * np.float32(2.0 ** -10)
    elif kind == "hot_channel":
        m = np.ones(C, np.float32)
        m[hot_index(C)] = 4096.0
        a = a * m.reshape(cshape)
    elif kind == "cancelling":
        a = (1.0 + rng.uniform(seed, "ac", a.shape, -1, 1) * np.float32(2.0 ** -4)).astype(np.float32)
        mag = np.abs(rng.normal(seed, "wc", w.shape, std=std)) + np.float32(0.5 * std)
        half = np.take(mag, np.arange(C) // 2 * 2, axis=1)                       # channels 2i and 2i + 1 share a magnitude
        sign = np.where(np.arange(C) % 2, -1.0, 1.0).astype(np.float32).reshape(wshape)
        w = half * sign
        if C % 2:
            w = w * (np.arange(C) < C - 1).reshape(wshape)                       # an odd last channel has no partner
        b = b * np.float32(2.0 ** -6)
    elif kind == "wide":
        a = a * _pow2(rng.integers(seed, "ea", (C,), -20, 21)).reshape(cshape)
        w = w * _pow2(rng.integers(seed, "ew", (C,), -20, 21)).reshape(wshape)
    elif kind == "subnormal":
        a, w, b = a * np.float32(2.0 ** -127), w * np.float32(2.0 ** 100), b * np.float32(2.0 ** -30)
        assert float(np.abs(a).max()) < SMALLEST_NORMAL and bool((a != 0).any())
    f = lambda v: np.ascontiguousarray(v, np.float32)   # noqa: E731
    return f(a), f(w), f(b)


def make_conv_case(rng, kind, B, T, Cin, M, seed=301):
    """(x fp32 [B, T, Cin], w fp32 [M, Cin, 3], b fp32 [M]) of `kind`."""
    assert kind in PLAIN_KINDS, kind
    x = rng.uniform(seed, "x", (B, T, Cin), -1, 1)
    w = rng.normal(seed, "w", (M, Cin, 3), std=0.1)
    b = rng.normal(seed, "b", (M,), std=0.1)
    return _shape_kind(rng, seed, kind, x, w, b, 2, 0.1)


def make_heads_case(rng, kind, R, C, T, H, seed=302):
    """(a, b fp32 [R, C, T], bias fp32 [C], w fp32 [H, C], bh fp32 [H]) of `kind`: mode 0 reads a alone; mode 1 and the pair grid
    (y = cat(a, b) on the channel axis) form relu(a + b (+ bias)).  `relu_edge`: b = -a (1 + 2^-10 U(-1, 1)) and no bias."""
    assert kind in KINDS, kind
    a = rng.uniform(seed, "a", (R, C, T), -1, 1)
    w = rng.normal(seed, "w", (H, C), std=0.1)
    bh = rng.normal(seed, "bh", (H,), std=0.1)
    bias = rng.normal(seed, "bias", (C,), std=0.3)
    if kind == "relu_edge":
        base = np.broadcast_to(a[:1], a.shape)            # ONE shared row, so that every (ia, ib) sits on the edge
        b = -base * (1 + rng.uniform(seed, "bd", a.shape, -1, 1) * np.float32(2.0 ** -10))
        a = base * (1 + rng.uniform(seed, "ad", a.shape, -1, 1) * np.float32(2.0 ** -10))
        f = lambda v: np.ascontiguousarray(v, np.float32)   # noqa: E731
        return f(a), f(b), np.zeros(C, np.float32), f(w), f(bh)
    a2, w, bh = _shape_kind(rng, seed, kind, a, w, bh, 1, 0.1)
    scale = np.float32(np.abs(a2).max() / np.abs(a).max()) if kind in ("large", "tiny", "subnormal") else np.float32(1.0)
    b = rng.uniform(seed, "b", (R, C, T), -1, 1) * scale
    if kind in ("hot_channel", "wide"):
        ratio = np.abs(a2).max((0, 2)) / np.maximum(np.abs(a).max((0, 2)), 1e-30)
        b = b * _pow2(np.round(np.log2(ratio)))[None, :, None]
    if kind == "cancelling":
        b = np.zeros_like(b)
        bias = np.zeros_like(bias)
    if kind == "subnormal":             # (a + b) + bias stays below the smallest normal: three terms of at most 2^-129 each
        a2, scale = a2 * np.float32(0.25), scale * np.float32(0.25)
        b = b * np.float32(0.25)
    return a2, np.ascontiguousarray(b, np.float32), np.ascontiguousarray(bias * scale, np.float32), w, bh


def make_linear_case(rng, kind, P, F, K, seed=303):
    """(x fp32 [P, F], w fp32 [K, F], b fp32 [K]) of `kind`."""
    assert kind in PLAIN_KINDS, kind
    x = rng.uniform(seed, "x", (P, F), -1, 1)
    w = rng.normal(seed, "w", (K, F), std=0.05)
    b = rng.normal(seed, "b", (K,), std=0.1)
    return _shape_kind(rng, seed, kind, x, w, b, 1, 0.05)


def make_mean_case(rng, kind, R, T, D, seed=304):
    """x fp32 [R, T, D]."""
    assert kind in MEAN_KINDS, kind
    x = rng.uniform(seed, "x", (R, T, D), -1, 3)
    if kind == "large":
        x = x * np.float32(2.0 ** 13)
    elif kind == "tiny":
        x = x * np.float32(2.0 ** -100)
    elif kind == "wide":
        x = x * _pow2(rng.integers(seed, "e", (R, T, D), -20, 21))
    elif kind == "cancelling":
        x = (1.0 + rng.uniform(seed, "xc", (R, T, D)) * np.float32(2.0 ** -4)) * np.where(np.arange(T) % 2, -1.0, 1.0)[None, :, None]
    return np.ascontiguousarray(x, np.float32)


# ------------------------------------------------------------------------------------------------ the exact cases
WIDE_LO, WIDE_HI = (1 << 23) - (1 << 20), 1 << 23


def _to_f32(m, q):
    x64 = np.ldexp(np.asarray(m, np.float64), q)
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64) and bool(np.isfinite(x).all())
    assert bool(((x == 0) | (np.abs(x) >= SMALLEST_NORMAL)).all()), "an exact operand is subnormal"
    return x


def _exact_acts(rng, seed, tag, which, shape, caxis, wide=True):
    """Integer activations (float64, -0.0 included) of `shape`: |m| <= 15; `plain` with wide = True: the last channel holds odd
    24-bit integers; `zeros`: a quarter +0 / -0."""
    m = rng.integers(seed, tag, shape, -15, 16).astype(np.float64)
    if which == "zeros":
        sel = rng.integers(seed, tag + "sel", shape, 0, 8)
        m[sel == 0] = 0.0
        m[sel == 1] = -0.0
    elif wide:
        big = (rng.integers(seed, tag + "big", shape, WIDE_LO // 2, WIDE_HI // 2) * 2 + 1).astype(np.float64)
        big = big * np.where(rng.integers(seed, tag + "sgn", shape, 0, 2) == 0, -1.0, 1.0)
        last = [slice(None)] * len(shape)
        last[caxis] = shape[caxis] - 1
        m[tuple(last)] = big[tuple(last)]
    return m


def _exact_weights(rng, seed, which, shape, wide=True):
    """Integer weights [rows, C, ...]: |m| <= 15; `plain` with wide: the last channel's weights are in {-1, 0, 1} (a conv: on
    the centre tap only); `zeros`: the all-zero rows of the module docstring.  Returns (m, rows whose weights are all zero)."""
    m = rng.integers(seed, "mw", shape, -15, 16)
    rows = shape[0]
    zero_rows = []
    if which == "zeros":
        if rows >= 2:
            zero_rows = [rows // 2]
        if rows >= 4:
            zero_rows += [rows // 2 + 1, rows // 2 - 1]
        m[zero_rows] = 0
    elif wide:
        m[:, -1] = rng.integers(seed, "mw1", m[:, -1].shape, -1, 2)
        if len(shape) == 3:
            m[:, -1, 0] = 0
            m[:, -1, 2] = 0
    return m, zero_rows


def _exact_bias(rng, seed, n, zero_rows):
    mb = rng.integers(seed, "mb", (n,), -1000, 1001)
    mb[mb == 0] = 3
    if len(zero_rows) == 3:
        mb[zero_rows[1]] = -1           # an output of exactly -1 unit
        mb[zero_rows[2]] = 0            # and of exactly 0
    return mb


def _units(tot, mb):
    top = int(np.max(tot)) + int(np.abs(mb).max())
    assert top < (1 << 24), f"{top} units in one output"
    return top


def exact_conv_case(rng, which, B, T, Cin, M, qa, qw, seed=311):
    """(x [B, T, Cin], w [M, Cin, 3], b [M], units, zero_rows)."""
    assert which in EXACT_KINDS
    mx = _exact_acts(rng, seed, "mx", which, (B, T, Cin), 2)
    mw, zero_rows = _exact_weights(rng, seed, which, (M, Cin, 3))
    mb = _exact_bias(rng, seed, M, zero_rows)
    units = _units(conv_ref64(np.abs(mx), np.abs(mw).astype(np.float64)), mb)
    return _to_f32(mx, qa), _to_f32(mw, qw), _to_f32(mb, qa + qw), units, zero_rows


def exact_heads_case(rng, which, R, C, T, H, qa, qw, seed=312):
    """(a, b [R, C, T], bias [C], w [H, C], bh [H], units, zero_rows).  Mode 0 reads a; mode 1 relu((a + b) + bias) and the pair
    grid relu(a_s + b_o) on ANY (s, o): |a|, |b| <= 15, bias in -3 .. 3, so every sum is an exact integer; `plain`: a's last
    channel is a positive odd 24-bit integer and b's and the bias's last channel are 0; `zeros`: b = -a, b = -a - 1 and -0.0
    are planted where a and b belong to the SAME row index (ia == ib rows and s == o never occur on the grid, so the grid's
    zeros come from the quarter of zero inputs).  units bounds every output of every (ia, ib)."""
    assert which in EXACT_KINDS
    ma = _exact_acts(rng, seed, "ma", which, (R, C, T), 1)
    mbb = _exact_acts(rng, seed, "mb2", which, (R, C, T), 1, wide=False)
    mbias = rng.integers(seed, "mbias", (C,), -3, 4).astype(np.float64)
    if which == "plain":
        ma[:, -1] = np.abs(ma[:, -1])
        mbb[:, -1] = 0.0
        mbias[-1] = 0.0
    else:
        sel = rng.integers(seed, "uv", (R, C, T), 0, 8)
        mbb = np.where(sel == 2, -ma - mbias[None, :, None], mbb)               # (a + b) + bias = 0 on the same row
        mbb = np.where(sel == 3, -ma - mbias[None, :, None] - 1, mbb)           # -1 unit
    mw, zero_rows = _exact_weights(rng, seed, which, (H, C))
    mb = _exact_bias(rng, seed, H, zero_rows)
    amax = np.maximum(np.abs(ma).max(0), 0) + np.abs(mbb).max(0) + np.abs(mbias)[:, None]      # [C, T]: any (ia, ib)
    units = _units(np.abs(mw).astype(np.float64) @ amax, mb)
    return (_to_f32(ma, qa), _to_f32(mbb, qa), _to_f32(mbias, qa), _to_f32(mw, qw), _to_f32(mb, qa + qw), units, zero_rows)


def exact_linear_case(rng, which, P, F, K, qa, qw, seed=313):
    """(x [P, F], w [K, F], b [K], units, zero_rows)."""
    assert which in EXACT_KINDS
    mx = _exact_acts(rng, seed, "mx", which, (P, F), 1)
    mw, zero_rows = _exact_weights(rng, seed, which, (K, F))
    mb = _exact_bias(rng, seed, K, zero_rows)
    units = _units(np.abs(mx) @ np.abs(mw).astype(np.float64).T, mb)
    return _to_f32(mx, qa), _to_f32(mw, qw), _to_f32(mb, qa + qw), units, zero_rows


def exact_norm_case(rng, which, P, F, K, first, block, nblocks, qa, qw, seed=314):
    """(x [P, F], w [K, F], b [K], units): module docstring, Block-L1.  The output unit is 2^(qw - NORM_P)."""
    assert which in EXACT_KINDS and block * 7 < (1 << NORM_P)
    mx = rng.integers(seed, "mx", (P, F), -7, 8).astype(np.float64)
    if which == "zeros":
        sel = rng.integers(seed, "sel", (P, F), 0, 8)
        mx[sel == 0] = 0.0
        mx[sel == 1] = -0.0
    inside = np.zeros(F, bool)
    for k in range(nblocks):
        lo = first + k * block
        inside[lo:lo + block] = True
        l1 = np.abs(mx[:, lo:lo + block]).sum(1)
        grow = (1 << NORM_P) - l1
        last = mx[:, lo + block - 1]
        mx[:, lo + block - 1] = np.where(np.signbit(last), last - grow, last + grow)
        assert bool((np.abs(mx[:, lo:lo + block]).sum(1) == (1 << NORM_P)).all())
    zrow, zblk = P // 2, min(1, nblocks - 1)
    mx[zrow, first + zblk * block:first + (zblk + 1) * block] = 0.0                  # the all-zero block: divides by 1
    mw = rng.integers(seed, "mw", (K, F), -15, 16)
    zero_rows = [K // 2] if which == "zeros" else []
    mw[zero_rows] = 0
    mb = _exact_bias(rng, seed, K, [])
    x = np.where(inside[None, :], np.ldexp(mx, qa), np.ldexp(mx, -NORM_P))
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    # in units of 2^(qw - NORM_P): a block contributes sum m_w m_x exactly (its norm is 2^NORM_P 2^qa), the rest sum m_w m_x
    units = _units(np.abs(mx) @ np.abs(mw).astype(np.float64).T, mb)
    return x32, _to_f32(mw, qw), _to_f32(mb, qw - NORM_P), units, zero_rows


def exact_mean_case(rng, R, T, D, q, seed=315):
    """(x [R, T, D], want_mean [R, D], want_sum [R, D]): integers |m| < 2^16 (a third negative, some zero and -0.0) times 2^q."""
    assert T * 65535 < (1 << 24)
    m = rng.integers(seed, f"m{T}", (R, T, D), 0, 1 << 16).astype(np.float64)
    m = np.where(rng.integers(seed, f"s{T}", (R, T, D), 0, 3) == 0, -m, m)
    m[rng.integers(seed, f"z{T}", (R, T, D), 0, 16) == 0] = -0.0
    x = _to_f32(m, q)
    s = m.sum(1)
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s)
    mean = (s32 / np.float32(T)) * _pow2(q)                                       # the scaling by 2^q is exact
    assert np.array_equal(mean.astype(np.float64), (s32 / np.float32(T)).astype(np.float64) * 2.0 ** q)
    return x, fold_zero(mean), fold_zero(s32 * _pow2(q))
