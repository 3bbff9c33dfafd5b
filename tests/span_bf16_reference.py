"""Float64 restatement of span pooling + predicate head on bf16 segments (DESIGN.md §2 "bf16 semantics", §4c;
`tspn_span_predicate_bf16`), the input generator of its tests and their tolerance.

For a row (s, o, (start, end)) on bf16 features f [NT,T,D], classifier w [K,2D], b [K]:

    [a, e)      = oracle.span_frames(start, end, T)
    pooled_h[c] = bf16((float)(sum_{t in [a,e)} (double) f[h,t,c] / (double)(e - a)))            h in {s, o}
    out[k]      = sigmoid(sum_c pooled_s[c] w16[k,c] + sum_c pooled_o[c] w16[k,D+c] + b16[k])

w16 / b16 = the parameters rounded to bf16.  The pooled operand is part of the SEMANTICS (reproducible to the bit, see
tests/test_span_bf16_host.py); what the GPU may differ by is the fp32 accumulation of the GEMM and the fp32 sigmoid.

Tolerance of an output, `tolerance(S, D)` = 0.25 c eps S + 4 eps, eps = 2^-24, S = the span mean of sum_c |f||w16| over
both halves (non-finite |f| counted as 0), c = min(2D/32 + 33, 2D + 2):
  * span_gemm_bf16_kernel adds a product into its output along ONE chain: v_mfma_f32_16x16x32_bf16 sums the 32 products
    of a k-step and the accumulator (at most 32 roundings on the way of any one product: 31 adds among the products, one
    onto the accumulator), the 2D/32 - 1 later k-steps round the accumulator once each, the epilogue adds b16 once:
    2D/32 + 32 roundings, each at most eps of the partial sum <= eps S to first order.  One more unit covers the 2^-8 by
    which |pooled| can exceed the span mean of |f| that S is made of (c <= 256 for every shape used here);
  * 2D + 2 is the bound for ANY order of the 2D + 1 terms, so c never exceeds it (D = 16: 34 either way);
  * the sigmoid has slope <= 1/4; evaluated in fp32 (expf, an add, a division, the final rounding) it adds at most 4 eps
    to a value in (0, 1)."""
import numpy as np
import torch

import oracle
from test_gpu_span_predicate import dot_rows, draw_spans, rule_rows   # noqa: F401  (re-exported for the tests)

EPS = 2.0 ** -24


def bf16(x):
    """Round to nearest even to bf16 (torch's cast), as float32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def chain_constant(D):
    return min(2 * D // 32 + 33, 2 * D + 2)


def tolerance(S, D):
    return 0.25 * chain_constant(D) * EPS * S + 4 * EPS


def make_operands(seed, NT, T, D, K):
    """(rs, f, w, b): features uniform(-1, 1) rounded to bf16 with magnitudes below 2^-12 set to 0, weights
    0.05 N(0,1) rounded to bf16, bias 0.1 N(0,1) in fp32 (the kernel and the restatement round it)."""
    rs = np.random.RandomState(seed)
    f = bf16(rs.uniform(-1.0, 1.0, size=(NT, T, D)).astype(np.float32))
    f[np.abs(f) < 2.0 ** -12] = 0.0
    w = bf16((0.05 * rs.standard_normal((K, 2 * D))).astype(np.float32))
    b = (0.1 * rs.standard_normal(K)).astype(np.float32)
    return rs, f, w, b


def spans_for(rs, P, T):
    """draw_spans where the table is long enough for it, else the first P rule rows (rotated by the table length)."""
    rules = rule_rows(T)
    if P >= len(rules) + 8:
        return draw_spans(rs, P, T)
    return np.array([rules[(i + P) % len(rules)] for i in range(P)], dtype=np.int64).reshape(-1, 2)


def span_frames_of(spans, T):
    return np.array([oracle.span_frames(a, e, T) for a, e in spans], dtype=np.int64).reshape(-1, 2)


def pooled_rows(f, pairs, spans):
    """The pooled operand [P, 2D] as float32 holding bf16 values: float64 sum, one float64 division, rounded to fp32,
    then to bf16."""
    NT, T, D = f.shape
    frames = span_frames_of(spans, T)
    out = np.empty((len(pairs), 2 * D), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(len(pairs)):
            a, e = frames[p]
            for h in (0, 1):
                x = f[pairs[p, h], a:e].astype(np.float64)
                out[p, h * D:(h + 1) * D] = (x.sum(axis=0) / np.float64(e - a)).astype(np.float32)
    return bf16(out)


def span_predicate_ref(f, pairs, spans, w, b):
    """(ref [P,K], z [P,K] = the value before the sigmoid, S [P,K], frames [P,2]) in float64, as `span_predicate_ref` of
    tests/test_gpu_span_predicate.py returns them."""
    NT, T, D = f.shape
    pairs = np.asarray(pairs)
    w16 = bf16(w).astype(np.float64)
    frames = span_frames_of(spans, T)
    pooled = pooled_rows(f, pairs, spans).astype(np.float64)
    P, K = len(pairs), w16.shape[0]
    z, S = np.zeros((P, K)), np.zeros((P, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for h in (0, 1):
            ma = np.empty((P, D))
            for p in range(P):
                a, e = frames[p]
                x = f[pairs[p, h], a:e].astype(np.float64)
                ma[p] = np.where(np.isfinite(x), np.abs(x), 0.0).sum(axis=0) / (e - a)
            wh = w16[:, h * D:(h + 1) * D]
            z += dot_rows(pooled[:, h * D:(h + 1) * D], wh)
            S += dot_rows(ma, np.abs(wh))
        if b is not None:
            z = z + bf16(b).astype(np.float64)[None]
        ref = 1.0 / (1.0 + np.exp(-z))
    return ref, z, S, frames


def check_against_ref(got, ref, z, S, D, what, extra=0.0):
    """`check_against_ref` of tests/test_gpu_span_predicate.py with the tolerance of this module (+ `extra`): NaN exactly
    where the restatement is NaN, 1 / 0 where it is +Inf / -Inf before the sigmoid.  Returns the largest error in units
    of the tolerance."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(z)), \
        f"{what}: NaN positions differ at {np.argwhere(np.isnan(got) != np.isnan(z))[:5].tolist()}"
    assert (got[np.isposinf(z)] == 1.0).all() and (got[np.isneginf(z)] == 0.0).all(), f"{what}: +-Inf logits"
    fin = np.isfinite(z)
    tol = tolerance(S, D) + extra
    ratio = np.abs(got - ref)[fin] / tol[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: max |got - ref| = {float(np.abs(got - ref)[fin].max()) if ratio.size else 0.0:.3g}, "
          f"{worst:.3f} of the tolerance (c = {chain_constant(D)}, S up to {float(S.max()):.3g})")
    assert worst <= 1.0, f"{what}: error {worst:.3f} x the tolerance 0.25 * {chain_constant(D)} eps S + 4 eps"
    return worst
