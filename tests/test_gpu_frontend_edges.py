"""The small kernels in front of the MFMA ones, past one block and at their limits: RoIAlign and the max pools
(csrc/tspn_roi.hip, csrc/tspn_stem_bf16.hip), the pair builder (csrc/tspn_pairs.hip) and the block-L1 normalisation
(csrc/tspn_preprocess.hip), each against a plain CPU reference.

Shapes are the smallest that reach a path: a second (ragged) trip of RoIAlign's thread loop, a second workgroup and
a second wave of the geometry kernel, a second and third slab of the pair builder's grids, a last workgroup of the
block-L1 kernel with idle waves, a row stride that is not the row length.  Outputs that a caller can hold are
pre-filled with a sentinel inside a guard band: every element is written, nothing outside is.  Tolerances: the
suite's for these kernels (2e-6 for RoIAlign and the geometry, 3e-6 relative for block-L1), bit equality for data
movement, pooling and wherever the arithmetic is exact; the float64 bound of RoIAlign is derived from the float32
oracle's own deviation (profiles/r15/README.md)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import roi_head_oracle as ro
from sentinel_buffers import (GUARD, SENTINEL, assert_untouched, assert_written_inside_only, held, p, refused,
                              sentinel_of)

pytestmark = pytest.mark.gpu


def t(x):
    return torch.from_numpy(np.array(x))        # a copy: the shared maps and references are read-only


# ================================================================================================== RoIAlign
ROI_NF, ROI_H, ROI_W = 3, 9, 12
ROI_SCALE = 1.0 / 16
ROI_SETTINGS = [(0, True), (2, True), (0, False), (3, False)]       # (sampling_ratio, aligned) of test_roi_align_nhwc_vs_oracle
ROI_PC = [(7, 160), (14, 80)]                                       # OP * C / 4 = 280 items: two trips of 256 threads, the second ragged
ROIS = np.array([[0, 10, 20, 100, 120], [1, 0, 0, 191, 143], [2, -30, -10, 60, 50], [0, 150, 100, 260, 200],
                 [1, 40.5, 33.25, 41.0, 34.0], [2, 5, 5, 180, 20], [1, 300, 300, 400, 400]], dtype=np.float32)
ROI_ATOL = 2e-6
# Largest |float32 oracle - float64 oracle| over the 8 cases ROI_PC x ROI_SETTINGS on the fp32 map below, measured
# on the CPU (1.1054e-6 at P = 14, C = 80, sampling_ratio 2, aligned; profiles/r15/README.md), rounded up in the fourth
# digit.  A sample coordinate near 12 carries an fp32 rounding of 1e-6, and neighbouring pixels differ by up to 2.  The
# kernel gets four times that: it follows the float32 oracle's steps and may differ from it only in the order of the
# sum over (iy, ix).
ROI_F32_ORACLE_DEV = 1.106e-6
ROI_F64_BOUND = 4 * ROI_F32_ORACLE_DEV
ROI_BF16_CAP = 0.01        # share of bf16 outputs that may differ from oracle(float32).to(bfloat16) (rounding boundaries)


@functools.lru_cache(maxsize=None)
def roi_map(C, bf16_exact):
    import tspn_mi355x as tspn
    f = tspn.hashrng.uniform(1501, "roi-map", (ROI_NF, ROI_H, ROI_W, C), -1, 1)
    if bf16_exact:
        f = t(f).to(torch.bfloat16).float().numpy()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def roi_ref(P, C, sampling_ratio, aligned, bf16_exact, f64):
    """The oracle on the shared map, computed once per case and left unchanged."""
    out = ro.roi_align_nhwc(roi_map(C, bf16_exact), ROIS, P, ROI_SCALE, sampling_ratio, aligned,
                            dtype=np.float64 if f64 else np.float32).numpy()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("sampling_ratio,aligned", ROI_SETTINGS)
@pytest.mark.parametrize("P,C", ROI_PC)
def test_roi_align_thread_loop_second_trip_vs_float32_and_float64_oracle(tspn, device, P, C, sampling_ratio, aligned):
    """OP * C / 4 = 280 items for 256 threads: items 256 .. 279 exist only if the loop strides.  fp32 kernel against
    the float32 oracle (the suite's 2e-6) and against the float64 oracle within four times the float32 oracle's own
    deviation from it."""
    assert P * (C // 4) == 280
    ref32 = roi_ref(P, C, sampling_ratio, aligned, False, False)
    ref64 = roi_ref(P, C, sampling_ratio, aligned, False, True)
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max())
    print(f"float32 oracle - float64 oracle: {dev:.3e}")
    assert dev <= ROI_F32_ORACLE_DEV, dev       # the recorded measurement still holds for this map
    got = tspn.ops.roi_align_nhwc(t(roi_map(C, False)).to(device), t(ROIS).to(device), P, ROI_SCALE, sampling_ratio,
                                  aligned).cpu().numpy()
    assert got.shape == (len(ROIS), P, P, C)
    e32 = float(np.abs(got - ref32).max())
    e64 = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"kernel - float32 oracle: {e32:.3e}; kernel - float64 oracle: {e64:.3e} (bound {ROI_F64_BOUND:.3e})")
    np.testing.assert_allclose(got, ref32, rtol=0, atol=ROI_ATOL)
    assert e64 <= ROI_F64_BOUND, e64


@pytest.mark.parametrize("sampling_ratio,aligned", ROI_SETTINGS)
@pytest.mark.parametrize("P,C", ROI_PC)
def test_roi_align_three_instantiations_on_a_bf16_exact_map(tspn, device, P, C, sampling_ratio, aligned):
    """<true, true> (bf16 map) and <false, true> (the same values as fp32, bf16 out) are bit-identical, and equal
    oracle(float32) rounded to bf16 except where the fp32 value lies within the fp32 tolerance of a bf16 rounding
    boundary; such exceptions stay under 1 % of the elements.  <false, false> on the same map: the fp32 tolerance."""
    fm = roi_map(C, True)
    ref32 = t(roi_ref(P, C, sampling_ratio, aligned, True, False))
    ref64 = t(roi_ref(P, C, sampling_ratio, aligned, True, True))
    want = ref32.to(torch.bfloat16)
    own = float((want != ref64.float().to(torch.bfloat16)).float().mean())
    print(f"float32 oracle against float64 oracle, both rounded to bf16: {own:.3%} differ")
    assert own <= ROI_BF16_CAP, own             # the seed leaves room under the cap
    rois = t(ROIS).to(device)
    a = tspn.ops.roi_align_nhwc(t(fm).to(torch.bfloat16).to(device), rois, P, ROI_SCALE, sampling_ratio, aligned)
    b = tspn.ops.roi_align_nhwc(t(fm).to(device), rois, P, ROI_SCALE, sampling_ratio, aligned, out_bf16=True)
    c = tspn.ops.roi_align_nhwc(t(fm).to(device), rois, P, ROI_SCALE, sampling_ratio, aligned)
    assert a.dtype == b.dtype == torch.bfloat16 and c.dtype == torch.float32
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    np.testing.assert_allclose(c.cpu().numpy(), ref32.numpy(), rtol=0, atol=ROI_ATOL)
    assert torch.equal(c.to(torch.bfloat16).view(torch.int16), b.view(torch.int16))     # one rounding of the fp32 result
    a = a.cpu()
    lo, hi = (ref32 - ROI_ATOL).to(torch.bfloat16), (ref32 + ROI_ATOL).to(torch.bfloat16)
    assert bool(((a == want) | (a == lo) | (a == hi)).all()), "a bf16 output differs away from a rounding boundary"
    share = float((a != want).float().mean())
    print(f"bf16 outputs that differ from oracle(float32).to(bfloat16): {share:.3%}")
    assert share <= ROI_BF16_CAP, share


def _limit_positions(n):
    """(sample position, row it reads or None when the sample is empty) along an axis of n pixels."""
    f = np.float32
    return [(f(-1.0), 0), (np.nextafter(f(-1.0), f(-np.inf)), None), (f(0.0), 0), (f(n - 1), n - 1), (f(n), n - 1),
            (np.nextafter(f(n), f(np.inf)), None)]


@pytest.mark.parametrize("H,W", [(5, 6), (1, 6), (5, 1)])
def test_roi_align_single_sample_on_the_limits_of_bilinear_setup(tspn, device, H, W):
    """aligned = False, scale 1, one sample, one bin: the sample sits at y1 + 0.5 * max(y2 - y1, 1), exact in fp32.
    It is placed at -1 (taken, row 0), just below -1 (empty -> 0), 0, H - 1, H (taken, row H - 1) and just above H
    (empty), in y with x on a pixel and in x with y on a pixel; every weight is then 0 or 1, so the output equals
    the float32 oracle bit for bit and is the map's own pixel (or zero)."""
    f, C = np.float32, 8
    fm = tspn.hashrng.uniform(1502, f"lim{H}x{W}", (1, H, W, C), -1, 1)
    fixed_y, fixed_x = f(min(2, H - 1)), f(min(3, W - 1))
    rois, want = [], []
    for s, row in _limit_positions(H):
        rois.append([0, fixed_x - f(0.5), s - f(0.5), fixed_x + f(0.5), s + f(0.5)])
        want.append(fm[0, row, int(fixed_x)] if row is not None else np.zeros(C, f))
    for s, col in _limit_positions(W):
        rois.append([0, s - f(0.5), fixed_y - f(0.5), s + f(0.5), fixed_y + f(0.5)])
        want.append(fm[0, int(fixed_y), col] if col is not None else np.zeros(C, f))
    rois = np.array(rois, dtype=f)
    # the construction is exact: the sample of row i is where it was meant to be
    sy = rois[:, 2] + f(0.5) * np.maximum(rois[:, 4] - rois[:, 2], f(1))
    sx = rois[:, 1] + f(0.5) * np.maximum(rois[:, 3] - rois[:, 1], f(1))
    assert sy.dtype == sx.dtype == f
    np.testing.assert_array_equal(sy[:6], [s for s, _ in _limit_positions(H)])
    np.testing.assert_array_equal(sx[6:], [s for s, _ in _limit_positions(W)])
    assert (sy[6:] == fixed_y).all() and (sx[:6] == fixed_x).all()
    ref = ro.roi_align_nhwc(fm, rois, 1, 1.0, 1, False).numpy()
    np.testing.assert_array_equal(ref.reshape(12, C), np.stack(want))         # the oracle itself follows the stated rule
    got = tspn.ops.roi_align_nhwc(t(fm).to(device), t(rois).to(device), 1, 1.0, 1, False).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), ref.view(np.int32))


def roi_raw(tspn, entry, feat, rois, R, P, sampling_ratio, aligned, bs, out, C=None):
    """A tspn_roi_align_nhwc_* entry on caller-held tensors; returns the status code."""
    NF, H, W, Cf = feat.shape
    return getattr(tspn._abi.lib(), entry)(p(feat), NF, H, W, Cf if C is None else C, p(rois), R, P, ROI_SCALE,
                                           sampling_ratio, 1 if aligned else 0, bs, p(out), tspn.ops._stream())


@pytest.mark.parametrize("bs", [1, 2, 3])
def test_roi_align_writes_every_element_and_nothing_else(tspn, device, bs):
    """Through the C ABI into a sentinel-filled buffer, the view 32 elements in (16-byte aligned): bin_stride 1, 2, 3
    of P = 7 give OP = 7, 4, 3; every element of [R,OP,OP,C] is written, the guard bands keep the sentinel, and the
    result is the bins (bs i, bs j) of the full grid bit for bit -- fp32 out and bf16 out."""
    P, C = 7, 160
    OP = (P + bs - 1) // bs
    feat, rois = t(roi_map(C, False)).to(device), t(ROIS).to(device)
    full = tspn.ops.roi_align_nhwc(feat, rois, P, ROI_SCALE, 0, True)
    np.testing.assert_allclose(full.cpu().numpy(), roi_ref(P, C, 0, True, False, False), rtol=0, atol=ROI_ATOL)
    for entry, dtype in (("tspn_roi_align_nhwc_f32", torch.float32), ("tspn_roi_align_nhwc_f32_bf16out", torch.bfloat16)):
        buf, out = held((len(ROIS), OP, OP, C), device, dtype)
        assert out.data_ptr() % 16 == 0 and out.storage_offset() == GUARD
        tspn._abi.check(roi_raw(tspn, entry, feat, rois, len(ROIS), P, 0, True, bs, out))
        assert_written_inside_only(buf, out, f"{entry} bin_stride={bs}")
        assert torch.equal(out, full[:, ::bs, ::bs].to(dtype)), f"{entry} bin_stride={bs}"


def test_roi_align_refusals_leave_the_output_alone(tspn, device):
    """C % 4 != 0, a map or an output that is not 16-byte aligned, and R * P >= 2^31 (by argument only: refused before
    anything is read) return TSPN_EUNSUPPORTED and write nothing."""
    P, C = 7, 8
    UNS = tspn._abi.TSPN_EUNSUPPORTED
    feat, rois = t(roi_map(160, False)[..., :C].copy()).to(device), t(ROIS).to(device)
    buf, out = held((len(ROIS), P, P, C), device)
    refused(tspn, roi_raw(tspn, "tspn_roi_align_nhwc_f32", feat, rois, len(ROIS), P, 0, True, 1, out, C=6), UNS, "C = 6")
    bufu, outu = held((len(ROIS), P, P, C), device, offset=1)
    assert outu.data_ptr() % 16 == 4
    refused(tspn, roi_raw(tspn, "tspn_roi_align_nhwc_f32", feat, rois, len(ROIS), P, 0, True, 1, outu), UNS, "out + 4 bytes")
    _, featu = held(tuple(feat.shape), device, offset=1)
    featu.copy_(feat)
    refused(tspn, roi_raw(tspn, "tspn_roi_align_nhwc_f32", featu, rois, len(ROIS), P, 0, True, 1, out), UNS, "feat + 4 bytes")
    big_r = (1 << 31) // P + 1
    assert big_r * P >= 1 << 31 and (big_r - 1) * P < 1 << 31
    refused(tspn, roi_raw(tspn, "tspn_roi_align_nhwc_f32", feat, rois, big_r, P, 0, True, 1, out), UNS, "R * P >= 2^31")
    buf16, out16 = held((len(ROIS), P, P, C), device, torch.bfloat16)
    for entry in ("tspn_roi_align_nhwc_f32_bf16out", "tspn_roi_align_nhwc_bf16"):
        src = feat if entry.endswith("out") else feat.to(torch.bfloat16)
        refused(tspn, roi_raw(tspn, entry, src, rois, len(ROIS), P, 0, True, 1, out16, C=6), UNS, f"{entry} C = 6")
        refused(tspn, roi_raw(tspn, entry, src, rois, big_r, P, 0, True, 1, out16), UNS, f"{entry} R * P >= 2^31")
    torch.cuda.synchronize()
    for b, what in ((buf, "fp32 out"), (bufu, "unaligned out"), (buf16, "bf16 out")):
        assert_untouched(b, what)
    with pytest.raises(tspn._abi.TspnError) as e:               # the Python wrapper reports the same refusal
        tspn.ops.roi_align_nhwc(torch.zeros(1, 4, 4, 6, device=device), rois, P, ROI_SCALE)
    assert e.value.code == UNS


def test_roi_align_many_rois_each_row_bit_identical_to_its_own_launch(tspn, device):
    """R = 20000 rows (140000 workgroups) repeating 8 distinct RoIs in a shuffled order: every row equals the row of
    its RoI from an 8-row launch bit for bit -- the workgroup-to-(roi, oph) map and the 64-bit output offsets."""
    P, C, R = 7, 8, 20000
    feat = t(roi_map(160, False)[..., 16:16 + C].copy()).to(device)
    eight = np.concatenate([ROIS, np.array([[2, 17.5, 3.25, 150.0, 97.75]], dtype=np.float32)])
    which = tspn.hashrng.integers(1503, "many", (R,), 0, 8)
    assert set(which.tolist()) == set(range(8)) and not (which[:8] == np.arange(8)).all()
    small = tspn.ops.roi_align_nhwc(feat, t(eight).to(device), P, ROI_SCALE, 0, True)
    np.testing.assert_allclose(small.cpu().numpy(), ro.roi_align_nhwc(feat.cpu().numpy(), eight, P, ROI_SCALE, 0, True).numpy(),
                               rtol=0, atol=ROI_ATOL)
    big = tspn.ops.roi_align_nhwc(feat, t(eight[which]).to(device), P, ROI_SCALE, 0, True)
    assert tuple(big.shape) == (R, P, P, C)
    same = (big.view(torch.int32) == small.view(torch.int32)[t(which).to(device)]).flatten(1).all(dim=1)
    assert bool(same.all()), f"rows {torch.nonzero(~same).flatten()[:8].tolist()} differ from their RoI's own launch"


def test_roi_align_map_index_interleaved_and_clamped(tspn, device):
    """Column 0 of a RoI selects the map.  Rows naming map NF - 1 and map 0 in turn read the right one, and an index
    outside [0, NF) is clamped (-1 reads map 0, NF reads map NF - 1), as include/tspn_mi355x.h states."""
    P, C, NF = 5, 8, ROI_NF
    fm = roi_map(160, False)[..., 32:32 + C].copy()
    box = [10, 20, 100, 120]
    idx = [NF - 1, 0, NF - 1, 0, 1, -1, NF, 0, NF - 1]
    rois = np.array([[i] + box for i in idx], dtype=np.float32)
    clamped = rois.copy()
    clamped[:, 0] = np.clip(clamped[:, 0], 0, NF - 1)
    ref = ro.roi_align_nhwc(fm, clamped, P, ROI_SCALE, 0, True).numpy()
    assert np.abs(ref[0] - ref[1]).max() > 1e-2                  # the maps differ where the box lies
    got = tspn.ops.roi_align_nhwc(t(fm).to(device), t(rois).to(device), P, ROI_SCALE, 0, True).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=ROI_ATOL)
    for i, j in ((5, 1), (6, 0), (2, 0), (3, 1), (7, 1), (8, 0)):   # the same map read from another row: the same bits
        np.testing.assert_array_equal(got[i].view(np.int32), got[j].view(np.int32), err_msg=f"rows {i}, {j}")


# ================================================================================================== max pool
POOL_SHAPES = [(1, 1, 1, 8), (1, 2, 1, 8), (3, 1, 2, 8), (2, 5, 7, 72), (1, 23, 40, 64)]
POOL_KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (1, 1, 0)]


def pool_input(tspn, shape):
    """Finite or -inf only: channels [0, C/2) are negative everywhere (a window of them has a negative maximum, and a
    padding position that took part as 0 would win), a tenth of the values and (on maps of more than two pixels) one whole pixel are -inf."""
    NB, H, W, C = shape
    x = tspn.hashrng.uniform(1510, f"pool{shape}", shape, -1, 1)
    x[..., :C // 2] -= np.float32(1.5)
    x[tspn.hashrng.uniform(1510, f"inf{shape}", shape) < 0.1] = -np.inf
    if H * W > 2:
        x[NB - 1, H // 2, W // 2, :] = -np.inf
    assert not np.isnan(x).any() and (x[..., :C // 2] < 0).all()
    return x


def pool_raw(tspn, x, k, s, pad, out, out_bf16=False, C=None):
    NB, H, W, Cx = x.shape
    C = Cx if C is None else C
    l = tspn._abi.lib()
    if x.dtype == torch.bfloat16:
        return l.tspn_max_pool_nhwc_bf16(p(x), NB, H, W, C, k, s, pad, p(out), tspn.ops._stream())
    return l.tspn_max_pool_nhwc_f32(p(x), NB, H, W, C, k, s, pad, p(out), 1 if out_bf16 else 0, tspn.ops._stream())


@pytest.mark.parametrize("k,s,pad", POOL_KSP)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_max_pool_all_three_forms_bit_for_bit_vs_torch(tspn, device, shape, k, s, pad):
    """fp32 -> fp32, fp32 -> bf16 and bf16 -> bf16 against torch.nn.functional.max_pool2d on the CPU: maps of one
    and two pixels (windows clipped on both sides), C = 72 and 64 (a thread's channel group matters), -inf and
    negative-only windows; outputs held in sentinel-filled buffers.  A window larger than the padded map has no
    output: refused by the wrapper and by the C entry, nothing written."""
    NB, H, W, C = shape
    x = pool_input(tspn, shape)
    xd = t(x).to(device)
    x16 = t(x).to(torch.bfloat16)
    forms = ((xd, False, torch.float32), (xd, True, torch.bfloat16), (x16.to(device), False, torch.bfloat16))
    if H + 2 * pad < k or W + 2 * pad < k:
        with pytest.raises(RuntimeError):
            torch.nn.functional.max_pool2d(t(x).permute(0, 3, 1, 2), k, s, pad)
        with pytest.raises(ValueError):
            tspn.ops.max_pool_nhwc(xd, k, s, pad)
        with pytest.raises(ValueError):
            tspn.ops.max_pool_nhwc_bf16(x16.to(device), k, s, pad)
        for src, out_bf16, dtype in forms:
            buf, out = held((NB, 1, 1, C), device, dtype)
            refused(tspn, pool_raw(tspn, src, k, s, pad, out, out_bf16), tspn._abi.TSPN_EINVAL, f"empty output {dtype}")
            torch.cuda.synchronize()
            assert_untouched(buf, f"empty output {dtype}")
        return
    ref = torch.nn.functional.max_pool2d(t(x).permute(0, 3, 1, 2), k, s, pad).permute(0, 2, 3, 1).contiguous()
    ref16 = torch.nn.functional.max_pool2d(x16.float().permute(0, 3, 1, 2), k, s, pad).permute(0, 2, 3, 1).contiguous()
    assert bool((ref[..., :C // 2] < 0).all())
    wants = (ref, ref.to(torch.bfloat16), ref16.to(torch.bfloat16))
    for (src, out_bf16, dtype), want in zip(forms, wants):
        what = f"{src.dtype} -> {dtype}"
        buf, out = held(tuple(want.shape), device, dtype)
        tspn._abi.check(pool_raw(tspn, src, k, s, pad, out, out_bf16))
        assert_written_inside_only(buf, out, what)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(out.cpu().view(bits), want.view(bits)), what
    # the wrappers size their output as torch does
    assert torch.equal(tspn.ops.max_pool_nhwc(xd, k, s, pad).cpu(), ref)
    assert torch.equal(tspn.ops.max_pool_nhwc(xd, k, s, pad, out_bf16=True).cpu(), wants[1])
    assert torch.equal(tspn.ops.max_pool_nhwc_bf16(x16.to(device), k, s, pad).cpu(), wants[2])


def test_max_pool_refuses_channel_counts_it_cannot_vectorise(tspn, device):
    """C % 4 != 0 (fp32 map) and C % 8 != 0 (bf16 map): TSPN_EUNSUPPORTED, nothing written."""
    UNS = tspn._abi.TSPN_EUNSUPPORTED
    x = torch.zeros(1, 4, 4, 12, device=device)
    buf, out = held((1, 2, 2, 12), device)
    buf16, out16 = held((1, 2, 2, 12), device, torch.bfloat16)
    refused(tspn, pool_raw(tspn, x, 3, 2, 1, out, C=6), UNS, "fp32 C = 6")
    refused(tspn, pool_raw(tspn, x, 3, 2, 1, out16, out_bf16=True, C=6), UNS, "fp32 -> bf16 C = 6")
    refused(tspn, pool_raw(tspn, x.to(torch.bfloat16), 3, 2, 1, out16), UNS, "bf16 C = 12")
    tspn._abi.check(pool_raw(tspn, x, 3, 2, 1, out))              # C = 12 is fine for the fp32 map
    torch.cuda.synchronize()
    assert_written_inside_only(buf, out, "fp32 C = 12")
    assert_untouched(buf16, "bf16 out")
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn.ops.max_pool_nhwc_bf16(x.to(torch.bfloat16), 3, 2, 1)
    assert e.value.code == UNS


# ================================================================================================== pair builder
GEOM_TOL = dict(rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("T", [256, 257, 513, 900])
def test_pair_gather_long_tracklets_second_workgroup_and_wave_edges(tspn, device, T):
    """T beyond one workgroup of 256 frames: lane 0 of every wave (t = 64, 128, ...) and of every further workgroup
    (t = 256, 512) takes the previous frame from memory, every other lane from its neighbour.  All eight geometry
    channels against the oracle, the two motion channels again frame by frame at the edges; features bit-exact."""
    N, D = 3, 4
    v = tspn.synth.make_video(1520, N, T, D)
    pairs = oracle.pair_index(N)
    ref_f, ref_g = oracle.pair_gather(t(v["tracklet_feats"]), t(v["tracklet_boxes"]), pairs)
    f, g = tspn.ops.pair_gather(t(v["tracklet_feats"]).to(device), t(v["tracklet_boxes"]).to(device), pairs.to(device))
    g = g.cpu().numpy()
    assert g.shape == (N * (N - 1), 8, T)
    for tt in (0, 63, 64, 255, 256, 257, 512):
        if tt < T:
            for ch in (5, 6):
                np.testing.assert_allclose(g[:, ch, tt], ref_g[:, ch, tt].numpy(), err_msg=f"channel {ch}, frame {tt}", **GEOM_TOL)
    assert float(ref_g[:, 5:7, 1:].abs().min()) > 1e-4           # a motion channel left at zero would show
    np.testing.assert_allclose(g, ref_g.numpy(), **GEOM_TOL)
    np.testing.assert_array_equal(f.cpu().numpy(), ref_f.numpy())


def slab_table(tspn, P, tag):
    """A pair table of P rows over N = 4 tracklets: rows 0 .. 11 are the 12 ordered pairs, every later row repeats
    one of them.  Returns (pairs int64 [P,2], code int64 [P]) with pairs[i] == pairs[code[i]], code[i] < 12."""
    first = oracle.pair_index(4)
    code = np.concatenate([np.arange(12), tspn.hashrng.integers(1521, tag, (P - 12,), 0, 12)])
    return first[t(code)].contiguous(), t(code)


def check_slabs(got, code, edges, ref_rows, what, tol=None):
    """`got` [P, ...] on the device: the rows `edges` against the oracle's rows, every row against the launch's own row
    of the same pair among the first 12, bit for bit."""
    e = got[t(np.array(edges)).to(got.device)].cpu().numpy()
    if tol is None:
        np.testing.assert_array_equal(e, ref_rows.numpy(), err_msg=what)
    else:
        np.testing.assert_allclose(e, ref_rows.numpy(), err_msg=what, **tol)
    bits = got.view(torch.int32).flatten(1)
    same = (bits == bits[:12][code.to(got.device)]).all(dim=1)
    assert bool(same.all()), f"{what}: rows {torch.nonzero(~same).flatten()[:8].tolist()} differ from their pair's first row"


def test_pair_geometry_walks_its_slabs_of_65535_pairs(tspn, device):
    """65535 + 65535 + 3 rows: three launches of pair_geometry_kernel.  The rows on both sides of every slab edge
    against the oracle, all others against the first occurrence of their pair."""
    N, T = 4, 3
    P = 65535 + 65535 + 3
    v = tspn.synth.make_video(1522, N, T, 1)
    boxes = t(v["tracklet_boxes"])
    pairs, code = slab_table(tspn, P, "geom")
    edges = [0, 65534, 65535, 65536, 131069, 131070, 131072]
    assert len({int(c) for c in code[edges]}) >= 4                 # the edge rows name several different pairs
    _, g = tspn.ops.pair_gather(None, boxes.to(device), pairs.to(device), want_feat=False)
    assert tuple(g.shape) == (P, 8, T)
    check_slabs(g, code, edges, oracle.pair_geometry(boxes, pairs[edges]), "geometry", GEOM_TOL)


@pytest.mark.parametrize("D,T,form", [(5, 3, "32x32"), (64, 2, "rows")])
def test_pair_features_beyond_65535_rows_in_both_forms(tspn, device, D, T, form):
    """32767 + 32767 + 2 pairs.  D = 5 forces the 32 x 32 transpose, which walks blockIdx.z in slabs of 65534 rows =
    32767 pairs (three launches); D = 64 takes the whole-tracklet form, one launch of 2 P workgroups.  The pairs on
    both sides of every slab edge against the oracle, every row against the first occurrence of its pair."""
    N = 4
    P = 32767 + 32767 + 2
    rows_form = D % 64 == 0 and T <= 160
    assert rows_form == (form == "rows") and P > 65535
    v = tspn.synth.make_video(1523, N, T, D)
    feats = t(v["tracklet_feats"])
    pairs, code = slab_table(tspn, P, form)
    edges = [0, 32766, 32767, 65533, 65534, 65535]
    assert len({int(c) for c in code[edges]}) >= 4
    f, _ = tspn.ops.pair_gather(feats.to(device), None, pairs.to(device), want_geom=False)
    assert tuple(f.shape) == (P, 2 * D, T)
    ref, _ = oracle.pair_gather(feats, t(v["tracklet_boxes"]), pairs[edges])
    check_slabs(f, code, edges, ref, f"features ({form} form)")


def test_transpose_td_refuses_65536_rows(tspn, device):
    """tspn_transpose_td_f32 puts R into blockIdx.z and does not walk slabs: R = 65535 works, R = 65536 is refused."""
    x = t(tspn.hashrng.uniform(1524, "x", (65535, 2, 3), -1, 1)).to(device)
    assert torch.equal(tspn.ops.transpose_td(x), x.transpose(1, 2).contiguous())
    buf, out = held((65536, 1, 1), device)
    rc = tspn._abi.lib().tspn_transpose_td_f32(p(torch.zeros(65536, 1, 1, device=device)), 65536, 1, 1, p(out), tspn.ops._stream())
    refused(tspn, rc, tspn._abi.TSPN_EUNSUPPORTED, "R = 65536")
    torch.cuda.synchronize()
    assert_untouched(buf, "R = 65536")


# ================================================================================================== block-L1
L1_CASES = [(3, 40, 4, 6, 3),      # 9 items: three workgroups of 4 waves, the last with three idle waves
            (1, 1, 0, 1, 1),
            (5, 130, 0, 65, 2),    # a block one element wider than a wave
            (2, 64, 0, 64, 1),
            (7, 200, 9, 63, 3)]    # blocks narrower than a wave; the last block ends at column 198 < F
L1_TOL = dict(rtol=3e-6, atol=1e-9)


def l1_input(tspn, P, F, first, block, nblocks):
    x = tspn.hashrng.uniform(1530, f"l1-{P}-{F}", (P, F), -1, 1)
    if P > 1:
        x[1, first:first + block] = 0            # a zero block stays zero (norm := 1)
    return x


def l1_ref(x, first, block, nblocks):
    """float64: x / sum|x| per block, a zero block unchanged; columns outside the blocks as they are."""
    ref = x.astype(np.float64)
    for k in range(nblocks):
        sl = slice(first + k * block, first + (k + 1) * block)
        n = np.abs(ref[:, sl]).sum(axis=1, keepdims=True)
        ref[:, sl] = ref[:, sl] / np.where(n == 0, 1.0, n)
    return ref


def inside_blocks(F, first, block, nblocks):
    m = np.zeros(F, dtype=bool)
    m[first:first + block * nblocks] = True
    return m


@pytest.mark.parametrize("P,F,first,block,nblocks", L1_CASES)
def test_block_l1_small_and_ragged_blocks_vs_float64(tspn, device, P, F, first, block, nblocks):
    x = l1_input(tspn, P, F, first, block, nblocks)
    ref = l1_ref(x, first, block, nblocks)
    np.testing.assert_allclose(oracle.feature_preprocess(t(x).double(), first, block, nblocks).numpy(), ref, rtol=1e-15, atol=0)
    got = tspn.ops.feature_preprocess_(t(x).to(device), first, block, nblocks).cpu().numpy()
    m = inside_blocks(F, first, block, nblocks)
    np.testing.assert_allclose(got[:, m], ref[:, m], **L1_TOL)
    np.testing.assert_array_equal(got[:, ~m].view(np.int32), x[:, ~m].view(np.int32))    # outside the blocks: untouched
    if P > 1:
        assert (got[1, first:first + block] == 0).all()


@pytest.mark.parametrize("P,F,first,block,nblocks", L1_CASES)
def test_block_l1_row_stride_longer_than_the_row(tspn, device, P, F, first, block, nblocks):
    """ld = F + 3 through the C ABI (ops.feature_preprocess_ always passes ld == F): rows are found at the stride and
    the three pad columns of every row, like the guard bands, keep their sentinel."""
    ld = F + 3
    x = l1_input(tspn, P, F, first, block, nblocks)
    ref = l1_ref(x, first, block, nblocks)
    buf, rows = held((P, ld), device)
    rows[:, :F] = t(x).to(device)
    tspn._abi.check(tspn._abi.lib().tspn_feature_preprocess_f32(p(rows), P, F, ld, first, block, nblocks, tspn.ops._stream()))
    got = rows.cpu().numpy()
    m = inside_blocks(F, first, block, nblocks)
    np.testing.assert_allclose(got[:, :F][:, m], ref[:, m], **L1_TOL)
    np.testing.assert_array_equal(got[:, :F][:, ~m].view(np.int32), x[:, ~m].view(np.int32))
    assert (got[:, F:] == np.float32(SENTINEL)).all(), "a pad column was written"
    b, s = buf.cpu(), sentinel_of(buf)
    assert bool((b[:GUARD] == s).all()) and bool((b[GUARD + P * ld:] == s).all()), "wrote outside the rows"


def test_block_l1_refusals(tspn, device):
    """ld < F and blocks that run past F: TSPN_EINVAL, the rows untouched."""
    P, F = 3, 40
    x = t(tspn.hashrng.uniform(1531, "x", (P, F), -1, 1)).to(device)
    keep = x.clone()
    fn = tspn._abi.lib().tspn_feature_preprocess_f32
    refused(tspn, fn(p(x), P, F, F - 1, 4, 6, 3, tspn.ops._stream()), tspn._abi.TSPN_EINVAL, "ld < F")
    refused(tspn, fn(p(x), P, F, F, 4, 6, 7, tspn.ops._stream()), tspn._abi.TSPN_EINVAL, "4 + 6 * 7 > 40")
    refused(tspn, fn(p(x), P, F, F + 3, 35, 6, 1, tspn.ops._stream()), tspn._abi.TSPN_EINVAL, "35 + 6 > 40 although < ld")
    assert fn(p(x), P, F, F, 4, 6, 6, tspn.ops._stream()) == 0 and not torch.equal(x, keep)   # 4 + 36 == F is allowed
    x.copy_(keep)
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn.ops.feature_preprocess_(x, 4, 6, 7)
    assert e.value.code == tspn._abi.TSPN_EINVAL
    assert torch.equal(x, keep)
