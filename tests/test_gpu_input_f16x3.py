"""The fused input side of the split-fp16 F(6,3) conv (csrc/inputf16/tspn_input_f16x3.hip: column maxima and temporal mean
in one read of the features, the split in a second) against the two-pass transform and the mean kernel it replaces: the same bytes everywhere -- split input, column exponents (padding columns included),
temporal mean, hot-sextet key, y of the stand-alone conv, heads / logits / guard reading of the fused pass.

ops.wino63_f16x3_set_input_form: 0 = by shape (default), 1 = two-pass everywhere, 2 = fused wherever supported.
Shapes: D 64 / 128 / 2048 (scan blocks of one partly filled wave, one half-filled wave, the full 512 threads), T = 2 (less than a
sextet), 6, 8 (a second sextet with two own frames), 150 (25 sextets), 200 (34: a second chunk of the scan), NT = 1 / 3 / 33
(sextet counts that do not fill a group, padding columns up to the 256-sextet tile)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 256     # output rows of the conv the workspace is laid out for (the smallest the split form takes)


@contextlib.contextmanager
def input_form(tspn, form):
    prev = tspn.ops.wino63_f16x3_set_input_form(form)
    try:
        yield
    finally:
        tspn.ops.wino63_f16x3_set_input_form(prev)


def features(tspn, seed, NT, T, D, device):
    return torch.from_numpy(tspn.hashrng.uniform(seed, "x", (NT, T, D), -1, 1)).to(device).contiguous()


def input_side(tspn, x, form):
    """(v, e, fbar, key) of the input side under `form`, from a workspace whose every byte was 0x5a before."""
    B, T, Cin = x.shape
    need = tspn._abi.lib().tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=x.device)
    with input_form(tspn, form):
        v, e, fbar, key = tspn.ops.wino63_f16x3_input(x, M, workspace=ws)
    torch.cuda.synchronize(x.device)
    return v.clone(), e.clone(), fbar, int(key)


def assert_same_input_side(tspn, x):
    two, one = input_side(tspn, x, 1), input_side(tspn, x, 2)   # two-pass + mean kernel, fused
    for name, a, b in zip(("split input", "column exponents", "temporal mean"), two[:3], one[:3]):
        # bytes, not values: NaN == NaN, -0 != +0
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name
    assert two[3] == one[3], f"hot-sextet key {two[3]:#x} != {one[3]:#x}"
    mean = tspn.ops.temporal_mean(x, True)
    assert torch.equal(one[2].view(torch.int32), mean.view(torch.int32))
    return one


SHAPES = [(1, 2, 64), (3, 6, 128), (33, 8, 64), (3, 150, 128), (1, 150, 2048), (33, 8, 2048), (3, 13, 2048), (2, 200, 320)]


@pytest.mark.parametrize("NT,T,D", SHAPES)
def test_fused_input_side_equals_the_two_pass_bytes(tspn, device, NT, T, D):
    x = features(tspn, 11 + NT + T, NT, T, D, device)
    v, e, fbar, key = assert_same_input_side(tspn, x)
    nq = -(-T // 6)
    assert v.shape[3] % 256 == 0 and v.shape[3] >= NT * nq
    # padding sextets: zeros, exponent 0 (the contraction multiplies them)
    assert bool((v[:, :, :, NT * nq:] == 0).all()) and bool((e[:, NT * nq:] == 0).all())
    # the key names the largest |x| and a sextet that holds it
    big = float(x.abs().max())
    assert np.array([key >> 32], dtype=np.uint32).view(np.float32)[0] == np.float32(big)
    trk, frame = [int(i[0]) for i in torch.nonzero(x.abs().amax(dim=2) == big, as_tuple=True)]
    assert key & 0xFFFFFFFF >= trk * nq + frame // 6


def test_value_cases_zero_column_nan_inf(tspn, device):
    NT, T, D = 3, 20, 128
    x = features(tspn, 5, NT, T, D, device)
    x[1, 5:14] = 0.0                      # sextet 1 of tracklet 1 (frames 5 .. 12) is all zeros: exponent 0, zero halves
    x[0, 3, 17] = float("nan")
    x[2, 8, 64] = float("inf")
    v, e, fbar, key = assert_same_input_side(tspn, x)
    nq = -(-T // 6)
    assert bool((e[:, 1 * nq + 1] == 0).all()) and bool((v[:, :, :, 1 * nq + 1] == 0).all())
    assert bool((e[:7, 0] == 0).all())    # a NaN column is not scaled (frame 3 is d4: in every point but the last)
    assert key & 0xFFFFFFFF == 0 and (key >> 32) == 0x7FC00000          # NaN ranks above Inf
    assert bool(torch.isnan(fbar[0, 17])) and bool(torch.isinf(fbar[2, 64]))


@pytest.mark.parametrize("frame,sextet", [(11, 1), (6, 1), (5, 0), (12, 2)])
def test_hot_value_counts_in_its_own_sextet_only(tspn, device, frame, sextet):
    """Frames 6 .. 11 are sextet 1's own; 5 and 12 are its overlap frames and belong to sextets 0 and 2."""
    NT, T, D = 2, 20, 64
    x = features(tspn, 9, NT, T, D, device)
    x[1, frame, 33] = -41.25
    _, _, _, key = assert_same_input_side(tspn, x)
    assert key & 0xFFFFFFFF == 1 * 4 + sextet
    assert np.array([key >> 32], dtype=np.uint32).view(np.float32)[0] == np.float32(41.25)


def test_shapes_outside_the_kernels_fall_back(tspn, device):
    """D above the register-resident limit under form 2, and few tracklets under the default: the two-pass kernels run
    (same bytes as under form 1), and the selection function says so for the device's CU count."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert tspn.ops.wino63_f16x3_input_form(3, 8, 2048, cus) == 0
    assert tspn.ops.wino63_f16x3_input_form(512, 150, 2048, cus) == 1
    x = features(tspn, 3, 2, 8, 2080, device)          # 2080 % 32 == 0, > 2048
    assert_same_input_side(tspn, x)
    x = features(tspn, 4, 3, 8, 2048, device)
    ref, got = input_side(tspn, x, 1), input_side(tspn, x, 0)
    for a, b in zip(ref[:3], got[:3]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert ref[3] == got[3]


@pytest.mark.parametrize("NT,T,D", [(3, 8, 64), (1, 150, 128), (33, 8, 2048), (2, 13, 2048)])
def test_conv_entry_y_is_the_same_under_both_forms(tspn, device, NT, T, D):
    x = features(tspn, 21, NT, T, D, device)
    w = torch.from_numpy(tspn.hashrng.uniform(22, "w", (M, D, 3), -0.05, 0.05)).to(device).contiguous()
    bias = torch.from_numpy(tspn.hashrng.uniform(23, "b", (M,), -1, 1)).to(device).contiguous()
    packed = tspn.ops.pack_conv3_wino63_f16x3(w)
    ys = []
    for form in (1, 2):
        with input_form(tspn, form):
            ys.append(tspn.ops.conv3_tc_wino63_f16x3(x, packed, bias=bias))
    torch.cuda.synchronize(device)
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))
    ref = torch.nn.functional.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), padding=1)
    assert float((ys[1].double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("T", [40, 6])
def test_fused_pass_and_guard_reading_are_the_same_under_both_forms(tspn, device, T):
    """Heads, logits, the hot-sextet slots and the measured error of tspn_forward_fused_f32.  The spot check draws three of
    its four sextets anew per call; with every row checked (conv_check = 4 D) and an outlier of 1000x in the hot sextet,
    which it always covers, the largest deviation is the hot sextet's and does not depend on the draw."""
    B, N, D = 2, 3, 64
    sd = tspn.synth.make_weights(50, c=2 * D, bias_std=0.05)
    pre = "relpn.duration_proposal_network.dpn_head."
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).contiguous()   # noqa: E731
    conv_w, conv_b = d(sd[pre + "conv.weight"]), d(sd[pre + "conv.bias"])
    hw = d(np.concatenate([sd[pre + "relness_pred.weight"][:, :, 0], sd[pre + "duration_pred.weight"][:, :, 0]]))
    hb = d(np.concatenate([sd[pre + "relness_pred.bias"], sd[pre + "duration_pred.bias"]]))
    cw, cb = d(sd["classifier.rel_predictor.weight"]), d(sd["classifier.rel_predictor.bias"])
    assert hw.shape[0] == 12
    feats = tspn.hashrng.uniform(7, "x", (B * N, T, D), -1, 1)
    trk, frame = 4, T - 1                                              # the last own frame of the tracklet's last sextet
    feats[trk, frame, 13] = -1000.0
    feats = torch.from_numpy(feats).to(device).contiguous()
    pairs = torch.cat([tspn.ops.pair_index(N, device, base=b * N) for b in range(B)])
    packed = tspn.ops.pack_conv3_wino63_f16x3(conv_w, split=D)
    need = tspn.ops.fused_workspace_bytes(B, N, T, D, 4, cw.shape[0], pairs.shape[0], conv_algo=tspn._abi.CONV_WINOGRAD63_F16X3)
    words = tspn.ops.status_words(device)
    got = []
    for form in (1, 2):
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        words[tspn._abi.STATUS_CONV_ERR] = 0
        words[tspn._abi.STATUS_CONV_CHECKS] = 0
        with input_form(tspn, form):
            heads, logits = tspn.ops.forward_fused(feats, pairs, B, N, packed, conv_b, hw, hb, cw, cb, workspace=ws,
                                                   canonical_pairs=True, conv_weight=conv_w, conv_check=4 * D)
        torch.cuda.synchronize(device)
        scratch = ws[need - tspn._abi.CONV_CHECK_SCRATCH_BYTES:].view(torch.int64)
        key = int(scratch[tspn._abi.CONV_CHECK_HOT_OFFSET // 8::32][:64].cpu().numpy().astype(np.uint64).max())
        got.append((heads, logits, key, int(words[tspn._abi.STATUS_CONV_ERR])))
    words[tspn._abi.STATUS_CONV_ERR] = 0
    words[tspn._abi.STATUS_CONV_CHECKS] = 0
    (h1, l1, k1, e1), (h2, l2, k2, e2) = got
    assert torch.equal(h1.view(torch.int32), h2.view(torch.int32))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    nq = -(-T // 6)
    assert k1 == k2 and k1 & 0xFFFFFFFF == trk * nq + frame // 6
    assert e1 == e2 and e1 != 0, (e1, e2)
