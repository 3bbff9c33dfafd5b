"""Every bf16 head contraction off H = 12: pack_heads_bf16, heads_pairgrid_bf16 (both forms), heads_pairlist_bf16 and the
dense form behind temporal_encoder_heads_bf16 take any H in 1..16; H <= 12 leaves head group 3 idle, H <= 4 three groups,
H = 5, 13 and 15 mask a group in part.

References and bounds are those of tests/test_gpu_bf16.py for the same operands and contraction depth: `heads_ref64` /
`heads_list_ref64` at atol = 3e-5 for the pair stages (C = 32), the float64 restatement of
test_dense_bf16_pieces_ragged_and_errors at 2e-3 / 2e-6 of the output scale for the dense form.  The entries are called
through the C ABI so that the output can be a view of exactly [P, H, T] inside a sentinel buffer with spare rows behind
it: a store to a head h >= H lands in the next frame row or pair row and shows.  head_b has exactly H elements with NaN
in front of and behind them, and the head weights are the first H rows of a [16, C] buffer whose other rows are NaN: a
load past H stays inside the buffer and must not reach the output."""
import numpy as np
import pytest
import torch

import oracle
import pairlist_reference as ref
from sentinel_buffers import SENTINEL, assert_untouched, held, p
from test_gpu_bf16 import heads_ref64, r16, t

pytestmark = pytest.mark.gpu

HEADS = [1, 3, 4, 5, 12, 13, 15, 16]
ATOL = 3e-5
# (B, N): <4,8,2> with two videos, <8,16,2> with two ragged tiles per axis; T % 16 != 0, two frame blocks
PAIR_SHAPES = [(2, 5), (1, 17)]
T, C = 18, 32


def nan_around(x, device, rows_behind=None):
    """`x` on the device as a view into a NaN-filled buffer: 32 NaN in front, and behind it 32 NaN (a vector) or the rows
    up to `rows_behind` (a matrix, 16-byte aligned)."""
    if x.dim() == 1:
        buf = torch.full((x.numel() + 64,), float("nan"), dtype=torch.float32, device=device)
        v = buf[32:32 + x.numel()]
    else:
        buf = torch.full((rows_behind + 1, x.shape[1]), float("nan"), dtype=torch.float32, device=device)
        v = buf[1:1 + x.shape[0]]
    v.copy_(x)
    assert v.is_contiguous()
    return v


def head_operands(tspn, device, Hh, c, seed=83):
    """(hw [H,c] bf16-rounded, hb [H]) on the host, and on the device the packed weights and the guarded bias."""
    hw = r16(tspn.hashrng.normal(seed, "hw", (Hh, c), std=0.1))
    hb = t(tspn.hashrng.normal(seed, "hb", (Hh,), std=0.1))
    packed = tspn.ops.pack_heads_bf16(nan_around(hw, device, rows_behind=16))
    return hw, hb, packed, nan_around(hb, device)


def held_rows(P, Hh, device, frames=T):
    """(buffer, view [P + spare, H, frames]): rows [:P] are the output; behind them spare rows for 16 heads (one row at
    H = 16, sixteen at H = 1), so that a store to any head h < 16 of the last pair lands in sentinel memory."""
    return held((P + (16 + Hh - 1) // Hh, Hh, frames), device)


def assert_rows_written_and_nothing_else(buf, v, P, what):
    b = buf.cpu()
    lo, n = v.storage_offset(), v[:P].numel()
    assert bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()), f"{what}: wrote outside [P, H, T]"
    never = int((b[lo:lo + n] == SENTINEL).sum())
    assert never == 0, f"{what}: {never} of {n} outputs never written"


@pytest.mark.parametrize("Hh", HEADS)
def test_pack_heads_bf16_zeroes_the_rows_from_h_up(tspn, device, Hh):
    c = 64
    hw = tspn.hashrng.normal(81, "hw", (Hh, c), std=0.1)
    got = tspn.ops.pack_heads_bf16(nan_around(t(hw), device, rows_behind=16)).cpu().float().numpy()      # [c/8, 16, 8]
    want = np.zeros((c // 8, 16, 8), np.float32)
    want[:, :Hh] = r16(hw).numpy().reshape(Hh, c // 8, 8).transpose(1, 0, 2)
    np.testing.assert_array_equal(got, want)


_grid = {}


def grid_launch(tspn, device, B, N, Hh):
    """heads_pairgrid_bf16 through the ABI into held rows [P, H, T]; checked once per (B, N, H), shared with the list test."""
    key = (B, N, Hh)
    if key not in _grid:
        y = t(tspn.hashrng.normal(83, "y", (B * N, T, 2 * C), std=1.0))
        hw, hb, packed, hb_dev = head_operands(tspn, device, Hh, C)
        P = B * N * (N - 1)
        buf, v = held_rows(P, Hh, device)
        yd = y.to(device)
        rc = tspn._abi.lib().tspn_heads_pairgrid_bf16(p(yd), 2 * C, B, N, C, T, p(packed), p(hb_dev), Hh, p(v), tspn.ops._stream())
        assert rc == 0, tspn._abi.lib().tspn_last_error()
        _grid[key] = (y, hw, hb, buf, v, v[:P].cpu())
    return _grid[key]


@pytest.mark.parametrize("Hh", HEADS)
@pytest.mark.parametrize("B,N", PAIR_SHAPES)
def test_heads_pairgrid_bf16_vs_fp64_for_every_h(tspn, device, B, N, Hh):
    y, hw, hb, buf, v, out = grid_launch(tspn, device, B, N, Hh)
    P = B * N * (N - 1)
    assert_rows_written_and_nothing_else(buf, v, P, f"grid H={Hh}")
    want = heads_ref64(y, B, N, hw, hb)
    assert out.shape == want.shape == (P, Hh, T)
    np.testing.assert_allclose(out.numpy(), want.numpy(), rtol=0, atol=ATOL)


def scattered_table(B, N):
    """Unequal axes, repeated rows, an (s, s) row, rows of both videos interleaved."""
    subj = [0, 2, 4] if N == 5 else [0, 3, 7, 8, 15, 16]
    obj = [1, 2] if N == 5 else [1, 7, 16]
    tab = np.concatenate([ref.cross(subj, obj, base=b * N) for b in range(B)])
    tab = np.concatenate([tab, tab[::3]])
    return tab[np.random.RandomState(N).permutation(len(tab))]


@pytest.mark.parametrize("Hh", HEADS)
@pytest.mark.parametrize("B,N", PAIR_SHAPES)
def test_heads_pairlist_bf16_vs_fp64_and_the_grid_rows_for_every_h(tspn, device, B, N, Hh):
    y, hw, hb, _, _, grid = grid_launch(tspn, device, B, N, Hh)
    table = scattered_table(B, N)
    P = len(table)
    packed = tspn.ops.pack_heads_bf16(nan_around(hw, device, rows_behind=16))
    buf, v = held_rows(P, Hh, device)
    pairs = torch.from_numpy(table).to(device)
    out = tspn.ops.heads_pairlist_bf16(y.to(device), pairs, B, N, packed, nan_around(hb, device), Hh, out=v[:P])
    assert out.data_ptr() == v.data_ptr()
    assert_rows_written_and_nothing_else(buf, v, P, f"list H={Hh}")
    got = v[:P].cpu()
    np.testing.assert_allclose(got.numpy(), ref.heads_list_ref64(y, table, hw, hb).numpy(), rtol=0, atol=ATOL)
    off = table[:, 0] != table[:, 1]
    b, s, o = table[off, 0] // N, table[off, 0] % N, table[off, 1] % N
    row = b * N * (N - 1) + s * (N - 1) + np.where(o < s, o, o - 1)
    assert int(off.sum()) > 0 and torch.equal(got[torch.from_numpy(off)], grid[torch.from_numpy(row)])


@pytest.mark.parametrize("Hh", HEADS)
def test_temporal_encoder_heads_bf16_vs_fp64_for_every_h(tspn, device, Hh):
    """The shape and the restatement of test_dense_bf16_pieces_ragged_and_errors (P = 5, C = 96, T = 37) at its bounds."""
    P, Cd, Td = 5, 96, 37
    x = tspn.hashrng.uniform(91, "x", (P, Cd, Td), -1, 1)
    cw = tspn.hashrng.normal(91, "cw", (Cd, Cd, 3), std=0.08)
    cb = r16(tspn.hashrng.normal(91, "cb", (Cd,), std=0.1))
    hw = tspn.hashrng.normal(91, "hw", (Hh, Cd), std=0.1)
    hb = r16(tspn.hashrng.normal(91, "hb", (Hh,), std=0.1))
    xt = tspn.ops.transpose_cast_bf16(t(x).to(device))
    conv_packed = tspn.ops.pack_conv3_bf16(t(cw).to(device))
    packed = tspn.ops.pack_heads_bf16(nan_around(t(hw), device, rows_behind=16))
    y_ws = torch.empty((P, Td, Cd), dtype=torch.float32, device=device)
    buf, v = held_rows(P, Hh, device, frames=Td)
    cbd = cb.to(device)
    rc = tspn._abi.lib().tspn_temporal_encoder_heads_bf16(p(xt), P, Cd, Td, p(conv_packed), p(cbd), p(packed),
                                                          p(nan_around(hb, device)), Hh, p(y_ws), p(v), tspn.ops._stream())
    assert rc == 0, tspn._abi.lib().tspn_last_error()
    b = buf.cpu()
    lo, n = v.storage_offset(), v[:P].numel()
    assert bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()) and int((b[lo:lo + n] == SENTINEL).sum()) == 0
    out = v[:P].cpu()
    h = torch.nn.functional.conv1d(r16(x).double(), r16(cw).double(), cb.double(), padding=1)
    h = oracle.bf16_round(torch.relu(h).float()).double()
    exp = torch.einsum("hc,pct->pht", r16(hw).double(), h) + hb.double()[None, :, None]
    scale = float(exp.abs().max())
    assert float((out.double() - exp).abs().max()) <= 2e-3 * scale
    assert float((out.double() - exp).abs().mean()) <= 2e-6 * scale


@pytest.mark.parametrize("Hh", [0, 17])
def test_h_outside_1_to_16_is_refused_with_outputs_untouched(tspn, device, Hh):
    lib, EINVAL = tspn._abi.lib(), tspn._abi.TSPN_EINVAL
    B, N = 1, 5
    P = N * (N - 1)
    y = torch.zeros((N, T, 2 * C), device=device)
    w = torch.zeros((17, C), device=device)
    bias = torch.zeros(17, device=device)
    good = tspn.ops.pack_heads_bf16(w[:12])
    stream = tspn.ops._stream()
    buf, v = held((C // 8, 16, 8), device, dtype=torch.bfloat16)
    assert lib.tspn_pack_heads_bf16(p(w), Hh, C, p(v), stream) == EINVAL
    assert_untouched(buf, f"pack_heads H={Hh}")
    buf, v = held((P, 17, T), device)
    assert lib.tspn_heads_pairgrid_bf16(p(y), 2 * C, B, N, C, T, p(good), p(bias), Hh, p(v), stream) == EINVAL
    assert_untouched(buf, f"grid H={Hh}")
    pairs = tspn.ops.pair_index(N, device)
    ws = torch.zeros(lib.tspn_heads_pairlist_bf16_workspace_bytes(B, N, P), dtype=torch.uint8, device=device)
    assert lib.tspn_heads_pairlist_bf16(p(y), 2 * C, B, N, C, T, p(pairs), P, p(good), p(bias), Hh, p(v), p(ws), ws.numel(),
                                        stream) == EINVAL
    assert_untouched(buf, f"list H={Hh}")
    assert not bool(ws.any()), "a refused call wrote its workspace"
    x = torch.zeros((P, T, C), dtype=torch.bfloat16, device=device)
    conv_packed = tspn.ops.pack_conv3_bf16(torch.zeros((C, C, 3), device=device))
    y_ws = torch.zeros((P, T, C), device=device)
    assert lib.tspn_temporal_encoder_heads_bf16(p(x), P, C, T, p(conv_packed), None, p(good), p(bias), Hh, p(y_ws), p(v),
                                                stream) == EINVAL
    assert_untouched(buf, f"dense H={Hh}")
    with pytest.raises((ValueError, RuntimeError)):
        tspn.ops.pack_heads_bf16(w[:Hh])
