"""The software-pipelined k-step of the split-fp16 F(6,3) contraction (tspn_wino63.hip, `wino63_f16x3_tile`) through
the C entry tspn_conv3_tc_wino63_f16x3, at the smallest shapes at which the pipeline can go wrong.

The ring of four LDS stages runs on across the 8 points, the fragments of k-step g + 1 are read under the third product
group of k-step g into a second register set, and the DMA pieces go out as buffer loads or with 64-bit pointers.  A
stale, half-landed or too early refilled stage counts one k-step twice and drops another: with random operands that is
orders of magnitude above the bounds of tests/test_gpu_wino63_f16x3.py, which are asserted here: 64 eps sum|x||w| per
output and 2e-5 max|y|.

  Cin = 32, 64, 96      nk = 2, 4, 6 k-steps per point: a point ends at another ring stage and, for the k-steps of the
                        next point, another parity of the register sets in each of the three
  (B, T) = (1, 5), (3, 150), (11, 150)   1, 75 and 275 sextets: one partly filled sextet tile; a full and a partly
                        filled one.  T = 5 takes the scalar stores.
  M = 256, 512          one row tile; two (the second one's lane offsets start 256 rows into every slab).  The entry takes
                        whole row tiles only (M % 256 == 0), so there is no partly filled row tile to clamp: M = 32 and
                        M = 288 are refused before anything is launched, which is asserted too.
  piece form 0, 1       every case under both, bit for bit the same
  tail split 1, 0       these grids have fewer tiles than the device has CUs, so with the split on every tile runs as
                        sub-tiles and with it off as full tiles: both bodies, bit for bit the same
"""
import numpy as np
import pytest
import torch

import sentinel_buffers as sb
from test_gpu_wino63_f16x3 import conv_ref, t

pytestmark = pytest.mark.gpu

CINS = (32, 64, 96)
MS = (256, 512)
BTS = ((1, 5), (3, 150), (11, 150))
M_MAX = max(MS)

_operands = {}


def operands(tspn, Cin, B, T):
    """(x, w, b, float64 conv, sum|x||w| + |b|) at M_MAX rows; a smaller M takes the first rows.  Made once per shape."""
    key = (Cin, B, T)
    if key not in _operands:
        x = tspn.hashrng.uniform(171, f"x{key}", (B, T, Cin), -1, 1)
        w = tspn.hashrng.normal(171, f"w{Cin}", (M_MAX, Cin, 3), std=0.1)
        b = tspn.hashrng.normal(171, "b", (M_MAX,), std=0.1)
        ref = conv_ref(x, w, b)
        mag = conv_ref(np.abs(x), np.abs(w), np.abs(b))
        _operands[key] = (x, w, b, ref, mag)
    return _operands[key]


def launch(tspn, x, pk, M, bias, relu, ws=None):
    """tspn_conv3_tc_wino63_f16x3 into a sentinel-filled buffer -> (buffer, y [B, M, T])."""
    B, T, Cin = x.shape
    lib = tspn._abi.lib()
    if ws is None:
        ws = torch.empty(max(lib.tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M), 256), dtype=torch.uint8,
                         device=x.device)
    buf, y = sb.held((B, M, T), x.device)
    rc = lib.tspn_conv3_tc_wino63_f16x3(sb.p(x), B, T, Cin, sb.p(pk), M, sb.p(bias), int(relu), sb.p(y), sb.p(ws),
                                        ws.numel(), tspn.ops._stream())
    return rc, buf, y


def assert_bounds(y, ref, mag, what):
    e = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    r = float((e / (2.0 ** -24 * mag + 1e-300)).max())
    rel = float(e.max() / np.abs(ref).max())
    print(f"{what}: max error {e.max():.3g} = {r:.3g} eps sum|x||w|, {rel:.3g} max|y|")
    assert r <= 64.0, f"{what}: {r:.3g} eps sum|x||w|"
    assert rel <= 2e-5, f"{what}: {rel:.3g} max|y|"


class settings:
    """Piece form and tail split of the process, put back on exit."""

    def __init__(self, tspn):
        self.ops = tspn.ops

    def __enter__(self):
        self.form = self.ops.wino63_set_piece_form(0)
        self.split = self.ops.wino63_f16x3_set_tail_split(1)
        return self

    def set(self, form, split):
        self.ops.wino63_set_piece_form(form)
        self.ops.wino63_f16x3_set_tail_split(split)

    def __exit__(self, *exc):
        self.ops.wino63_set_piece_form(self.form)
        self.ops.wino63_f16x3_set_tail_split(self.split)


@pytest.mark.parametrize("B,T", BTS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("Cin", CINS)
def test_pipeline_against_float64_under_both_piece_forms(tspn, device, Cin, M, B, T):
    x, w, b, ref, mag = operands(tspn, Cin, B, T)
    xd, bd = t(x).to(device), t(b[:M]).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w[:M]).to(device))
    outs = {}
    with settings(tspn) as s:
        for form in (0, 1):
            for split in (1, 0):
                s.set(form, split)
                rc, buf, y = launch(tspn, xd, pk, M, bd, False)
                assert rc == 0
                sb.assert_written_inside_only(buf, y, f"form {form} split {split}")
                outs[(form, split)] = y
    what = f"Cin={Cin} M={M} B={B} T={T}"
    assert_bounds(outs[(0, 1)], ref[:, :M], mag[:, :M], what)
    for key, y in outs.items():
        assert torch.equal(y.view(torch.int32), outs[(0, 1)].view(torch.int32)), \
            f"{what}: (piece form, tail split) = {key} differs from (0, 1)"


@pytest.mark.parametrize("M", [32, 288])
def test_rows_that_are_no_whole_tile_are_refused_before_any_launch(tspn, device, M):
    B, T, Cin = 3, 150, 32
    x = torch.zeros((B, T, Cin), device=device)
    pk = torch.zeros((8, 2 * Cin // 8 + 1, M, 8), dtype=torch.int16, device=device)
    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device=device)
    with pytest.raises(ValueError):
        tspn.ops.pack_conv3_wino63_f16x3(torch.zeros((M, Cin, 3), device=device))
    for form in (0, 1):
        with settings(tspn) as s:
            s.set(form, 1)
            rc, buf, _ = launch(tspn, x, pk, M, None, False, ws)
        sb.refused(tspn, rc, tspn._abi.TSPN_EUNSUPPORTED, f"M={M} form {form}")
        torch.cuda.synchronize(device)
        sb.assert_untouched(buf, f"M={M} form {form}")
        assert not bool(ws.any()), "a refused call wrote to the workspace"


def test_pipeline_is_deterministic_and_stays_inside_y(tspn, device):
    """The largest case five times, into fresh sentinel-filled outputs, full tiles and sub-tiles."""
    Cin, M, (B, T) = CINS[-1], M_MAX, BTS[-1]
    x, w, b, ref, mag = operands(tspn, Cin, B, T)
    xd, bd = t(x).to(device), t(b).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w).to(device))
    with settings(tspn) as s:
        for split in (1, 0):
            s.set(0, split)
            ys = []
            for k in range(5):
                rc, buf, y = launch(tspn, xd, pk, M, bd, False)
                assert rc == 0
                sb.assert_written_inside_only(buf, y, f"split {split} launch {k}")
                ys.append(y)
            assert all(torch.equal(y.view(torch.int32), ys[0].view(torch.int32)) for y in ys[1:]), f"split {split}"
    assert_bounds(ys[0], ref, mag, "fifth run")


def test_pipeline_with_and_without_bias_and_relu(tspn, device):
    Cin, M, (B, T) = 64, 256, BTS[1]
    x, w, b, _, _ = operands(tspn, Cin, B, T)
    xd = t(x).to(device)
    pk = tspn.ops.pack_conv3_wino63_f16x3(t(w[:M]).to(device))
    with settings(tspn) as s:
        for split in (1, 0):
            s.set(0, split)
            for bias in (b[:M], None):
                for relu in (False, True):
                    rc, buf, y = launch(tspn, xd, pk, M, None if bias is None else t(bias).to(device), relu)
                    assert rc == 0
                    what = f"split {split} bias {bias is not None} relu {relu}"
                    sb.assert_written_inside_only(buf, y, what)
                    ref = conv_ref(x, w[:M], bias, relu)
                    mag = conv_ref(np.abs(x), np.abs(w[:M]), None if bias is None else np.abs(bias))
                    assert_bounds(y, ref, mag, what)
