"""Tail split of the split-fp16 F(6,3) contraction (tspn_wino63.hip, tspn_conv3_tc_wino63_f16x3_set_tail_split).

The contraction runs one 256 x 256 tile per CU at a time; the R = tiles mod CUs tiles of the last round are cut into
f = min(4, CUs / R) tiles of 256 x 256 / f when f >= 2.  Every output element keeps its operands and their order, so the
launch with the split must equal the launch without it bit for bit.  The grids are chosen from the device's CU count so
that f = 4, f = 2, no split (R > CUs / 2), R = 0 and tiles < CUs (every tile cut) all occur, at T = 150 / 149 / 7,
Cin = 64 / 2048, M = 256 / 8192, with the 8-byte and the scalar stores, into a sentinel-filled y.  The reference is the
float64 conv on sampled tracklets and rows (first and last ones: full tiles and cut tiles) at the bounds of
tests/test_gpu_wino63_f16x3.py: 64 eps sum|x||w| per output, and 6e-5 absolute (Cin = 64, x in [-1, 1), w ~ 0.1 N) or
3e-5 absolute and 2e-5 max|y| (Cin = 2048, the benchmark's distribution)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -3.0e33
F_BM = F_BN = 256


def split_factor(tiles, cus):
    """The launcher's rule: (R, f)."""
    r = tiles % cus
    if r == 0 or cus // r < 2:
        return r, 1
    return r, 4 if cus // r >= 4 else 2


SCENARIOS = {
    "f4": lambda tiles, cus: tiles > cus and split_factor(tiles, cus)[1] == 4,
    "f2": lambda tiles, cus: tiles > cus and split_factor(tiles, cus)[1] == 2,
    "none": lambda tiles, cus: tiles > cus and 2 * split_factor(tiles, cus)[0] > cus,
    "r0": lambda tiles, cus: tiles % cus == 0,
    "small": lambda tiles, cus: tiles < cus and split_factor(tiles, cus)[1] >= 2,
}


def grid_for(scenario, tiles_m, cus):
    """Smallest number of sextet tiles whose grid is of the scenario's kind (None if this CU count has none)."""
    for tiles_n in range(1, 4 * cus + 2):
        if SCENARIOS[scenario](tiles_m * tiles_n, cus):
            return tiles_n
    return None


_weights = {}


def weights(tspn, device, M, Cin):
    """(w on the device, packed); the benchmark's distribution at Cin = 2048, that of test_gpu_wino63_f16x3 at 64."""
    if (M, Cin) not in _weights:
        _weights.clear()                                  # one set at a time: 200 MB at M = 8192, Cin = 2048
        g = torch.Generator(device=device).manual_seed(1000 + M + Cin)
        w = torch.randn((M, Cin, 3), generator=g, device=device) * (0.01 if Cin == 2048 else 0.1)
        _weights[(M, Cin)] = (w, tspn.ops.pack_conv3_wino63_f16x3(w))
    return _weights[(M, Cin)]


def make_x(device, B, T, Cin, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.rand((B, T, Cin), generator=g, device=device)
    return x if Cin == 2048 else 2.0 * x - 1.0


def launch(tspn, x, pk, M, bias, offset, ws):
    """tspn_conv3_tc_wino63_f16x3 into a sentinel-filled buffer; y starts 32 + offset floats in (offset 1: not 8-byte
    aligned, the scalar stores).  Returns (buffer, y)."""
    B, T, Cin = x.shape
    n = B * M * T
    buf = torch.full((n + 64 + offset,), SENTINEL, dtype=torch.float32, device=x.device)
    y = buf[32 + offset:32 + offset + n].view(B, M, T)
    assert y.data_ptr() % 8 == (4 if offset else 0)
    p = tspn.ops._p
    tspn._abi.check(tspn._abi.lib().tspn_conv3_tc_wino63_f16x3(p(x), B, T, Cin, p(pk), M, p(bias), 0, p(y), p(ws), ws.numel(),
                                                               tspn.ops._stream()))
    return buf, y


def workspace(tspn, device, B, T, Cin, M):
    need = tspn._abi.lib().tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M)
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


def ref64(x, w, bias, tracklets, rows):
    """float64 conv and sum |x||w| (+ |bias|) on the sampled tracklets and rows: [len(tracklets), len(rows), T]."""
    xs = x[tracklets].double().cpu().transpose(1, 2)
    ws, bs = w[rows].double().cpu(), bias[rows].double().cpu()
    ref = torch.nn.functional.conv1d(xs, ws, bs, padding=1)
    mag = torch.nn.functional.conv1d(xs.abs(), ws.abs(), bs.abs(), padding=1)
    return ref.numpy(), mag.numpy()


def check_against_float64(y, x, w, bias, what):
    B, M = y.shape[0], y.shape[1]
    tracklets = sorted({0, B // 2, max(B - 2, 0), B - 1})
    rows = sorted({0, 1, 255, M // 2, M - 256, M - 3, M - 1})
    ref, mag = ref64(x, w, bias, tracklets, rows)
    got = y[tracklets][:, rows].double().cpu().numpy()
    e = np.abs(got - ref)
    r = (e / (2.0 ** -24 * mag + 1e-300)).max()
    print(f"{what}: max error {e.max():.3g} = {r:.3g} eps sum|x||w|, {e.max() / np.abs(ref).max():.3g} max|y|")
    assert r <= 64.0, f"{what}: {r:.3g} eps sum|x||w|"
    if x.shape[2] == 2048:
        assert e.max() <= 3e-5 and e.max() <= 2e-5 * np.abs(ref).max(), f"{what}: max error {e.max():.3g}"
    else:
        assert e.max() <= 6e-5, f"{what}: max error {e.max():.3g}"


def check_sentinels(buf, y, what):
    n = y.numel()
    edge = torch.cat([buf[:buf.numel() - n - 32], buf[buf.numel() - 32:]])
    assert bool((edge == SENTINEL).all()), f"{what}: wrote outside y"
    assert not bool((y == SENTINEL).any()), f"{what}: outputs never written"


@pytest.fixture
def split_on(tspn):
    """The process-wide switch is on by default and is left on."""
    assert tspn.ops.wino63_f16x3_set_tail_split(1) == 1
    yield
    tspn.ops.wino63_f16x3_set_tail_split(1)


@pytest.mark.parametrize("scenario", ["f4", "f2", "none", "r0", "small"])
@pytest.mark.parametrize("M", [256, 8192])
@pytest.mark.parametrize("Cin", [64, 2048])
@pytest.mark.parametrize("T", [150, 149, 7])
def test_tail_split_is_bit_identical_and_within_the_float64_bounds(tspn, device, split_on, T, Cin, M, scenario):
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    tiles_m, nq = M // F_BM, -(-T // 6)
    tiles_n = grid_for(scenario, tiles_m, cus)
    assert tiles_n is not None, f"no grid of kind {scenario} with {tiles_m} row tiles on {cus} CUs"
    B = tiles_n * F_BN // nq                      # the last sextet tile is full or has padded columns at its end
    assert -(-(B * nq) // F_BN) == tiles_n
    R, f = split_factor(tiles_m * tiles_n, cus)
    what = f"{scenario} T={T} Cin={Cin} M={M} B={B} tiles={tiles_m * tiles_n} CUs={cus} R={R} f={f}"
    w, pk = weights(tspn, device, M, Cin)
    g = torch.Generator(device=device).manual_seed(7)
    bias = torch.randn((M,), generator=g, device=device) * 0.05
    x = make_x(device, B, T, Cin, 2000 + T)
    ws = workspace(tspn, device, B, T, Cin, M)
    for offset in (0, 1):                         # T = 150: 8-byte stores, then scalar stores; odd T: scalar both times
        buf_on, y_on = launch(tspn, x, pk, M, bias, offset, ws)
        assert tspn.ops.wino63_f16x3_set_tail_split(0) == 1
        buf_off, y_off = launch(tspn, x, pk, M, bias, offset, ws)
        assert tspn.ops.wino63_f16x3_set_tail_split(1) == 0
        torch.cuda.synchronize(device)
        check_sentinels(buf_on, y_on, what + " (split)")
        check_sentinels(buf_off, y_off, what + " (whole tiles)")
        assert torch.equal(y_on, y_off), f"{what} offset={offset}: split and whole-tile launches differ"
        check_against_float64(y_on, x, w, bias, f"{what} offset={offset} (split)")
        check_against_float64(y_off, x, w, bias, f"{what} offset={offset} (whole tiles)")
        del buf_on, y_on, buf_off, y_off


def test_tail_split_repeated_launches_are_bit_identical_at_the_cfg2_shape(tspn, device, split_on):
    """16 videos x 32 tracklets, T = 150, D = 2048, 2C = 8192 rows: 1600 tiles.  24 more launches equal the first."""
    B, T, Cin, M = 512, 150, 2048, 8192
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    print(f"cfg2 shape on {cus} CUs: (R, f) = {split_factor(M // F_BM * -(-(B * 25) // F_BN), cus)}")
    w, pk = weights(tspn, device, M, Cin)
    x = make_x(device, B, T, Cin, 3000)
    ws = workspace(tspn, device, B, T, Cin, M)
    _, first = launch(tspn, x, pk, M, None, 0, ws)
    for k in range(24):
        _, y = launch(tspn, x, pk, M, None, 0, ws)
        assert torch.equal(y, first), f"launch {k + 2} differs from the first"
        del y
    tspn.ops.wino63_f16x3_set_tail_split(0)
    _, whole = launch(tspn, x, pk, M, None, 0, ws)
    tspn.ops.wino63_f16x3_set_tail_split(1)
    assert torch.equal(whole, first)


@pytest.mark.parametrize("T,B", [(150, 20), (7, 300)])
def test_nan_in_a_cut_tile_stays_in_its_sextet(tspn, device, split_on, T, B):
    """Fewer tiles than CUs: every tile is cut.  A NaN in an own frame (not a halo frame) of one sextet reaches that
    sextet's six frames at most; every other output is bit for bit the clean launch's, with and without the split."""
    Cin, M = 64, 256
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    nq = -(-T // 6)
    tiles = -(-(B * nq) // F_BN)
    assert tiles < cus and split_factor(tiles, cus)[1] >= 2
    w, pk = weights(tspn, device, M, Cin)
    x = make_x(device, B, T, Cin, 4000)
    ws = workspace(tspn, device, B, T, Cin, M)
    _, clean = launch(tspn, x, pk, M, None, 0, ws)
    qmax = (T - 3) // 6                                               # last sextet with its third frame inside T
    for b, q in ((0, 0), (B // 2, qmax), (B - 1, qmax // 2)):        # three places in the launch
        frame = 6 * q + 2                                             # in no neighbour's halo (frames 6 q' - 1, 6 q' + 6)
        assert frame + 1 <= T - 1
        bad = x.clone()
        bad[b, frame, 9] = float("nan")
        outs = []
        for on in (1, 0):
            tspn.ops.wino63_f16x3_set_tail_split(on)
            outs.append(launch(tspn, bad, pk, M, None, 0, ws)[1])
        tspn.ops.wino63_f16x3_set_tail_split(1)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        y = outs[0]
        inside = torch.zeros((B, T), dtype=torch.bool, device=device)
        inside[b, 6 * q:6 * q + 6] = True
        outside = ~inside[:, None, :].expand_as(y)
        assert torch.equal(y.view(torch.int32)[outside], clean.view(torch.int32)[outside]), "the NaN left its sextet"
        assert bool(torch.isnan(y[b, :, frame - 1:frame + 2]).all()), "a frame under the NaN's taps is finite"
