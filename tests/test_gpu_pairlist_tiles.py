"""The list tile of the bf16 pair-list stage (`ops.heads_pairlist_bf16`) where its subject and object axes differ: unequal
compact extents, dead tiles beside live ones, three videos with different extents in one launch, T around the 16-frame
block, rows of y wider than 2C, chains of thousands of rows, and a non-finite value in the V half.

Operands are `operands()` of tests/test_gpu_pairlist_bf16.py with C <= 96 and H = 12, so its bound carries over unchanged:
an output is one C-term fp32 accumulation of the same operands whatever N, B or the table are (ATOL = 3e-5 against the
float64 restatement).  Against the grid kernel's row of the same (s, o) the requirement is equality of bits."""
import numpy as np
import pytest
import torch

import pairlist_reference as ref
from sentinel_buffers import SENTINEL
from test_gpu_nonfinite import assert_same_nonfinite
from test_gpu_pairlist_bf16 import ATOL, H, canonical_row, grid_rows, operands, run_list

pytestmark = pytest.mark.gpu


def check_vs_fp64_and_grid(tspn, device, shape, table, out=None):
    """Score `table`, compare every row with the float64 restatement and every (s != o) row with the grid kernel's row,
    bit for bit.  Returns the output on the host."""
    B, N, T, C = shape
    y, hw, hb = operands(tspn, *shape)
    got = run_list(tspn, device, y, table, B, N, hw, hb).cpu() if out is None else out
    assert got.shape == (len(table), H, T)
    np.testing.assert_allclose(got.numpy(), ref.heads_list_ref64(y, table, hw, hb).numpy(), rtol=0, atol=ATOL)
    off = torch.from_numpy(table[:, 0] != table[:, 1])
    assert int(off.sum()) > 0
    want = grid_rows(tspn, device, shape)[torch.from_numpy(canonical_row(table[off.numpy()], N))]
    assert torch.equal(got[off], want)
    return got


# ------------------------------------------------------------------------------------------------ unequal axes, <8,16,2>
BIG = (1, 70, 20, 32)
_rs = np.random.RandomState(70)
SUBJECTS50 = np.sort(_rs.permutation(70)[:50])
OBJECTS5 = np.array([3, 20, 41, 55, 69])
TRACKLETS48 = np.sort(_rs.permutation(70)[:48])


def fifty_by_five():
    return ref.cross(SUBJECTS50, OBJECTS5)                     # 4 live subject tiles x 1 object tile, (s, s) rows included


def five_by_fifty():
    return fifty_by_five()[:, ::-1].copy()


def anti_diagonal_blocks():
    """48 tracklets on both axes (3 of the 5 tiles per axis): subject ranks 0..15 pair only with object ranks 32..47 and
    ranks 32..47 only with 0..15.  The middle ranks must occur on both axes to keep their places; they pair among
    themselves, one row each.  Live tiles (0,2), (1,1), (2,0); the diagonal tiles (0,0) and (2,2) and the four tiles
    between the live ones are dead, as is everything past the counts."""
    L = TRACKLETS48
    mid = np.stack([L[16:32], np.roll(L[16:32], -1)], axis=1)
    return np.concatenate([ref.cross(L[:16], L[32:]), mid, ref.cross(L[32:], L[:16])])


@pytest.mark.parametrize("make", [fifty_by_five, five_by_fifty, anti_diagonal_blocks], ids=lambda f: f.__name__)
def test_unequal_axes_big_form(tspn, device, make):
    table = make()
    plan = ref.plan_np(table, 1, 70)
    want = {"fifty_by_five": [50, 5], "five_by_fifty": [5, 50], "anti_diagonal_blocks": [48, 48]}[make.__name__]
    assert plan["counts"].tolist() == [want]
    if make is anti_diagonal_blocks:
        live = {(i // 16, j // 16) for _, i, j in plan["chains"]}
        assert live == {(0, 2), (1, 1), (2, 0)}
    table = table[np.random.RandomState(1).permutation(len(table))]
    check_vs_fp64_and_grid(tspn, device, BIG, table)


# ------------------------------------------------------------------------------------------------ unequal axes, <4,8,2>
def test_unequal_axes_small_form(tspn, device):
    """N = 12: 9 subjects x 2 objects -- two subject tiles of 8 slots (the second with one listed slot), one object tile."""
    table = ref.cross([0, 1, 2, 4, 5, 7, 8, 10, 11], [3, 9])
    assert ref.plan_np(table, 1, 12)["counts"].tolist() == [[9, 2]]
    check_vs_fp64_and_grid(tspn, device, (1, 12, 18, 32), table)


@pytest.mark.parametrize("N", [12, 13])
def test_one_local_table_on_both_sides_of_the_form_switch(tspn, device, N):
    """The same local table at N = 12 (<4,8,2>) and N = 13 (<8,16,2>), each against its own grid launch."""
    table = np.concatenate([ref.cross([0, 1, 2, 4, 5, 7, 8, 10, 11], [3, 9]), ref.cross([11, 6], [0, 10, 11])])
    check_vs_fp64_and_grid(tspn, device, (1, N, 18, 32), table)


# ------------------------------------------------------------------------------------------------ three extents, one launch
def test_three_videos_with_different_compact_extents(tspn, device):
    """N = 40: video 0 names all 40 tracklets (3 tiles per axis), video 1 three, video 2 seventeen; rows shuffled across
    the videos.  The grid is the same 3 x 3 tiles for each: tiles past a video's own counts must be dead."""
    shape = (3, 40, 20, 32)
    table = np.concatenate([ref.among(np.arange(40)), ref.among([5, 22, 39], base=40), ref.among(ref.SCATTERED17, base=80)])
    assert ref.plan_np(table, 3, 40)["counts"].tolist() == [[40, 40], [3, 3], [17, 17]]
    table = table[np.random.RandomState(2).permutation(len(table))]
    check_vs_fp64_and_grid(tspn, device, shape, table)


# ------------------------------------------------------------------------------------------------ T around the frame block
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33])
def test_every_listed_row_is_written_and_nothing_else(tspn, device, T):
    """B = 2, N = 17, 5 x 3 pairs per video, one row that joins the two videos and one out of range, check_pairs=False:
    the output is a view of a sentinel buffer with one spare row."""
    shape = (2, 17, T, 32)
    B, N, _, C = shape
    good = np.concatenate([ref.cross([1, 4, 9, 15, 16], [0, 4, 13]), ref.cross([0, 2, 7, 8, 16], [3, 11, 16], base=N)])
    table = np.concatenate([good[:11], [[3, 20]], good[11:25], [[40, 2]], good[25:]])
    skipped = [11, 26]
    P = len(table)
    assert all(ref.row_slots(table, B, N)[1][p] < 0 for p in skipped) and int((ref.row_slots(table, B, N)[1] < 0).sum()) == 2
    y, hw, hb = operands(tspn, *shape)
    buf = torch.full((P + 1, H, T), SENTINEL, dtype=torch.float32, device=device)
    out = run_list(tspn, device, y, table, B, N, hw, hb, out=buf[:P], check_pairs=False)
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu()
    assert bool((got[P] == SENTINEL).all()), "wrote past the last row"
    assert bool((got[skipped] == SENTINEL).all()), "wrote a skipped row"
    keep = np.array([p for p in range(P) if p not in skipped])
    kept = got[torch.from_numpy(keep)]
    assert int((kept == SENTINEL).sum()) == 0, "rows not fully written"
    check_vs_fp64_and_grid(tspn, device, shape, table[keep], out=kept)


# ------------------------------------------------------------------------------------------------ rows of y wider than 2C
@pytest.mark.parametrize("N", [5, 13])
def test_padded_rows_of_y_give_the_same_bits(tspn, device, N):
    """ldm = 2C + 4: the four extra columns of every row hold NaN; both forms."""
    B, T, C = 2, 18, 32
    y, hw, hb = operands(tspn, B, N, T, C)
    table = np.concatenate([ref.cross([0, 2, 4], [1, 2, N - 1]), ref.cross([N - 1, 1], [0, 3], base=N)])
    want = run_list(tspn, device, y, table, B, N, hw, hb).cpu()
    wide = torch.full((B * N, T, 2 * C + 4), float("nan"), dtype=torch.float32)
    wide[:, :, :2 * C] = y
    got = run_list(tspn, device, wide, table, B, N, hw, hb).cpu()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ long chains
def test_a_million_rows_on_380_chains_equal_the_grid_rows(tspn, device):
    """The long-chain table of tests/test_gpu_pairplan_scan.py scored at T = 1, C = 32: every one of the 256 * 4096 + 300
    rows (50 MB of output) holds the bits of the grid row of its pair; the expected tensor is the 380 grid rows indexed."""
    N = ref.LONG_CHAIN_N
    shape = (1, N, 1, 32)
    table = ref.long_chain_table()
    y, hw, hb = operands(tspn, *shape)
    out = run_list(tspn, device, y, table, 1, N, hw, hb, check_pairs=False)
    grid = grid_rows(tspn, device, shape)
    assert grid.shape == (380, H, 1)
    np.testing.assert_allclose(grid.numpy(), ref.heads_list_ref64(y, ref.canonical_table(1, N), hw, hb).numpy(), rtol=0,
                               atol=ATOL)
    want = grid.to(device)[torch.from_numpy(canonical_row(table, N)).to(device)]
    assert out.shape == want.shape == (len(table), H, 1) and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ confinement, V half
NF_SHAPE = (1, 9, 20, 32)
NF_OBJECT, NF_CHAN = 4, 21
NF_TABLE = np.concatenate([ref.among([1, 4, 6, 8]), [[4, 4], [1, 4], [4, 0], [2, 2]], ref.among([4, 6])])


@pytest.mark.parametrize("frame", [13, 19], ids=["second_piece", "last_frame"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_activation_in_the_v_half_stays_in_its_object_rows_and_frame(tspn, device, value, frame):
    """The plant of test_a_nonfinite_activation_stays_in_its_subject_rows_and_frame on the object side: channel C + c of
    one tracklet's row (the V half: staging offset + C, fragment registers `vq`), at frame 13 (the second 8-frame piece of
    block 0) and at frame T - 1 = 19 (T % 16 = 4: that frame is staged again into the twelve lanes past T)."""
    B, N, T, C = NF_SHAPE
    y, hw, hb = operands(tspn, *NF_SHAPE)
    assert bool((hw[:, NF_CHAN] != 0).all())                      # Inf * w is +-Inf for every head
    clean = run_list(tspn, device, y, NF_TABLE, B, N, hw, hb).cpu()
    y = y.clone()
    y[NF_OBJECT, frame, C + NF_CHAN] = value
    got = run_list(tspn, device, y, NF_TABLE, B, N, hw, hb).cpu()
    assert_same_nonfinite(got.numpy(), ref.heads_list_ref64(y, NF_TABLE, hw, hb).numpy(), ATOL, "planted " + str(value))
    hit = torch.zeros(got.shape, dtype=torch.bool)
    hit[torch.from_numpy(NF_TABLE[:, 1] == NF_OBJECT), :, frame] = True
    assert int(hit.sum()) > 0 and torch.equal(~torch.isfinite(got), hit)
    assert torch.equal(got[~hit], clean[~hit])


@pytest.mark.parametrize("frame", [13, 19], ids=["second_piece", "last_frame"])
def test_inf_times_a_zero_head_weight_in_the_v_half_is_nan(tspn, device, frame):
    """+Inf at channel C + c with column c of the head weights zeroed for heads 1, 5 and 10: NaN in those heads, +-Inf in
    the others, as the float64 restatement has it (products elementwise)."""
    B, N, T, C = NF_SHAPE
    y, hw, hb = operands(tspn, *NF_SHAPE)
    zeroed = [1, 5, 10]
    hw = hw.clone()
    hw[zeroed, NF_CHAN] = 0.0
    clean = run_list(tspn, device, y, NF_TABLE, B, N, hw, hb).cpu()
    y = y.clone()
    y[NF_OBJECT, frame, C + NF_CHAN] = float("inf")
    got = run_list(tspn, device, y, NF_TABLE, B, N, hw, hb).cpu()
    assert_same_nonfinite(got.numpy(), ref.heads_list_ref64(y, NF_TABLE, hw, hb).numpy(), ATOL, "Inf * 0")
    rows = torch.from_numpy(NF_TABLE[:, 1] == NF_OBJECT)
    others = [h for h in range(H) if h not in zeroed]
    assert bool(torch.isnan(got[rows][:, zeroed, frame]).all()) and bool(torch.isinf(got[rows][:, others, frame]).all())
    hit = torch.zeros(got.shape, dtype=torch.bool)
    hit[rows, :, frame] = True
    assert torch.equal(~torch.isfinite(got), hit) and torch.equal(got[~hit], clean[~hit])
