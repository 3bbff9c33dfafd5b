"""The plan of the bf16 pair-list stage (`ops.pair_plan`: pair_plan_lists_kernel, pair_plan_link_kernel) past its first
wave, its first stride and its first grid pass, held to `pairlist_reference.check_plan_fast`.

pair_plan_lists_kernel ranks the tracklets that occur with a two-level scan: thread t owns tracklets 2t and 2t + 1, a
wave of 64 threads covers 128 tracklets, and the ranks of a later wave add the totals of the waves before it (`wave_sum`,
`before`), once per side with a barrier in between.  Every N here is >= 128, so that part runs with non-zero values; the
table loop strides by 1024 rows and the link kernel's grid by 256 * 4096 rows, and both are crossed.  Everything asserted
is equality of integers."""
import numpy as np
import pytest
import torch

import pairlist_reference as ref

pytestmark = pytest.mark.gpu

SIZES = [128, 129, 130, 1024, 1025, 2047, 2048]


def device_plan(tspn, device, table, B, N):
    pairs = torch.as_tensor(np.asarray(table), dtype=torch.int64).reshape(-1, 2).to(device)
    plan = tspn.ops.pair_plan(pairs, B, N)
    assert all(v.dtype == torch.int32 for v in plan.values())
    return {k: v.cpu().numpy() for k, v in plan.items()}


def every_tracklet(N):
    i = np.arange(N)
    return np.stack([i, (7 * i + 1) % N], axis=1)              # 7 is coprime to every N of SIZES: all N objects occur


def odd_tracklets(N):
    odd = np.arange(1, N, 2)
    return np.stack([odd, odd[::-1]], axis=1)


def last_tracklet(N):
    return np.array([[N - 1, N - 1]])


def upper_subjects_lower_objects(N):
    """Subjects N//2 .. N-1, objects 0 .. N//2 - 1: the rank of a tracklet differs between the sides, and the waves that
    hold subjects hold no object."""
    k = np.arange(N // 2)
    return np.stack([N - 1 - k, (5 * k + 2) % (N // 2)], axis=1)


def boundary_set(N):
    keep = sorted({x for x in (0, 127, 128, 129, 1023, 1024, 1025, N - 2, N - 1) if 0 <= x < N})
    return ref.cross(keep, keep)


OCCUPANCIES = [every_tracklet, odd_tracklets, last_tracklet, upper_subjects_lower_objects, boundary_set]


@pytest.mark.parametrize("occupancy", OCCUPANCIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("N", SIZES)
def test_ranks_past_the_first_wave(tspn, device, N, occupancy):
    table = occupancy(N)
    got = device_plan(tspn, device, table, 1, N)
    ref.check_plan_fast(got, table, 1, N)
    # the check's own reference, stated once more without it
    assert got["counts"].tolist() == [[len(set(table[:, 0].tolist())), len(set(table[:, 1].tolist()))]]
    assert got["s_list"][0, :got["counts"][0, 0]].tolist() == sorted(set(table[:, 0].tolist()))
    assert got["o_list"][0, :got["counts"][0, 1]].tolist() == sorted(set(table[:, 1].tolist()))


def test_three_videos_with_different_occupancies_and_bad_rows_in_one_launch(tspn, device):
    """B = 3, N = 300 (three waves): video 0 has every tracklet, video 1 no row at all, video 2 the boundary set on the
    subject side and the upper half on the object side; rows interleaved across videos, with negative ids, ids >= B * N
    and rows that join two videos mixed in -- those are on no chain and their next is -1."""
    B, N = 3, 300
    v0 = every_tracklet(N)
    v2 = ref.cross([0, 127, 128, 129, 298, 299], np.arange(150, 300), base=2 * N)
    bad = np.array([[-1, 5], [5, -1], [B * N, 601], [601, B * N + 7], [10, 310], [310, 10], [299, 300], [650, 10],
                    [2 ** 40, 3], [-2 ** 40, -2 ** 40], [301, 302], [5, 599]], dtype=np.int64)      # [301, 302] is video 1
    table = np.concatenate([v0, v2, np.tile(bad, (20, 1))])
    table = table[np.random.RandomState(4).permutation(len(table))]
    in_video_1 = (table[:, 0] == 301).sum()
    table = table[table[:, 0] != 301]                          # ... and taken out again: video 1 has no row
    assert in_video_1 == 20
    got = device_plan(tspn, device, table, B, N)
    slot = ref.check_plan_fast(got, table, B, N)
    assert got["counts"].tolist() == [[300, 300], [0, 0], [6, 150]]
    assert int((slot < 0).sum()) == 11 * 20 and bool((got["next"][slot < 0] == -1).all())
    assert bool((got["head"][1] == -1).all())


@pytest.mark.parametrize("P", [1023, 1024, 1025, 3000])
def test_table_rows_past_the_first_stride(tspn, device, P):
    """Row p names subject p % N, which no earlier row of the first N names: a row the 1024-row stride skipped would be
    a missing list entry and a missing chain."""
    N = 2048
    p = np.arange(P)
    table = np.stack([p % N, (N - 1 - 3 * p) % N], axis=1)
    got = device_plan(tspn, device, table, 1, N)
    ref.check_plan_fast(got, table, 1, N)
    assert got["counts"][0, 0] == min(P, N)


def test_five_thousand_identical_rows_are_one_chain(tspn, device):
    N = 130
    table = np.tile(np.array([[129, 128]]), (5000, 1))
    got = device_plan(tspn, device, table, 1, N)
    ref.check_plan_fast(got, table, 1, N)
    assert got["counts"].tolist() == [[1, 1]] and int((got["head"] >= 0).sum()) == 1
    assert int((got["next"] == -1).sum()) == 1


def test_link_kernel_second_grid_pass_and_long_chains_twice(tspn, device):
    """P = 256 * 4096 + 300: the last 300 rows are linked in the grid-stride loop's second pass; 380 slot pairs with
    chains of about 2760 rows.  Two launches: the order inside a chain may differ, the check does not look at it, and
    everything that is not an order is equal."""
    N, table = ref.LONG_CHAIN_N, ref.long_chain_table()
    P = len(table)
    assert P > 256 * 4096 and len(np.unique(table[:, 0] * N + table[:, 1])) == 380
    a = device_plan(tspn, device, table, 1, N)
    b = device_plan(tspn, device, table, 1, N)
    slot = ref.check_plan_fast(a, table, 1, N)
    assert np.array_equal(slot, ref.check_plan_fast(b, table, 1, N))            # equal chain sets: slot is the table's
    assert np.bincount(slot)[np.unique(slot)].min() > 2000
    for key in ("s_list", "o_list", "counts"):
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(a["head"] >= 0, b["head"] >= 0)
    assert int((a["next"] == -1).sum()) == 380
