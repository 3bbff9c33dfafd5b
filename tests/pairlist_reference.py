"""Restatements for the bf16 pair-list stage (csrc/pairlist/), shared by tests/test_pairlist_bf16_host.py and
tests/test_gpu_pairlist_bf16.py, tests/test_gpu_pairplan_scan.py and tests/test_gpu_pairlist_tiles.py: the plan of
`tspn_pair_plan_i32` in numpy, two checks of a device plan against it (a literal walk for small tables, a vectorised
one for N = 2048 or a million rows), the pair tables the tests score, and `heads_ref64` of tests/test_gpu_bf16.py
restated for a pair list."""
import numpy as np
import torch


def plan_np(pairs, B, N):
    """The plan's order-free content: per video the ascending lists of the distinct subjects / objects that occur,
    their counts, and {(b, rank s, rank o): set of rows} -- rows with an id outside [0, B*N) or ids in two videos are
    in no set."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rows = [[] for _ in range(B)]
    for p, (s, o) in enumerate(pairs):
        if 0 <= s < B * N and 0 <= o < B * N and s // N == o // N:
            rows[s // N].append((p, int(s % N), int(o % N)))
    s_list = [sorted({s for _, s, _ in r}) for r in rows]
    o_list = [sorted({o for _, _, o in r}) for r in rows]
    chains = {}
    for b, r in enumerate(rows):
        for p, s, o in r:
            chains.setdefault((b, s_list[b].index(s), o_list[b].index(o)), set()).add(p)
    counts = np.array([[len(s_list[b]), len(o_list[b])] for b in range(B)], dtype=np.int64).reshape(B, 2)
    return {"s_list": s_list, "o_list": o_list, "counts": counts, "chains": chains}


def check_plan(plan, pairs, B, N):
    """A device plan (dict of arrays: s_list, o_list, counts, head, next) against plan_np: ascending lists, counts, -1 at
    every slot pair outside the table's pairs, and each chain = exactly the set of rows of its pair."""
    ref = plan_np(pairs, B, N)
    P = np.asarray(pairs).reshape(-1, 2).shape[0]
    Np = (N + 15) // 16 * 16
    g = {k: np.asarray(v) for k, v in plan.items()}
    assert g["s_list"].shape == (B, Np) and g["o_list"].shape == (B, Np) and g["head"].shape == (B, Np, Np)
    assert g["counts"].shape == (B, 2) and g["next"].shape == (P,)
    np.testing.assert_array_equal(g["counts"], ref["counts"])
    seen = set()
    for b in range(B):
        ns, no = ref["counts"][b]
        assert g["s_list"][b, :ns].tolist() == ref["s_list"][b] and g["o_list"][b, :no].tolist() == ref["o_list"][b]
        assert ((0 <= g["s_list"][b]) & (g["s_list"][b] < max(N, 1))).all()      # the slots beyond the count too
        assert ((0 <= g["o_list"][b]) & (g["o_list"][b] < max(N, 1))).all()
        for i in range(Np):
            for j in range(Np):
                want = ref["chains"].get((b, i, j))
                p = int(g["head"][b, i, j])
                if want is None:
                    assert p == -1, (b, i, j, p)
                    continue
                got = []
                while p != -1:
                    assert 0 <= p < P and len(got) < len(want), (b, i, j, got, p)
                    got.append(p)
                    p = int(g["next"][p])
                assert set(got) == want and len(got) == len(want), (b, i, j, got, want)
                seen |= want
    off_chain = sorted(set(range(P)) - seen)
    assert all(int(g["next"][p]) == -1 for p in off_chain)
    return ref


def plan_arrays(pairs, B, N, rs=None):
    """A plan in the device layout (int32 arrays) written from plan_np; `rs` (a RandomState) shuffles each chain's order,
    as the link kernel's atomics may."""
    ref = plan_np(pairs, B, N)
    P, Np = np.asarray(pairs).reshape(-1, 2).shape[0], (N + 15) // 16 * 16
    plan = {"s_list": np.zeros((B, Np), np.int32), "o_list": np.zeros((B, Np), np.int32),
            "counts": ref["counts"].astype(np.int32), "head": np.full((B, Np, Np), -1, np.int32),
            "next": np.full((P,), -1, np.int32)}
    for b in range(B):
        plan["s_list"][b, :len(ref["s_list"][b])] = ref["s_list"][b]
        plan["o_list"][b, :len(ref["o_list"][b])] = ref["o_list"][b]
    for key, rows in ref["chains"].items():
        rows = sorted(rows)
        if rs is not None:
            rows = [rows[i] for i in rs.permutation(len(rows))]
        plan["head"][key] = rows[0]
        for a, nx in zip(rows, rows[1:]):
            plan["next"][a] = nx
    return plan


def row_slots(pairs, B, N):
    """Vectorised plan_np: (valid [P] bool, slot [P] int64 = (b * Np + rank s) * Np + rank o of a valid row, -1 of a
    skipped one, present [2,B,max(N,1)] bool, rank [2,B,max(N,1)] = the rank of a tracklet that occurs)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Np, n1 = (N + 15) // 16 * 16, max(N, 1)
    s, o = pairs[:, 0], pairs[:, 1]
    valid = (s >= 0) & (o >= 0) & (s < B * N) & (o < B * N)
    valid &= (np.where(valid, s, 0) // n1) == (np.where(valid, o, 0) // n1)
    vb, ls, lo = s[valid] // n1, s[valid] % n1, o[valid] % n1
    present = np.zeros((2, max(B, 1), n1), dtype=bool)
    present[0, vb, ls] = True
    present[1, vb, lo] = True
    rank = np.cumsum(present, axis=2) - 1
    slot = np.full(pairs.shape[0], -1, dtype=np.int64)
    slot[valid] = (vb * Np + rank[0, vb, ls]) * Np + rank[1, vb, lo]
    return valid, slot, present[:, :B], rank[:, :B]


def check_plan_fast(plan, pairs, B, N):
    """What check_plan checks, order-free and in numpy without a loop over rows or slot pairs (N = 2048 or P = 10^6 in
    well under a second): counts and ascending lists, -1 heads exactly on the slot pairs no valid row names, and the
    chains as a functional graph -- a valid row is pointed at exactly once (by a head or by another row's next), a
    skipped row never and its next is -1, every pointer stays inside its slot pair, each named slot pair has exactly one
    terminal row, and pointer doubling over `next` reaches -1 from everywhere (no cycle).  Together: the rows of a slot
    pair form one path that starts at its head.  Returns the slot of every row (-1 for a skipped one)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P, Np, n1 = pairs.shape[0], (N + 15) // 16 * 16, max(N, 1)
    g = {k: np.asarray(v).astype(np.int64) for k, v in plan.items()}
    assert g["s_list"].shape == (B, Np) and g["o_list"].shape == (B, Np) and g["head"].shape == (B, Np, Np)
    assert g["counts"].shape == (B, 2) and g["next"].shape == (P,)
    valid, slot, present, rank = row_slots(pairs, B, N)
    np.testing.assert_array_equal(g["counts"], present.sum(axis=2).T.reshape(B, 2))
    for side, key in enumerate(("s_list", "o_list")):
        lst = g[key]
        assert ((0 <= lst) & (lst < n1)).all(), f"{key}: a slot outside [0, N)"                # past the count too
        want = np.zeros((B, Np), dtype=np.int64)
        b_of, trk = np.nonzero(present[side])                                                # row-major: ascending per b
        want[b_of, rank[side][b_of, trk]] = trk
        listed = np.arange(Np)[None, :] < g["counts"][:, side][:, None]
        assert (lst[listed] == want[listed]).all(), f"{key}: not the ascending distinct tracklets"
    head, nxt = g["head"].reshape(-1), g["next"]
    assert ((head >= -1) & (head < P)).all() and ((nxt >= -1) & (nxt < P)).all(), "a pointer outside [-1, P)"
    named = np.zeros(head.shape[0], dtype=bool)
    named[slot[valid]] = True
    assert ((head >= 0) == named).all(), "head != -1 must hold exactly on the slot pairs a valid row names"
    assert (nxt[~valid] == -1).all(), "a skipped row has a next"
    at = np.nonzero(head >= 0)[0]
    assert (slot[head[at]] == at).all(), "a head points at a row of another slot pair"
    frm = np.nonzero(nxt >= 0)[0]
    assert (slot[nxt[frm]] == slot[frm]).all(), "a link leaves its slot pair"
    indeg = np.bincount(head[at], minlength=P) + np.bincount(nxt[frm], minlength=P)
    assert (indeg[valid] == 1).all(), "a valid row must be pointed at exactly once"
    assert (indeg[~valid] == 0).all(), "a skipped row is on a chain"
    ends = np.bincount(slot[valid & (nxt == -1)], minlength=head.shape[0])
    assert (ends == named).all(), "each named slot pair has exactly one terminal row"
    ptr = nxt.copy()
    for _ in range(int(np.ceil(np.log2(max(P, 2)))) + 1):                                     # ptr = next^(2^k)
        live = ptr >= 0
        ptr[live] = ptr[ptr[live]]
    assert (ptr == -1).all(), "a cycle"
    return slot


def canonical_table(B, N):
    """All ordered pairs (s != o), i-major, of B videos with global ids: the table of ops.pair_index per video."""
    s, o = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    keep = s != o
    local = np.stack([s[keep], o[keep]], axis=1).astype(np.int64)
    return np.concatenate([local + b * N for b in range(B)]) if B * N else np.zeros((0, 2), np.int64)


def among(tracklets, base=0):
    """All ordered pairs (s != o) among the given tracklets (the proposal filter's table), global ids from `base`."""
    tr = np.asarray(tracklets, dtype=np.int64)
    return np.array([[a, b] for a in tr for b in tr if a != b], dtype=np.int64).reshape(-1, 2) + base


def cross(subjects, objects, base=0):
    """Every (s, o) with s from `subjects` and o from `objects`, s-major, (s, s) rows included: unequal axes."""
    s, o = np.meshgrid(np.asarray(subjects, dtype=np.int64), np.asarray(objects, dtype=np.int64), indexing="ij")
    return np.stack([s.ravel(), o.ravel()], axis=1) + base


def _triple():
    tab = np.tile(among([0, 2, 5]), (3, 1))
    return tab[np.random.RandomState(3).permutation(len(tab))]


SCATTERED17 = [0, 2, 3, 7, 8, 12, 15, 16, 19, 23, 24, 28, 31, 33, 36, 38, 39]
# name -> (B, N, T, C, table): the tables tests/test_gpu_pairlist_bf16.py scores
TABLES = {
    "single_pair": (1, 5, 18, 32, np.array([[3, 1]])),
    "diagonal_rows": (1, 5, 18, 32, np.array([[0, 0], [2, 2], [4, 4], [1, 3], [2, 2]])),
    "every_row_three_times": (1, 6, 18, 32, _triple()),
    "among_17_scattered_of_40": (1, 40, 20, 32, among(SCATTERED17)),        # two ragged tiles per axis
    "no_row_for_the_middle_video": (3, 5, 18, 32, np.concatenate([among([0, 1, 3]), among([2, 4], base=10)])),
    "empty": (2, 5, 18, 32, np.zeros((0, 2), np.int64)),
}
CROSS_VIDEO = (3, 4, np.array([[9, 8], [1, 2], [1, 5], [-1, 2], [2, 12], [11, 8], [1, 2]]))   # (B, N, table)


LONG_CHAIN_N = 20


def long_chain_table():
    """P = 256 * 4096 + 300 rows (the link kernel's grid-stride loop takes a second pass) drawn from the 380 ordered
    pairs (s != o) of one N = 20 video: chains of about 2760 rows, every row also a row of the grid kernel."""
    P = 256 * 4096 + 300
    canon = canonical_table(1, LONG_CHAIN_N)
    return canon[np.random.RandomState(20).randint(0, len(canon), size=P)]


def heads_list_ref64(y, pairs, hw, hb):
    """heads_ref64 of tests/test_gpu_bf16.py for a pair list: y [B*N,T,2C] fp32 torch, pairs int64 [P,2] global ids ->
    [P,H,T] float64 with the kernel's rounding point (fp32 add, ReLU, ONE bf16 rounding, float64 contraction).
    Products and sums elementwise (no BLAS), so a non-finite activation behaves as in the kernel (Inf * 0 = NaN)."""
    C = y.shape[2] // 2
    pairs = torch.as_tensor(np.asarray(pairs), dtype=torch.int64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        a = torch.relu(y[pairs[:, 0], :, :C] + y[pairs[:, 1], :, C:])            # fp32 add, as on the GPU
        a = a.to(torch.bfloat16).double()                                         # [P,T,C]
        out = (a.unsqueeze(1) * hw.double().view(1, hw.shape[0], 1, C)).sum(dim=3)   # [P,H,T]
    return out + hb.double().view(1, -1, 1)
