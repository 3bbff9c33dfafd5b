"""Restatements for the bf16 pair-list stage (csrc/pairlist/), shared by tests/test_pairlist_bf16_host.py and
tests/test_gpu_pairlist_bf16.py: the plan of `tspn_pair_plan_i32` in numpy, the check of a device plan against it, the
pair tables the tests score, and `heads_ref64` of tests/test_gpu_bf16.py restated for a pair list."""
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
