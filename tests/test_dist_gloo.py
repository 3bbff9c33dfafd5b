"""The N>1 path on CPU: world_size-2 gloo processes shard a video list and gather results."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, num_videos, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import tspn_mi355x as tspn
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = tspn.dist.shard_range(num_videos, rank, world)
    # stand-in for the per-video result rows a rank computes (video id encoded in the values)
    local = torch.stack([torch.full((3, 2), float(v)) for v in range(lo, hi)]) if hi > lo \
        else torch.zeros((0, 3, 2))
    out = tspn.dist.gather_results(local, num_videos)
    q.put((rank, lo, hi, out[:, 0, 0].tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("num_videos", [8, 5])
def test_shard_and_gather_world2(num_videos):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, num_videos, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    covered = []
    for rank, lo, hi, vals in sorted(res):
        covered += list(range(lo, hi))
        assert vals == [float(v) for v in range(num_videos)]  # global order restored on every rank
    assert covered == list(range(num_videos))  # disjoint, complete, no pad-by-repeat


def test_shard_range_properties(tspn):
    for n in (0, 1, 7, 512):
        for w in (1, 2, 4, 8):
            r = [tspn.dist.shard_range(n, k, w) for k in range(w)]
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            sizes = [b - a for a, b in r]
            assert max(sizes) - min(sizes) <= 1 and sizes == tspn.dist.shard_counts(n, w)
    with pytest.raises(ValueError):
        tspn.dist.shard_range(4, 2, 2)
    assert tspn.dist.gather_results(torch.ones(2, 3), 2).shape == (2, 3)  # no process group: identity


def _decoded_of(video, m=200, k=256):
    """A video's decoded result rows (deterministic in the video id): what a rank holds after
    forward + decode — top-m (score, triplet, pair) + top-k pair proposals."""
    g = torch.Generator().manual_seed(1000 + video)
    return (torch.rand(m, generator=g).sort(descending=True)[0],
            torch.randint(0, 132, (m, 3), generator=g), torch.randint(0, 32, (m, 2), generator=g),
            torch.randperm(1024, generator=g)[:k])


def _worker_decoded(rank, world, port, num_videos, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import tspn_mi355x as tspn
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = tspn.dist.shard_range(num_videos, rank, world)
    rows = [_decoded_of(v) for v in range(lo, hi)]
    stack = lambda i, shape, dt: torch.stack([r[i] for r in rows]) if rows else torch.zeros((0,) + shape, dtype=dt)  # noqa: E731
    out = tspn.dist.gather_decoded(stack(0, (200,), torch.float32), stack(1, (200, 3), torch.int64),
                                   stack(2, (200, 2), torch.int64), num_videos,
                                   pair_proposals=stack(3, (256,), torch.int64))
    ok = True
    for v in range(num_videos):   # every rank holds every video's rows, bit for bit, in global order
        sc, tr, pt, pp = _decoded_of(v)
        ok = ok and torch.equal(out["scores"][v], sc) and torch.equal(out["triplets"][v], tr) \
            and torch.equal(out["pair_tids"][v], pt) and torch.equal(out["pair_proposals"][v], pp)
    q.put((rank, ok, tuple(out["scores"].shape), out["triplets"].dtype == torch.int64))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("num_videos", [8, 5, 1])
def test_gather_of_decoded_results_world2(num_videos):
    """The real payload of the N>1 step (bench.py, predict.py:106-116): packed decoded rows cross the
    pad-to-max all-gather (ragged shards for 5 and 1 videos: rank 1 may hold none) and come back typed."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_decoded, args=(r, 2, port, num_videos, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, shape, typed in res:
        assert ok and shape == (num_videos, 200) and typed


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` alone must start 2 ranks itself (VERDICT r1 missing #2): rehearsed on the
    CPU with --launch-check (gloo rendezvous + rank-count assertion + one gather, no GPU work); a rank
    count that disagrees with --gpus must fail loudly, not time one GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1 and json.loads(line[0]) == {"launch_check": True, "n_gpus": 2, "gpus_flag": 2}
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, env=env2)
    assert r.returncode != 0 and "--gpus 4" in (r.stderr + r.stdout)


def test_bench_rank_body_world2_with_stubbed_gpu_step():
    """the REAL rank body of bench.py on two gloo ranks — self-launch of torch.distributed.run,
    rendezvous, warm-up, barrier-bracketed timed loop with the decoded-result all-gather in every step, the
    max-over-ranks time (all_reduce MAX), the `gathered[lo:hi] == local` check on every rank, ONE JSON
    line from rank 0 — with only the GPU step replaced by recorded decoded rows (`--stub-gpu`).  Whole-job value =
    world x units per step x steps / max time."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--stub-gpu", "--steps", "4",
                        "--warmup", "1", "--videos", "3"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["stub"] is True and out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 1
    assert out["scaling"] == "weak" and out["unit"] == "tracklet-pairs/s" and out["roofline"] is None
    assert "cpu_baseline" not in out
    pairs = 2 * 3 * 32 * 31 * 4      # world x videos x N(N-1) x steps
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * 4 - pairs) < 1e-6 * pairs
    # one rank through the same body (no collective unless forced), and the forced collective on one rank
    for extra in ([], ["--force-collective"]):
        r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--stub-gpu", "--steps", "2", "--warmup", "1"]
                            + extra, capture_output=True, text=True, timeout=300, env=env)
        assert r1.returncode == 0, r1.stderr[-3000:]
        assert json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][0])["n_gpus"] == 1


def test_bench_dump_outputs_through_the_stubbed_rank_body(tmp_path):
    """`--dump-outputs DIR` writes the last step's results as float32 / float64 .npy files, the same from run to run with
    the same arguments; with two ranks rank 0 adds the all-gathered rows.  A plain run carries no CPU baseline."""
    import numpy as np
    for run in ("a", "b"):
        out = _run_bench("--stub-gpu", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / run))
        assert "cpu_baseline" not in out and "secondary" not in out and out["ms_per_step"] > 0
    a = {p.name: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.name: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert set(a) == {"scores.npy", "triplets.npy", "pair_tids.npy", "pair_proposals.npy"} == set(b)
    assert a["scores.npy"].dtype == np.float32 and a["triplets.npy"].dtype == np.float64
    assert a["triplets.npy"].shape == (4, 200, 3) and all(np.array_equal(a[k], b[k]) for k in a)
    _run_bench("--gpus", "2", "--stub-gpu", "--steps", "2", "--warmup", "1", "--videos", "3",
               "--dump-outputs", str(tmp_path / "w2"))
    g = np.load(tmp_path / "w2" / "gathered_scores.npy")
    assert g.shape == (6, 200) and np.array_equal(g[:3], np.load(tmp_path / "w2" / "scores.npy"))


def _run_bench(*flags, timeout=600):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["OMP_NUM_THREADS"] = "1"          # eight rank processes on this container's eight cores
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + list(flags), capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_rank_body_world8_ragged_shard_with_per_rank_diagnosis():
    """the rank body on EIGHT gloo ranks with a video count that does not divide (509 over 8 =
    5 x 64 + 3 x 63, dist.shard_range): the pad-to-max all-gather restores global order on every rank (checked inside
    bench.py: gathered[lo:hi] == local), the whole-job value counts the 509 videos once, and rank 0's line carries every
    rank's own ms_per_step and its time inside the collective."""
    out = _run_bench("--gpus", "8", "--stub-gpu", "--steps", "3", "--warmup", "1", "--total-videos", "509")
    assert out["stub"] is True and out["n_gpus"] == 8 and out["config"]["videos_per_step"] == 509
    pr = out["per_rank"]
    assert pr["units_per_step"] == [64 * 992] * 5 + [63 * 992] * 3
    assert len(pr["ms_per_step"]) == 8 and len(pr["gather_ms"]) == 8
    assert pr["ms_per_step_max"] <= out["ms_per_step"] * (1 + 1e-9) and pr["ms_per_step_min"] > 0
    assert all(0 < g <= m * (1 + 1e-9) for g, m in zip(pr["gather_ms"], pr["ms_per_step"]))
    pairs = 509 * 32 * 31 * 3
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * 3 - pairs) < 1e-6 * pairs


def test_bench_rank_body_cfg5_shape_one_video_per_rank():
    """cfg5's N > 1 form (one VidOR-scale video of 64 tracklets per rank per step) through the same rank body, four
    gloo ranks; and a shard that leaves one rank of three with a single video while the others hold two."""
    out = _run_bench("--gpus", "4", "--stub-gpu", "--workload", "cfg5", "--steps", "2", "--warmup", "1")
    assert out["n_gpus"] == 4 and out["config"]["videos_per_gpu_per_step"] == 1 and out["config"]["videos_per_step"] == 4
    assert out["per_rank"]["units_per_step"] == [64 * 63] * 4
    pairs = 4 * 64 * 63 * 2
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * 2 - pairs) < 1e-6 * pairs
    out = _run_bench("--gpus", "3", "--stub-gpu", "--steps", "2", "--warmup", "0", "--total-videos", "5")
    assert out["per_rank"]["units_per_step"] == [2 * 992, 2 * 992, 1 * 992]


def test_bench_refuses_more_ranks_than_devices():
    """`--gpus N` on a node that shows fewer HIP devices must stop with a clear message before any launch."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    assert "HIP device(s) are visible" in src and "torch.cuda.device_count() < local_world" in src
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    # here (no GPU at all) the non-stub body stops earlier, with the no-CPU-fallback message
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    if not torch.cuda.is_available():
        assert r.returncode != 0 and "needs a HIP device" in r.stderr
